"""Every deformable-aggregation path of csrc/daf.hip on inputs whose results are EXACT in float32: the same bits as the float64
restatement (tests/daf_fused_ref.py), whatever the order of summation.

The pixel-major backward adds a pixel row's taps in the order of integer LDS atomics, so on ordinary inputs the last bits of
``grad_mc_ms_feat`` differ from run to run and the other tests judge it by tolerance -- under which one tap dropped or counted
twice beneath a crowded pixel can hide.  Here nothing rounds: the pyramid's sizes are powers of two, the sampling locations are
m / 256 with integer m, the weights, features and output gradients small integers.  Tap fractions are then multiples of 1 / 32,
bilinear coefficients multiples of 1 / 512 at the coarsest level, and every product, partial sum and result a multiple of 1 / 512
far below 2^24 / 512.  The set-up asserts this before it trusts the inputs: the float32 restatement equals the float64 one bit
for bit, and the restatement on the inputs' absolute values (a bound on every partial sum of any order) stays below 2^23 / 512."""
import functools

import pytest
import torch

import daf_fused_ref as ref

pytestmark = pytest.mark.gpu

LEVELS = [(32, 64), (16, 32), (8, 16)]
N_PTS = 12000
K_REG_ITEM = 512     # csrc/daf.hip kRegItem: samples per work item of the region accumulation
K_DAF_CHUNK = 2048   # kDafChunk: taps per work item of the tile accumulation
K_TILE_FLOATS = 8192

# shapes of test_daf_truth_gpu.ARMS that between them reach every kernel of csrc/daf.hip; the kernels are the ones that file's
# comments list.  Every pixel-major mode also runs gf_daf_bwd_kernel<8 | 4, true, false> and its formulation's bucket / scan kernels.
CASES = {
    # gf_daf_fwd4_kernel<8>; region: gf_daf_raccumulate_kernel<32>, tiles: gf_daf_accumulate_kernel<32>, scatter: gf_daf_bwd_kernel<4, true, true>
    "C128_G4": dict(cams=6, C=128, G=4, modes=("region", "tiles", "scatter")),
    # pinned: gf_daf_fwd_grouped_kernel<8>; region: gf_daf_raccumulate_kernel<16>
    "C64_G2": dict(cams=6, C=64, G=2, modes=("pinned", "region")),
    # not region_ok (C / 4 = 64 lanes): gf_daf_accumulate_kernel<64>
    "C256_G8": dict(cams=6, C=256, G=8, modes=("tiles",)),
    # more than 8 cameras: gf_daf_fwd_kernel<4>
    "cams10": dict(cams=10, C=128, G=4, modes=("region",)),
    # (C / G) % 8 != 0: gf_daf_fwd4_kernel<4>; no pixel-major backward, 12 lanes per point: gf_daf_bwd_kernel<4, false, true>
    "C48_G4": dict(cams=6, C=48, G=4, modes=("region",)),
    # gf_daf_fwd_kernel<2>, gf_daf_bwd_kernel<2, false, true>
    "vec2_C24_G4": dict(cams=6, C=24, G=4, modes=("region",)),
    # gf_daf_fwd_kernel<1>, gf_daf_bwd_kernel<1, true, true>
    "vec1_C8_G8": dict(cams=5, C=8, G=8, modes=("region",)),
}
NAMES = ("output", "grad_mc_ms_feat", "grad_sampling_location", "grad_weights")


def _pyramid(dev):
    ss = torch.tensor(LEVELS, dtype=torch.int32)
    sizes = ss[:, 0] * ss[:, 1]
    st = torch.cat([torch.zeros(1, dtype=torch.int32), torch.cumsum(sizes, 0)[:-1].to(torch.int32)])
    return ss.to(dev), st.to(dev), int(sizes.sum())


def _locations(B, cams, g):
    """m [B, N_PTS, cams, 2] (w, h), integers in [-16, 272]: two thirds uniform (0 and 256 sit on the gate, values beyond them
    outside it), a third within +-2 of four centres per camera, each centre in the middle of a region of 8 x 8 level-0 pixels."""
    third = N_PTS // 3
    m = torch.randint(-16, 273, (B, N_PTS, cams, 2), generator=g)
    cw = 14 + 32 * torch.randint(0, 8, (B, cams, 4), generator=g)     # m / 4 - 0.5 = 3 + 8 i: level-0 column 3 of region i
    ch = 28 + 64 * torch.randint(0, 4, (B, cams, 4), generator=g)     # m / 8 - 0.5 = 3 + 8 j
    centre = torch.stack([cw, ch], -1)                                # [B, cams, 4, 2]
    pick = torch.randint(0, 4, (B, third, cams), generator=g)
    bi, ci = torch.arange(B)[:, None, None], torch.arange(cams)[None, None, :]
    m[:, :third] = centre[bi, ci, pick] + torch.randint(-2, 3, (B, third, cams, 2), generator=g)
    return torch.stack([m[b, torch.randperm(N_PTS, generator=g)] for b in range(B)])   # crowded points in every wave


def _assert_crowded(m, C):
    """From the inputs: some region holds more than kRegItem visible samples (a full item and a remainder), and -- where the
    shape takes the pixel-major backward -- some tile of 8192 / C pixel rows receives more than kDafChunk taps (a tile shared
    by several work items: the atomic flush)."""
    B, N, cams, _ = m.shape
    vis = ((m > 0) & (m < 256)).all(-1)
    share = float(vis.float().mean())
    assert 0.7 < share < 0.95, share
    (h0, w0), num_feat = LEVELS[0], sum(h * w for h, w in LEVELS)
    RX, RY = w0 // 8 + 1, h0 // 8 + 1
    wl, hl = (m[..., 0] * w0 - 128) // 256, (m[..., 1] * h0 - 128) // 256      # floor(loc * size - 0.5)
    rx, ry = ((wl + 1).clamp(min=0) >> 3).clamp(max=RX - 1), ((hl + 1).clamp(min=0) >> 3).clamp(max=RY - 1)
    cam = torch.arange(cams)[None, None, :].expand(B, N, cams)
    tile_rows = K_TILE_FLOATS // C
    for b in range(B):
        reg = ((cam[b] * RY + ry[b]) * RX + rx[b])[vis[b]]
        assert int(torch.bincount(reg).max()) > K_REG_ITEM
        if C // 4 not in (16, 32, 64):
            continue
        rows, start = [], 0
        for h, w in LEVELS:
            x0, y0 = (m[b, ..., 0] * w - 128) // 256, (m[b, ..., 1] * h - 128) // 256
            for dy in (0, 1):
                for dx in (0, 1):
                    px, py = x0 + dx, y0 + dy
                    ok = vis[b] & (px >= 0) & (px < w) & (py >= 0) & (py < h)
                    rows.append((cam[b] * num_feat + start + py * w + px)[ok])
            start += h * w
        assert int(torch.bincount(torch.cat(rows) // tile_rows).max()) > K_DAF_CHUNK


def _exact_inputs(B, cams, C, G, seed):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    m = _locations(B, cams, g)
    _assert_crowded(m, C)
    ss, st, num_feat = _pyramid(dev)
    loc = m.float() / 256
    w = torch.randint(0, 4, (B, N_PTS, cams, len(LEVELS), G), generator=g).float()
    feat = torch.randint(-3, 4, (B, cams, num_feat, C), generator=g).float()
    gout = torch.randint(-2, 3, (B, N_PTS, C), generator=g).float()
    args = (feat.to(dev), ss, st, loc.to(dev), w.to(dev), gout.to(dev))
    # the truth, and the conditions under which no order of float32 arithmetic rounds
    truth = ref.daf_chunked(*args, dtype=torch.float64)
    truth32 = ref.daf_chunked(*args, dtype=torch.float32)
    bound = ref.daf_chunked(args[0].abs(), ss, st, args[3], args[4].abs(), args[5].abs(), dtype=torch.float64)
    for name, t, t32, bd in zip(NAMES, truth, truth32, bound):
        grain = 2 if name == "grad_sampling_location" else 512
        assert torch.equal(t.float().double(), t), name                         # representable in float32
        assert torch.equal(t * grain, torch.round(t * grain)), name             # a multiple of 1 / 512 (of 1 / 2)
        assert torch.equal(t32, t.float()), name                                # the float32 restatement: the same bits
        assert float(t.abs().max()) > 0, name
        print(f"  {name:24s} max |truth| * {grain} = {float(t.abs().max()) * grain:.0f}, of absolute inputs {float(bd.abs().max()) * grain:.0f}")
        if name != "grad_sampling_location":
            assert float(bd.abs().max()) < 2 ** 23 / 512, (name, float(bd.abs().max()))
    # grad_sampling_location is made of corner DIFFERENCES, which absolute inputs do not bound, and of coarser numbers: per
    # level, x = weight * sum over the channels of grad_output * (fraction * difference) is a multiple of 1 / 32 (the finest
    # fraction: 8 rows) and at most max|w| * C * max|g| * 2 max|feat|; the gradient adds size * x over the levels, a multiple of
    # 1 / 2 (64 / 8, 32 / 16, 16 / 32 and the same for the heights).  Both stay below 2^23 grains for any inputs of these ranges.
    x_max = float(w.max()) * C * float(gout.abs().max()) * 2 * float(feat.abs().max())
    assert x_max * 32 < 2 ** 23 and sum(max(h, wd) for h, wd in LEVELS) * x_max * 2 < 2 ** 23, x_max
    return args, tuple(t.float() for t in truth)


@functools.lru_cache(maxsize=None)
def _case(name):
    cfg = CASES[name]
    return _exact_inputs(1, cfg["cams"], cfg["C"], cfg["G"], seed=300 + list(CASES).index(name))


def _run(args, mode):
    """(out, grad_feat, grad_loc, grad_weights) of one native path: DAF.apply with the region or the tile backward (the scatter
    where the shape has no pixel-major backward), or forward + gf_daf_backward (``scatter``); ``pinned``: the forward only."""
    from gaussianformer_amd import _lib
    from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF
    from gaussianformer_amd.deformable_aggregation import deformable_aggregation_backward, deformable_aggregation_forward
    feat, ss, st, loc, w, gout = args
    if mode == "pinned":
        with torch.no_grad():
            return (deformable_aggregation_forward(feat, ss, st, loc, w, pin_channel_groups=True),)
    if mode == "scatter":
        with torch.no_grad():
            out = deformable_aggregation_forward(feat, ss, st, loc, w)
            gf, gl, gw = torch.zeros_like(feat), torch.zeros_like(loc), torch.zeros_like(w)
            deformable_aggregation_backward(feat, ss, st, loc, w, gout, gf, gl, gw, pixel_major=False)
        return out, gf, gl, gw
    f, l_, w_ = (t.clone().requires_grad_(True) for t in (feat, loc, w))
    with _lib.option("daf.backward_tiles", 1 if mode == "tiles" else 0):
        out = DAF.apply(f, ss, st, l_, w_)
        out.backward(gout)
    torch.cuda.synchronize()
    return out.detach(), f.grad, l_.grad, w_.grad


def _assert_same_bits(tag, got, truth):
    for name, g, t in zip(NAMES, got, truth):
        diff = g != t
        assert torch.equal(g, t), f"{tag}: {name}: {int(diff.sum())} of {diff.numel()} elements differ, " \
                                  f"max |diff| {float((g.double() - t.double()).abs().max()):.3g}"


@pytest.mark.parametrize("case,mode", [(c, m) for c in CASES for m in CASES[c]["modes"]],
                         ids=[f"{c}-{m}" for c in CASES for m in CASES[c]["modes"]])
def test_exact_inputs_same_bits(case, mode):
    args, truth = _case(case)
    got = _run(args, mode)
    _assert_same_bits(f"{case}/{mode}", got, truth)
    if mode == "pinned":
        assert torch.equal(got[0], _run(args, "region")[0])                    # pinned groups: the same bits as unpinned


def test_exact_inputs_two_batch_elements():
    """B = 2 at C128_G4, other locations in the second element: the pixel-major backward's per-b loop and its reused workspace."""
    cfg = CASES["C128_G4"]
    args, truth = _exact_inputs(2, cfg["cams"], cfg["C"], cfg["G"], seed=399)
    assert not torch.equal(args[3][0], args[3][1])
    for mode in ("region", "tiles"):
        _assert_same_bits(f"B2/{mode}", _run(args, mode), truth)
