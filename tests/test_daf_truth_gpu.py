"""Every deformable-aggregation path against the float64 restatement of the reference (tests/daf_fused_ref.py), ROW BY ROW.

The restatement runs on the GPU in slices of points (``daf_chunked`` / ``block_chunked``), in float64 (the truth) and in float32
(the yardstick of what plain float32 arithmetic of the same formula errs).  ``util.assert_daf_rows_close`` bounds each row -- a
point of the output, a ``(b, cam, pixel)`` row of ``grad_mc_ms_feat``, a ``(b, point, cam)`` row of ``grad_sampling_location`` /
``grad_weights`` -- by max(rtol x max(|ref row|, floor), 4 x the float32 restatement's error on that row), and holds the rows no
visible tap touches to exactly 0.  A tensor-wide bound would let a row under a sparsely sampled pixel be wholly wrong: rows under
crowded pixels are tens of times the typical row (the full-size case asserts more than ten).

Cell edges: the bilinear sample's derivative with respect to its location jumps where a tap coordinate crosses a pixel centre, so
``grad_sampling_location`` (and the key-point gradients built from it) has no float32-resolvable truth for a pair whose tap
coordinate float32 arithmetic may put on the other side of one.  Those pairs (a few per hundred thousand, counted in the printed
``exempt``; where the fused kernels project the key points themselves, the pairs within 1e-4 pixels of an edge, under 1 %) are
judged by the other gradients only; their sample and its weights' gradients are continuous there and stay bounded.  A tap
coordinate EXACTLY on an edge (the arm cases place some) is no such pair: every arithmetic agrees on its side.

(a) full size with projected geometry, (b) one case per dispatch arm of the forward and of the pixel-major backward, (c) the
reference's own fixture (tests/golden/daf_ref.npz, made by tools/make_golden_daf_ref.py)."""
import os

import numpy as np
import pytest
import torch

import daf_fused_ref as ref
from daf_fused_ref import edge_pairs as _edge_pairs, visible_pairs as _visible_pairs
from util import assert_daf_rows_close

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "daf_ref.npz")
FWD_RTOL, GRAD_RTOL = 1e-4, 1e-3
DROP = 0.15


def _cameras(dev, B, cams, yaw0=0.0, wh=(1600.0, 864.0)):
    """A ring of pinhole cameras looking outwards (tests/test_daf_fused_train_gpu.py); batch element b > 0 turned by ``yaw0``
    and moved, so that its points crowd other pixels."""
    pm = torch.eye(4).repeat(B, cams, 1, 1)
    K = torch.tensor([[1260.0, 0, wh[0] / 2], [0, 1260.0, wh[1] / 2], [0, 0, 1.0]])
    for b in range(B):
        for c in range(cams):
            yaw = 2 * np.pi * c / cams + b * yaw0
            R = torch.tensor([[-np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, -1.0], [np.cos(yaw), np.sin(yaw), 0.0]], dtype=torch.float32)
            pm[b, c, :3, :3] = K @ R
            pm[b, c, :3, 3] = K @ torch.tensor([0.3 * b, 1.5 + 0.2 * b, 0.5 * b])
    return pm.to(dev), torch.tensor([[list(wh)] * cams] * B, device=dev)


def _pyramid(levels, dev):
    ss = torch.tensor(levels, dtype=torch.int32)
    sizes = ss[:, 0] * ss[:, 1]
    st = torch.cat([torch.zeros(1, dtype=torch.int32), torch.cumsum(sizes, 0)[:-1].to(torch.int32)])
    return ss.to(dev), st.to(dev), int(sizes.sum())


def _check_daf(name, got, truth, truth32, loc, ss, st, num_feat, forward_only=False):
    """The four results of a DAF.apply-level path (out, grad_feat, grad_loc, grad_weights) row by row; returns the records."""
    print(f"\n[{name}]")
    vis = _visible_pairs(loc)
    recs = {"out": assert_daf_rows_close(got[0], truth[0], truth32[0], f"{name}: output", 2, FWD_RTOL, touched=vis.any(-1))}
    if forward_only:
        return recs
    touched = ref.touched_rows(ss, st, loc, num_feat)
    recs["feat"] = assert_daf_rows_close(got[1], truth[1], truth32[1], f"{name}: grad_mc_ms_feat", 3, GRAD_RTOL, touched=touched)
    recs["loc"] = assert_daf_rows_close(got[2], truth[2], truth32[2], f"{name}: grad_sampling_location", 3, GRAD_RTOL,
                                        touched=vis, exempt=_edge_pairs(loc, ss))
    assert recs["loc"]["exempt"] <= 1e-3 * max(recs["loc"]["touched"], 1000)
    recs["w"] = assert_daf_rows_close(got[3], truth[3], truth32[3], f"{name}: grad_weights", 3, GRAD_RTOL, touched=vis)
    return recs


def _run_daf(feat, ss, st, loc, w, gout, mode="region", pinned=False):
    """One native DAF.apply-level path: ``region`` / ``tiles`` (DAF.apply, pixel-major backward by regions or by tiles where the
    shape allows), ``scatter`` (the reference's atomic formulation, deformable_aggregation_backward(pixel_major=False)), or
    forward only (``pinned``)."""
    from gaussianformer_amd import _lib
    from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF
    from gaussianformer_amd.deformable_aggregation import deformable_aggregation_backward, deformable_aggregation_forward
    if pinned:
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


def _truths(*args):
    return ref.daf_chunked(*args, dtype=torch.float64), ref.daf_chunked(*args, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) full size, projected geometry: 25 600 anchors x 9 key points clustered around their centres, six ring cameras, the
# DAF_LEVELS pyramid, C 128, G 4 (as test_daf_fused_train_gpu.py::test_full_block_shape_gradients_and_memory); and B = 2 at a
# quarter of that, the second element's cameras turned and moved (the backward's per-b loop under crowding).

def _block_case(B, A, seed):
    from gaussianformer_amd.deformable_prepare import deformable_prepare
    from gaussianformer_amd.synthetic import DAF_LEVELS
    dev = torch.device("cuda:0")
    pts, cams, C, G = 9, 6, 128, 4
    levels = [tuple(x) for x in DAF_LEVELS]
    L = len(levels)
    g = torch.Generator().manual_seed(seed)
    pm, wh = _cameras(dev, B, cams, yaw0=0.4)
    centre = torch.rand(B, A, 1, 3, generator=g) * torch.tensor([100.0, 100.0, 8.0]) - torch.tensor([50.0, 50.0, 5.0])
    kp = (centre + torch.randn(B, A, pts, 3, generator=g) * 0.35).to(dev)
    # anchors with a point within 1e-4 of the visibility gate (or of the depth epsilon) out of sight: float32 and float64 may
    # disagree on which cameras see it, and the masked softmax of the whole anchor with it
    uv, _ = ref.project(kp.double(), pm.double(), wh.double())
    z = torch.einsum("bcij,bapj->bapci", pm.double(), torch.cat([kp.double(), torch.ones_like(kp[..., :1]).double()], -1))[..., 2]
    near = ((uv.abs() < 1e-4) | ((uv - 1).abs() < 1e-4)).any(-1) | ((z - ref.DEPTH_EPS).abs() < 1e-4)
    kp[near.any(-1).any(-1)] = torch.tensor([0.0, 0.0, 80.0], device=dev)
    ss, st, num_feat = _pyramid(levels, dev)
    c = dict(kp=kp, pm=pm, wh=wh, ss=ss, st=st, num_feat=num_feat,
             feat=torch.randn(B, cams, num_feat, C, generator=g).to(dev),
             ra=torch.randn(B, A, L, pts, G, generator=g).to(dev), rc=(torch.randn(B, cams, L, pts, G, generator=g) * 0.7).to(dev),
             keep=(torch.rand(B, A, cams, L, pts, G, generator=g) > DROP).to(dev),
             gout_pts=torch.randn(B, A * pts, C, generator=g).to(dev), gout=torch.randn(B, A, C, generator=g).to(dev))
    with torch.no_grad():
        c["loc"], c["w"] = deformable_prepare(kp, pm, wh, (c["ra"][:, :, None] + c["rc"][:, None]).contiguous())
    return c


@pytest.fixture(scope="module")
def full():
    c = _block_case(1, 25600, seed=7)
    c["truth"], c["truth32"] = _truths(c["feat"], c["ss"], c["st"], c["loc"], c["w"], c["gout_pts"])
    # crowding: the rows under the busiest pixels are far larger than the typical touched row
    rowmax = c["truth"][1].abs().amax(-1)
    crowd = float(rowmax.max()) / float(rowmax[ref.touched_rows(c["ss"], c["st"], c["loc"], c["num_feat"])].median())
    print(f"\n[full] largest grad_mc_ms_feat row / median touched row = {crowd:.0f}")
    assert crowd > 10
    return c


@pytest.mark.parametrize("mode", ["region", "tiles", "scatter", "pinned"])
def test_full_size_daf_paths(full, mode):
    """DAF.apply with the region backward (default; gf_daf_raccumulate_kernel<32>), the tile backward (option
    daf.backward_tiles = 1; gf_daf_accumulate_kernel<32>), the scatter backward (pixel_major=False; gf_daf_bwd_kernel<4, true, true>),
    and the forward with pinned channel groups (gf_daf_fwd_grouped_kernel, G = 4)."""
    c = full
    got = _run_daf(c["feat"], c["ss"], c["st"], c["loc"], c["w"], c["gout_pts"], mode, pinned=mode == "pinned")
    _check_daf(f"full/{mode}", got, c["truth"], c["truth32"], c["loc"], c["ss"], c["st"], c["num_feat"], forward_only=mode == "pinned")


def _check_block(name, out, grads, truth, truth32, c):
    """The fused op's output and leaf gradients (kp, feat, ra, rc) row by row."""
    B, A, pts = c["kp"].shape[:3]
    cams = c["pm"].shape[1]
    uv, vis = ref.project(c["kp"].double(), c["pm"].double(), c["wh"].double())          # [B, A, pts, cams]
    print(f"\n[{name}]")
    assert_daf_rows_close(out, truth[0], truth32[0], f"{name}: output", 2, FWD_RTOL, touched=vis.any(-1).any(-1))
    if grads is None:
        return
    t, t32 = truth[1], truth32[1]
    loc = uv.reshape(B, A * pts, cams, 2)
    assert_daf_rows_close(grads["feat"], t["feat"], t32["feat"], f"{name}: grad_mc_ms_feat", 3, GRAD_RTOL,
                          touched=ref.touched_rows(c["ss"], c["st"], loc, c["num_feat"], slack=2e-3))
    # a key point's gradient comes through its sampling locations: exempt where one of its pairs is on a cell edge
    edge = _edge_pairs(loc, c["ss"], 1e-4).reshape(B, A, pts, cams).any(-1)
    e = assert_daf_rows_close(grads["kp"], t["kp"], t32["kp"], f"{name}: grad_key_points", 3, GRAD_RTOL,
                              touched=vis.any(-1), exempt=edge)
    assert e["exempt"] <= 1e-2 * e["touched"]
    perm = lambda x: x.permute(0, 1, 3, 2, 4)                                             # [B, A | cams, pts, L, G]
    assert_daf_rows_close(perm(grads["ra"]), perm(t["ra"]), perm(t32["ra"]), f"{name}: grad_raw_anchor", 3, GRAD_RTOL,
                          touched=vis.any(-1))
    assert_daf_rows_close(perm(grads["rc"]), perm(t["rc"]), perm(t32["rc"]), f"{name}: grad_raw_cam", 3, GRAD_RTOL)


@pytest.fixture(scope="module")
def full_block(full):
    c = full
    truths = {}
    for masked in (False, True):
        kw = dict(raw_anchor=c["ra"], raw_cam=c["rc"], weight_mask=c["keep"] if masked else None)
        args = (c["kp"], c["pm"], c["wh"], c["feat"], c["ss"], c["st"], c["gout"])
        truths[masked] = (ref.block_chunked(*args, **kw, dtype=torch.float64), ref.block_chunked(*args, **kw, dtype=torch.float32))
    return truths


@pytest.mark.parametrize("path", ["fused_forward", "fused", "fused_masked"])
def test_full_size_fused_paths(full, full_block, path):
    """deformable_fused_forward (inference: gf_daf_fused_kernel<8, false>) and deformable_fused (training:
    gf_daf_fused_kernel<8, MASK> + gf_daf_fused_bwd_kernel<8> + gf_daf_fused_cam_reduce_kernel) with and without the keep-mask,
    split logits (raw_anchor + raw_cam)."""
    from gaussianformer_amd.deformable_prepare import deformable_fused, deformable_fused_forward
    c = full
    masked = path == "fused_masked"
    mask = c["keep"] if masked else None
    truth, truth32 = full_block[masked]
    if path == "fused_forward":
        with torch.no_grad():
            out = deformable_fused_forward(c["kp"], c["pm"], c["wh"], c["feat"], c["ss"], c["st"], raw_anchor=c["ra"], raw_cam=c["rc"])
        _check_block(f"full/{path}", out, None, truth, truth32, c)
        return
    kp, feat, ra, rc = (c[k].clone().requires_grad_(True) for k in ("kp", "feat", "ra", "rc"))
    out = deformable_fused(kp, c["pm"], c["wh"], feat, c["ss"], c["st"], raw_anchor=ra, raw_cam=rc, weight_mask=mask)
    out.backward(c["gout"])
    _check_block(f"full/{path}", out.detach(), dict(kp=kp.grad, feat=feat.grad, ra=ra.grad, rc=rc.grad), truth, truth32, c)


@pytest.mark.parametrize("mode", ["region", "tiles"])
def test_two_batch_elements_crowded(mode):
    """B = 2 at a quarter of the full size: the pixel-major backward's per-b loop (workspace reused, grad_feat offset per b)."""
    c = _block_case(2, 6400, seed=17)
    truth, truth32 = _truths(c["feat"], c["ss"], c["st"], c["loc"], c["w"], c["gout_pts"])
    got = _run_daf(c["feat"], c["ss"], c["st"], c["loc"], c["w"], c["gout_pts"], mode)
    _check_daf(f"B2/{mode}", got, truth, truth32, c["loc"], c["ss"], c["st"], c["num_feat"])
    # both elements carry gradient
    assert all(float(got[1][b].abs().max()) > 0 for b in range(2))


# ---------------------------------------------------------------------------------------------------------------------------
# (b) every dispatch arm.  Forward: daf_forward_impl (csrc/daf.hip); backward: DAF.apply -> gf_daf_backward_sorted where
# gf_daf_backward_workspace_bytes > 0 (C / 4 lanes in {16, 32, 64}, (C / G) % 4 == 0), region accumulation where region_ok
# (C / 4 in {16, 32}, L * G <= 16, G <= 4, L <= 4) and daf.backward_tiles is 0, tile accumulation otherwise; the scatter
# gf_daf_backward for the other shapes (reduce = C / vec and C / G / vec powers of two <= 64).  Confirmed once with
# rocprofv3 --kernel-trace --stats, one run per case (the kernel names in ARMS' comments and in test_full_size_daf_paths'
# docstring are the ones it listed; every pixel-major case also runs gf_daf_bwd_kernel<8, true, false> for the point-major
# gradients and the bucket / scan kernels of its formulation).
ARMS = {
    # pin_channel_groups, vec 4, G = 1, C / G = 32 -> gf_daf_fwd_grouped_kernel<8>; backward: C / 4 = 8 lanes, not eligible for
    # the pixel-major backward -> gf_daf_bwd_kernel<4, true, true> (scatter, reduced in-wave)
    "pinned_G1_C32": dict(cams=6, C=32, G=1, pinned=True),
    # pin_channel_groups, G = 2, C / G = 32 -> gf_daf_fwd_grouped_kernel<8>; backward: region_ok (C / 4 = 16, L * G = 6) ->
    # gf_daf_bwd_kernel<8, true, false> + gf_daf_raccumulate_kernel<16>
    "pinned_G2_C64": dict(cams=6, C=64, G=2, pinned=True),
    # num_cams > 8 -> gf_daf_fwd_kernel<4>; backward: region_ok (C / 4 = 32, L * G = 12) -> gf_daf_raccumulate_kernel<32>
    "cams10_C128_G4": dict(cams=10, C=128, G=4),
    # vec 4, cams <= 8, C % 8 == 0, (C / G) % 8 == 0 -> gf_daf_fwd4_kernel<8>; backward with daf.backward_tiles = 1 ->
    # gf_daf_accumulate_kernel<16>
    "C64_G4_tiles": dict(cams=6, C=64, G=4, tiles=True),
    # gf_daf_fwd4_kernel<8>; backward with daf.backward_tiles = 1 -> gf_daf_accumulate_kernel<32>
    "C128_G4_tiles": dict(cams=6, C=128, G=4, tiles=True),
    # gf_daf_fwd4_kernel<8>; backward: G = 8 > 4, not region_ok -> gf_daf_accumulate_kernel<32>
    "C128_G8": dict(cams=6, C=128, G=8),
    # gf_daf_fwd4_kernel<8>; backward: C / 4 = 64 lanes, not region_ok -> gf_daf_accumulate_kernel<64>
    "C256_G8": dict(cams=6, C=256, G=8),
    # vec 4 but (C / G) % 8 != 0 (C / G = 12) -> gf_daf_fwd4_kernel<4>; backward: C / 4 = 12 lanes, not eligible, not a power
    # of two -> gf_daf_bwd_kernel<4, false, true>
    "C48_G4": dict(cams=6, C=48, G=4),
    # C / G = 6: vec 2 -> gf_daf_fwd_kernel<2>; backward: C / 2 = 12 lanes -> gf_daf_bwd_kernel<2, false, true>
    "vec2_C24_G4": dict(cams=6, C=24, G=4),
    # C / G = 1: vec 1 -> gf_daf_fwd_kernel<1>; backward: 8 lanes per point, 1 per group -> gf_daf_bwd_kernel<1, true, true>
    "vec1_C8_G8": dict(cams=5, C=8, G=8),
}
ARM_LEVELS = [(48, 80), (24, 40), (12, 20)]
ARM_PTS = 60000


def _arm_inputs(cams, C, G, seed):
    """ARM_PTS points over ``cams`` cameras: a third crowded around eight centres per camera (a few pixels wide), a third uniform
    over (-0.1, 1.1)^2 (some outside), a third on edges -- exactly on the gate (0 or 1: skipped), 1e-6 inside the border, and
    inside (0, 0.5 / h) where the taps above or left of the sample are off the map."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    N, L = ARM_PTS, len(ARM_LEVELS)
    third = N // 3
    centres = torch.rand(cams, 8, 2, generator=g) * 0.8 + 0.1
    pick = torch.randint(0, 8, (third, cams), generator=g)
    crowded = centres[torch.arange(cams)[None, :], pick] + torch.randn(third, cams, 2, generator=g) * 0.004
    uniform = torch.rand(third, cams, 2, generator=g) * 1.2 - 0.1
    n_e = N - 2 * third
    edge = torch.rand(n_e, cams, 2, generator=g) * 0.98 + 0.01
    choices = torch.tensor([0.0, 1.0, 1e-6, 1.0 - 1e-6, 0.3 / ARM_LEVELS[0][0], 0.45 / ARM_LEVELS[0][1], 0.2 / ARM_LEVELS[-1][0]])
    which = torch.randint(0, len(choices), (n_e, cams), generator=g)
    coord = torch.randint(0, 2, (n_e, cams), generator=g)
    edge[torch.arange(n_e)[:, None], torch.arange(cams)[None, :], coord] = choices[which]
    loc = torch.cat([crowded, uniform, edge])[None]
    loc = loc[:, torch.randperm(N, generator=g)].contiguous()                    # edge points next to crowded ones in every wave
    w = torch.rand(1, N, cams, L, G, generator=g)
    w[torch.rand(1, N, cams, L, G, generator=g) < 0.1] = 0.0
    ss, st, num_feat = _pyramid(ARM_LEVELS, dev)
    feat = torch.randn(1, cams, num_feat, C, generator=g)
    gout = torch.randn(1, N, C, generator=g)
    return feat.to(dev), ss, st, num_feat, loc.to(dev), w.to(dev), gout.to(dev)


@pytest.mark.parametrize("arm", list(ARMS), ids=list(ARMS))
def test_dispatch_arm(arm):
    cfg = ARMS[arm]
    feat, ss, st, num_feat, loc, w, gout = _arm_inputs(cfg["cams"], cfg["C"], cfg["G"], seed=100 + list(ARMS).index(arm))
    vis = _visible_pairs(loc)
    assert 0.3 < float(vis.float().mean()) < 0.95
    truth, truth32 = _truths(feat, ss, st, loc, w, gout)
    if cfg.get("pinned"):
        got = _run_daf(feat, ss, st, loc, w, gout, pinned=True)
        _check_daf(f"{arm}/pinned", got, truth, truth32, loc, ss, st, num_feat, forward_only=True)
        unpinned = _run_daf(feat, ss, st, loc, w, gout)
        assert torch.equal(got[0], unpinned[0])                                   # pinned groups: the same bits
    got = _run_daf(feat, ss, st, loc, w, gout, "tiles" if cfg.get("tiles") else "region")
    _check_daf(arm, got, truth, truth32, loc, ss, st, num_feat)


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the reference's own fixture: the chain the encoder runs, on the inputs the reference's fallback was executed on.

def _softmax_vjp(d, grad_w):
    """grad_weights [bs, A, cams, L, K, G] -> grad_raw through the masked softmax over (cams, L, K) per group, in float64; the
    weights are recomputed in float64 from the fixture's raw logits and visibility."""
    raw = torch.tensor(d["raw"], dtype=torch.float64)
    vis = torch.tensor(d["visible"]).permute(0, 2, 1, 3)[:, :, :, None, :, None].expand(raw.shape)   # [bs, A, cams, 1, K, 1]
    bs, A, cams, L, K, G = raw.shape
    flat = raw.masked_fill(~vis, float("-inf")).permute(0, 1, 5, 2, 3, 4).reshape(bs, A, G, -1)
    none = torch.isinf(flat).all(-1, keepdim=True)
    w = torch.where(none, torch.zeros_like(flat), flat.masked_fill(none, 0.0).softmax(-1))
    gw = torch.as_tensor(grad_w, dtype=torch.float64).permute(0, 1, 5, 2, 3, 4).reshape(bs, A, G, -1)
    gr = w * (gw - (w * gw).sum(-1, keepdim=True))
    return gr.reshape(bs, A, G, cams, L, K).permute(0, 1, 3, 4, 5, 2)


def _bound(name, got, d, key, f64=None, f32=None):
    want = d[f"{key}_f64"] if f64 is None else f64
    want32 = d[f"{key}_f32"] if f32 is None else f32
    got = np.asarray(got, dtype=np.float64)
    err, err32 = np.abs(got - want).max(), np.abs(np.asarray(want32, np.float64) - want).max()
    bound = 4 * err32 + 1e-6 * np.abs(want).max()
    print(f"  {name:40s} max err {err:.2e} <= {bound:.2e} (f32 run - f64: {err32:.2e}, max {np.abs(want).max():.2e})")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= bound, (name, err, bound)
    assert np.abs(want).max() > 0


def _pad_groups(x, G, to):
    """[..., C] -> [..., G * to]: each group's C / G channels followed by zeros.  The fused ops need (C / G) % 8 == 0 and the
    fixture has C / G = 4; zero channels leave the weights, the other channels and every other gradient as they are."""
    cg = x.shape[-1] // G
    return torch.nn.functional.pad(x.reshape(*x.shape[:-1], G, cg), (0, to - cg)).reshape(*x.shape[:-1], G * to)


def _unpad_groups(x, G, cg):
    return x.reshape(*x.shape[:-1], G, -1)[..., :cg].reshape(*x.shape[:-1], G * cg)


def test_reference_fixture():
    """feature_maps_format -> deformable_prepare(kp, pm, wh, raw) -> DAF.apply, against the arrays the reference's own fallback
    produced (output, feature-map, key-point and -- through the masked softmax -- raw-logit gradients); and the fused ops'
    output against the fixture's output summed over the key points.  The fixture's gradients are of sum(output * grad_output) with
    a gradient per key point, which the fused ops -- whose output is already summed over the key points -- cannot take: their
    gradients are held to the restatement on the fixture's inputs, under the same kind of bound (its float32 run's error)."""
    from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF
    from gaussianformer_amd.deformable_prepare import deformable_fused, deformable_fused_forward, deformable_prepare
    dev = torch.device("cuda:0")
    d = np.load(GOLDEN)
    levels = [tuple(int(v) for v in row) for row in d["levels"]]
    t = lambda k, grad=False: torch.tensor(d[k], device=dev).requires_grad_(grad)
    bs, A, K, C = d["output_f64"].shape
    G = d["raw"].shape[-1]
    kp, pm, wh, raw = t("key_points", True), t("projection_mat"), t("image_wh"), t("raw", True)
    maps = [t(f"feature_map{i}", True) for i in range(len(levels))]
    table, ss, st = DAF.feature_maps_format(maps)
    loc, w = deformable_prepare(kp, pm, wh, raw)
    out = DAF.apply(table, ss, st, loc, w).reshape(bs, A, K, C)
    out.backward(t("grad_output"))
    print("\n[reference fixture: feature_maps_format -> deformable_prepare -> DAF.apply]")
    _bound("output", out.detach().cpu(), d, "output")
    for i in range(len(levels)):
        _bound(f"grad_feature_map{i}", maps[i].grad.cpu(), d, f"grad_feature_map{i}")
    _bound("grad_key_points", kp.grad.cpu(), d, "grad_key_points")
    _bound("grad_raw (softmax VJP of grad_weights)", raw.grad.cpu(), d, "grad_raw",
           f64=_softmax_vjp(d, d["grad_weights_f64"]).numpy(), f32=_softmax_vjp(d, d["grad_weights_f32"]).numpy())

    print("[reference fixture: fused ops, channels padded to 8 per group]")
    table = table.detach()
    wide = _pad_groups(table, G, 8).contiguous()
    want, want32 = d["output_f64"].sum(axis=2), d["output_f32"].astype(np.float64).sum(axis=2)
    with torch.no_grad():
        fwd = deformable_fused_forward(kp.detach(), pm, wh, wide, ss, st, raw_weights=raw.detach())
    _bound("deformable_fused_forward (sum over K)", _unpad_groups(fwd, G, C // G).cpu(), d, "-", f64=want, f32=want32)
    kp2, wide, raw2 = kp.detach().clone().requires_grad_(True), wide.requires_grad_(True), raw.detach().clone().requires_grad_(True)
    gout = t("grad_output").sum(dim=2)
    fused = deformable_fused(kp2, pm, wh, wide, ss, st, raw_weights=raw2)
    fused.backward(_pad_groups(gout, G, 8))
    _bound("deformable_fused (sum over K)", _unpad_groups(fused.detach(), G, C // G).cpu(), d, "-", f64=want, f32=want32)
    args = (kp.detach(), pm, wh, table, ss, st, gout)
    (o64, g64), (o32, g32) = (ref.block_chunked(*args, raw=raw.detach(), dtype=dt) for dt in (torch.float64, torch.float32))
    assert np.abs(o64.cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()          # the restatement is the fixture's op
    for name, got, key in (("grad_mc_ms_feat", _unpad_groups(wide.grad, G, C // G), "feat"), ("grad_key_points", kp2.grad, "kp"),
                           ("grad_raw", raw2.grad, "raw")):
        _bound(f"deformable_fused {name}", got.cpu(), d, "-", f64=g64[key].cpu().numpy(), f32=g32[key].cpu().numpy())
