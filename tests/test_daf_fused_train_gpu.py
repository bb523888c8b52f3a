"""The training form of the fused deformable aggregation (deformable_fused: gf_daf_fused_forward_masked + gf_daf_fused_backward)
against the three-step path it stands for (deformable_prepare -> DAF.apply -> sum over the key points, with torch autograd), each
step of which is held to the reference by its own tests, and against the float64 restatement of the reference's block
(tests/daf_fused_ref.py).  Forward and gradients, with and without the attention-dropout keep-mask."""
import os
import sys

import numpy as np
import pytest
import torch

import daf_fused_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = 0.15


def _cameras(dev, cams, wh=(1600.0, 864.0)):
    """A ring of pinhole cameras looking outwards: a point is seen by one or two of them."""
    pm = torch.eye(4).repeat(1, cams, 1, 1)
    K = torch.tensor([[1260.0, 0, wh[0] / 2], [0, 1260.0, wh[1] / 2], [0, 0, 1.0]])
    for c in range(cams):
        yaw = 2 * np.pi * c / cams
        R = torch.tensor([[-np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, -1.0], [np.cos(yaw), np.sin(yaw), 0.0]], dtype=torch.float32)
        pm[0, c, :3, :3] = K @ R
        pm[0, c, :3, 3] = K @ torch.tensor([0.0, 1.5, 0.0])
    return pm.to(dev), torch.tensor([[list(wh)] * cams], device=dev)


def _case(A, pts, cams, levels, G, C, B, with_wh, seed, spread=50.0):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    L = len(levels)
    pm, wh = _cameras(dev, cams)
    if B > 1:
        pm, wh = pm.repeat(B, 1, 1, 1).contiguous(), wh.repeat(B, 1, 1).contiguous()
        pm[1, :, :3, 3] += 0.5
    if not with_wh:
        pm = pm * torch.tensor([1.0 / 1600.0, 1.0 / 864.0, 1.0, 1.0], device=dev)[None, None, :, None]
        wh = None
    kp = torch.empty(B, A, pts, 3).uniform_(-spread, spread, generator=g)
    kp[..., 2] = torch.empty(B, A, pts).uniform_(-3.0, 5.0, generator=g)
    kp[:, :7] = torch.tensor([0.0, 0.0, 80.0])                 # anchors no camera sees
    ss = torch.tensor(levels, dtype=torch.int32)
    sizes = ss[:, 0] * ss[:, 1]
    st = torch.cat([torch.zeros(1, dtype=torch.int32), torch.cumsum(sizes, 0)[:-1].to(torch.int32)])
    feat = torch.randn(B, cams, int(sizes.sum()), C, generator=g)
    ra = torch.randn(B, A, L, pts, G, generator=g)
    rc = torch.randn(B, cams, L, pts, G, generator=g) * 0.7
    keep = torch.rand(B, A, cams, L, pts, G, generator=g) > DROP
    gout = torch.randn(B, A, C, generator=g)
    d = dict(kp=kp, pm=pm, wh=wh, feat=feat, ss=ss, st=st, ra=ra, rc=rc, keep=keep, gout=gout)
    return {k: (v.to(dev) if v is not None else None) for k, v in d.items()}


def _fused(c, split, mask, grads=True):
    from gaussianformer_amd.deformable_prepare import deformable_fused
    kp, feat, ra, rc = (c[k].clone().requires_grad_(grads) for k in ("kp", "feat", "ra", "rc"))
    if split:
        out = deformable_fused(kp, c["pm"], c["wh"], feat, c["ss"], c["st"], raw_anchor=ra, raw_cam=rc, weight_mask=mask)
        leaves = dict(kp=kp, feat=feat, ra=ra, rc=rc)
    else:
        raw = (ra[:, :, None] + rc[:, None]).detach().contiguous().requires_grad_(grads)
        out = deformable_fused(kp, c["pm"], c["wh"], feat, c["ss"], c["st"], raw_weights=raw, weight_mask=mask)
        leaves = dict(kp=kp, feat=feat, raw=raw)
    if grads:
        out.backward(c["gout"])
    return out.detach(), {k: v.grad for k, v in leaves.items()}


def _three(c, split, mask, grads=True):
    from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF
    from gaussianformer_amd.deformable_prepare import deformable_prepare
    kp, feat, ra, rc = (c[k].clone().requires_grad_(grads) for k in ("kp", "feat", "ra", "rc"))
    B, A, pts = kp.shape[:3]
    if split:
        raw = ra[:, :, None] + rc[:, None]
        leaves = dict(kp=kp, feat=feat, ra=ra, rc=rc)
    else:
        raw = (ra[:, :, None] + rc[:, None]).detach().contiguous().requires_grad_(grads)
        leaves = dict(kp=kp, feat=feat, raw=raw)
    loc, w = deformable_prepare(kp, c["pm"], c["wh"], raw.contiguous(), mask)
    out = DAF.apply(feat, c["ss"], c["st"], loc, w).reshape(B, A, pts, -1).sum(dim=2)
    if grads:
        out.backward(c["gout"])
    return out.detach(), {k: v.grad for k, v in leaves.items()}


def _rel(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-12)


CASES = [
    (3000, 9, 6, [(64, 176), (32, 88), (16, 44), (8, 22)], 4, 128, 1, True),     # the encoder's block
    (1001, 13, 6, [(20, 30), (10, 15)], 8, 128, 2, True),                         # two batch elements (workgroups straddle them), G = 8
    (500, 5, 4, [(12, 9), (6, 5), (3, 3)], 2, 64, 1, False),                      # no image_wh, C = 64
    (257, 7, 3, [(9, 9)], 1, 32, 1, True),                                         # one level, one group, C = 32
]
IDS = ["block", "B2_G8", "no_wh_C64", "L1_G1"]


@pytest.mark.parametrize("split", [True, False], ids=["split", "full"])
@pytest.mark.parametrize("case", CASES + [(3000, 9, 6, [(64, 176), (32, 88), (16, 44), (8, 22)], 4, 128, 1, True)],
                         ids=IDS + ["block_again"])
def test_unmasked_forward_is_bit_identical_to_fused_forward(case, split):
    from gaussianformer_amd.deformable_prepare import deformable_fused, deformable_fused_forward
    A, pts, cams, levels, G, C, B, with_wh = case
    c = _case(A, pts, cams, levels, G, C, B, with_wh, seed=A + pts)
    kw = dict(raw_anchor=c["ra"], raw_cam=c["rc"]) if split else dict(raw_weights=(c["ra"][:, :, None] + c["rc"][:, None]).contiguous())
    with torch.no_grad():
        want = deformable_fused_forward(c["kp"], c["pm"], c["wh"], c["feat"], c["ss"], c["st"], **kw)
    got = deformable_fused(c["kp"], c["pm"], c["wh"], c["feat"], c["ss"], c["st"], **kw)
    assert torch.equal(got, want)


@pytest.mark.parametrize("split", [True, False], ids=["split", "full"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_masked_forward_and_gradients_equal_three_steps(case, split):
    A, pts, cams, levels, G, C, B, with_wh = case
    c = _case(A, pts, cams, levels, G, C, B, with_wh, seed=A + pts + 1)
    for mask in (None, c["keep"]):
        got, gg = _fused(c, split, mask)
        want, gw = _three(c, split, mask)
        scale = want.abs().amax(dim=-1, keepdim=True).clamp(min=1e-3)
        assert float(((got - want).abs() / scale).max()) <= 1e-5
        assert float(got[:, :7].abs().max()) == 0.0
        assert (want.abs().amax(dim=-1) > 0).float().mean() > 0.5
        assert _rel(gg["feat"], gw["feat"]) <= 2e-5
        assert _rel(gg["kp"], gw["kp"]) <= 2e-4
        for k in (("ra", "rc") if split else ("raw",)):
            assert _rel(gg[k], gw[k]) <= 2e-5, k
        if not split:
            # invisible, dropped and all-miss entries: exactly zero
            from gaussianformer_amd.deformable_prepare import deformable_prepare
            raw = (c["ra"][:, :, None] + c["rc"][:, None]).contiguous()
            loc, _ = deformable_prepare(c["kp"], c["pm"], c["wh"], raw)
            vis = ((loc > 0) & (loc < 1)).all(-1).reshape(B, A, pts, cams).permute(0, 1, 3, 2)[:, :, :, None, :, None]
            dead = ~vis.expand(raw.shape)
            if mask is not None:
                dead = dead | ~mask
            assert float(gg["raw"][dead].abs().max()) == 0.0
            assert float(gg["raw"][:, :7].abs().max()) == 0.0


def test_dropped_group_gives_zero_channels():
    from gaussianformer_amd.deformable_prepare import deformable_fused
    c = _case(3000, 9, 6, [(64, 176), (32, 88), (16, 44), (8, 22)], 4, 128, 1, True, seed=5)
    keep = c["keep"].clone()
    with torch.no_grad():
        base = deformable_fused(c["kp"], c["pm"], c["wh"], c["feat"], c["ss"], c["st"], raw_anchor=c["ra"], raw_cam=c["rc"])
    a = int(torch.nonzero(base[0].abs().amax(-1) > 0)[0, 0])
    keep[0, a, ..., 1] = False                                   # every entry of group 1 of anchor a dropped
    got, _ = _fused(c, True, keep, grads=False)
    want, _ = _three(c, True, keep, grads=False)
    gc = 128 // 4
    assert float(got[0, a, gc:2 * gc].abs().max()) == 0.0
    for g in (0, 2, 3):
        assert float(got[0, a, g * gc:(g + 1) * gc].abs().max()) > 0.0
    scale = want.abs().amax(dim=-1, keepdim=True).clamp(min=1e-3)
    assert float(((got - want).abs() / scale).max()) <= 1e-5
    # the group's logits get no gradient either
    ra = c["ra"].clone().requires_grad_(True)
    out = deformable_fused(c["kp"], c["pm"], c["wh"], c["feat"], c["ss"], c["st"], raw_anchor=ra, raw_cam=c["rc"], weight_mask=keep)
    out.backward(c["gout"])
    assert float(ra.grad[0, a, ..., 1].abs().max()) == 0.0 and float(ra.grad[0, a].abs().max()) > 0.0


@pytest.mark.parametrize("masked", [False, True])
def test_against_float64_restatement(masked):
    """Small shapes against tests/daf_fused_ref.py (float64 autograd), through DAF.feature_maps_format's autograd to the pyramid
    levels.  Anchors with a point within 1e-4 of the visibility boundary are moved out of sight (float32 and float64 may disagree
    on their visibility)."""
    from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF
    from gaussianformer_amd.deformable_prepare import deformable_fused
    dev = torch.device("cuda:0")
    B, A, pts, cams, L, G, C = 2, 200, 5, 4, 3, 4, 64
    levels = [(24, 40), (12, 20), (6, 10)]
    c = _case(A, pts, cams, levels, G, C, B, True, seed=11, spread=20.0)
    uv, vis = ref.project(c["kp"].double(), c["pm"].double(), c["wh"].double())
    z = torch.einsum("bcij,bapj->bapci", c["pm"].double(), torch.cat([c["kp"].double(), torch.ones_like(c["kp"][..., :1]).double()], -1))[..., 2]
    near = ((uv.abs() < 1e-4) | ((uv - 1).abs() < 1e-4)).any(-1) | ((z - 1e-5).abs() < 1e-4)
    kp0 = c["kp"].clone()
    kp0[near.any(-1).any(-1)] = torch.tensor([0.0, 0.0, 80.0], device=dev)
    g = torch.Generator().manual_seed(3)
    maps32 = [torch.randn(B, cams, C, h, w, generator=g).to(dev) for h, w in levels]
    mask = c["keep"] if masked else None
    # fused, float32
    kp = kp0.clone().requires_grad_(True)
    maps = [m.clone().requires_grad_(True) for m in maps32]
    ra, rc = c["ra"].clone().requires_grad_(True), c["rc"].clone().requires_grad_(True)
    table, ss, st = DAF.feature_maps_format(maps)
    out = deformable_fused(kp, c["pm"], c["wh"], table, ss, st, raw_anchor=ra, raw_cam=rc, weight_mask=mask)
    out.backward(c["gout"])
    # restatement, float64
    kpd = kp0.double().requires_grad_(True)
    mapsd = [m.double().requires_grad_(True) for m in maps32]
    rad, rcd = c["ra"].double().requires_grad_(True), c["rc"].double().requires_grad_(True)
    want = ref.block(kpd, c["pm"].double(), c["wh"].double(), mapsd, rad[:, :, None] + rcd[:, None], mask)
    want.backward(c["gout"].double())
    want = want.detach()
    assert float(want.abs().max()) > 0.1
    assert _rel(out.double(), want) <= 1e-5
    for got, w, name in [(m.grad, md.grad, f"map{i}") for i, (m, md) in enumerate(zip(maps, mapsd))] + \
                        [(ra.grad, rad.grad, "raw_anchor"), (rc.grad, rcd.grad, "raw_cam"), (kp.grad, kpd.grad, "key_points")]:
        assert _rel(got.double(), w) <= (1e-3 if name == "key_points" else 1e-4), name


def test_full_block_shape_gradients_and_memory():
    """A = 25 600, pts 9, cams 6, L 4, G 4, C 128, the DAF_LEVELS pyramid, projected key points, split logits: the bounds above
    hold, and forward + backward allocate less than one [A * pts, cams, L, G] weights tensor beyond the grad_mc_ms_feat table."""
    from gaussianformer_amd.synthetic import DAF_LEVELS
    dev = torch.device("cuda:0")
    A, pts, cams, L, G, C = 25600, 9, 6, 4, 4, 128
    c = _case(A, pts, cams, [tuple(x) for x in DAF_LEVELS], G, C, 1, True, seed=7)
    g = torch.Generator().manual_seed(8)
    centre = torch.rand(1, A, 1, 3, generator=g) * torch.tensor([100.0, 100.0, 8.0]) - torch.tensor([50.0, 50.0, 5.0])
    c["kp"] = (centre + torch.randn(1, A, pts, 3, generator=g) * 0.35).to(dev)
    weights_bytes = A * pts * cams * L * G * 4
    for mask in (None, c["keep"]):
        from gaussianformer_amd.deformable_prepare import deformable_fused
        kp, feat, ra, rc = (c[k].clone().requires_grad_(True) for k in ("kp", "feat", "ra", "rc"))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = deformable_fused(kp, c["pm"], c["wh"], feat, c["ss"], c["st"], raw_anchor=ra, raw_cam=rc, weight_mask=mask)
        out.backward(c["gout"])
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base - feat.numel() * 4
        assert extra < weights_bytes, (extra, weights_bytes)
        got, gg = out.detach(), dict(kp=kp.grad, feat=feat.grad, ra=ra.grad, rc=rc.grad)
        del out, kp, feat, ra, rc
        want, gw = _three(c, True, mask)
        scale = want.abs().amax(dim=-1, keepdim=True).clamp(min=1e-3)
        assert float(((got - want).abs() / scale).max()) <= 1e-5
        assert (want.abs().amax(dim=-1) > 0).float().mean() > 0.5
        assert _rel(gg["feat"], gw["feat"]) <= 2e-5
        assert _rel(gg["kp"], gw["kp"]) <= 2e-4
        assert _rel(gg["ra"], gw["ra"]) <= 2e-5 and _rel(gg["rc"], gw["rc"]) <= 2e-5
        del gg, gw


@pytest.mark.parametrize("masked", [False, True])
def test_worst_case_every_pair_visible(masked):
    """pts * cams = 256 with every pair visible: the LDS of the gw values at its largest."""
    dev = torch.device("cuda:0")
    A, pts, cams, G, C = 300, 64, 4, 4, 128
    levels = [(32, 48), (16, 24), (8, 12), (4, 6)]
    c = _case(A, pts, cams, levels, G, C, 1, False, seed=21)
    g = torch.Generator().manual_seed(22)
    pm = torch.zeros(1, cams, 4, 4)
    for k in range(cams):                                       # u = x / z, v = y / z, slightly different per camera
        pm[0, k] = torch.tensor([[1.0, 0, 0.02 * k, 0], [0, 1.0, -0.01 * k, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])
    z = torch.rand(1, A, pts, generator=g) + 1.0
    kp = torch.stack([torch.rand(1, A, pts, generator=g) * 0.8 + 0.1, torch.rand(1, A, pts, generator=g) * 0.8 + 0.1, torch.ones(1, A, pts)], -1) * z[..., None]
    c["kp"], c["pm"] = kp.to(dev), pm.to(dev)
    mask = c["keep"] if masked else None
    got, gg = _fused(c, True, mask)
    want, gw = _three(c, True, mask)
    from gaussianformer_amd.deformable_prepare import deformable_prepare
    loc, _ = deformable_prepare(c["kp"], c["pm"], None, (c["ra"][:, :, None] + c["rc"][:, None]).contiguous())
    assert bool(((loc > 0) & (loc < 1)).all())
    scale = want.abs().amax(dim=-1, keepdim=True).clamp(min=1e-3)
    assert float(((got - want).abs() / scale).max()) <= 1e-5
    assert _rel(gg["feat"], gw["feat"]) <= 2e-5
    assert _rel(gg["kp"], gw["kp"]) <= 2e-4
    assert _rel(gg["ra"], gw["ra"]) <= 2e-5 and _rel(gg["rc"], gw["rc"]) <= 2e-5


def test_only_requested_gradients():
    from gaussianformer_amd.deformable_prepare import deformable_fused
    c = _case(500, 5, 4, [(12, 9), (6, 5)], 2, 64, 1, True, seed=4)
    ra = c["ra"].clone().requires_grad_(True)
    kp, feat, rc = c["kp"].clone(), c["feat"].clone(), c["rc"].clone()
    deformable_fused(kp, c["pm"], c["wh"], feat, c["ss"], c["st"], raw_anchor=ra, raw_cam=rc).backward(c["gout"])
    _, gw = _three(c, True, None)
    assert kp.grad is None and feat.grad is None and rc.grad is None
    assert _rel(ra.grad, gw["ra"]) <= 2e-5


def test_bench_step_fused_gives_every_leaf_a_gradient():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_step
    r = bench_step.run(anchors=3000, steps=1, warmup=1, daf="fused")
    assert r["leaves_without_finite_nonzero_grad"] == [] and r["daf"] == "fused"
