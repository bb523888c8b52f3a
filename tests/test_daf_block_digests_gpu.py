"""The deformable block's kernels, output bit for output bit: the fused forward and backward (``gf_daf_fused_kernel``,
``gf_daf_fused_bwd_kernel``) and the prepare forward and backward (``gf_daf_prepare_kernel``, ``gf_daf_prepare_bwd_kernel``)
against SHA-256 digests of their outputs recorded in tests/golden/daf_block_digests.json (tools/make_golden_daf_block_digests.py).
The other tests hold these kernels to the fp64 definition within a bound; only this one notices a change of the arithmetic that
stays inside it -- another product contracted into an FMA, another order of a sum --, which moving the shared pieces
(csrc/gf_daf.hpp) between the kernels must not bring.

Recorded: the fused forward's output; the fused backward's ``grad_key_points``, ``grad_raw_weights`` and ``grad_raw_anchor``; the
prepare's ``points_2d`` and ``weights``; the prepare backward's ``grad_raw_weights`` and ``grad_key_points``.  NOT recorded, because
float atomics sum them in no fixed order: ``grad_mc_ms_feat`` (global float atomics) and the fused backward's ``grad_raw_cam`` (a
per-workgroup LDS ``atomicAdd``); tests/test_daf_truth_gpu.py and tests/test_daf_fused_train_gpu.py hold those two.

The inputs come from integer draws alone (numpy's generator and exact rational camera rotations: no torch generator, no libm
function), so the file does not depend on a library's random stream.  Every case asserts from its inputs that it reaches the
path it is there for: see FUSED and PREPARE below."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "daf_block_digests.json")

# fused cases: B, A, pts, cams, levels (h, w), G, C, image_wh given
FUSED = {
    # A % 4 = 1 with two batch elements: one workgroup straddles them (camera table from memory); 78 pairs = two passes of the
    # pair loop; L G = 16 divides 64 (stepped entry walk); backward: 16 anchors per workgroup, the last chunk holds 5
    "straddle": dict(B=2, A=101, pts=13, cams=6, levels=[(20, 30), (10, 15)], G=8, C=128, wh=True),
    # L G = 6 does not divide 64 (division walk); C / 8 = 8 lanes per row = eight lane groups, each takes every eighth pair
    "division": dict(B=1, A=50, pts=5, cams=4, levels=[(12, 9), (6, 5), (3, 3)], G=2, C=64, wh=False),
    # one level, one group, four lanes per row
    "narrow": dict(B=1, A=37, pts=7, cams=3, levels=[(9, 9)], G=1, C=32, wh=True),
}
# prepare cases: B, A, pts, cams, L, G, image_wh given, keep-mask given
PREPARE = {
    "g4": dict(B=2, A=37, pts=7, cams=6, L=4, G=4, wh=True, mask=False),      # staged, the float4 form
    "g8_mask": dict(B=2, A=37, pts=7, cams=6, L=4, G=8, wh=False, mask=True),  # staged, scalar form, mask, no image_wh
    "g1": dict(B=2, A=37, pts=7, cams=6, L=4, G=1, wh=True, mask=True),
    "unstaged": dict(B=2, A=37, pts=13, cams=6, L=4, G=16, wh=True, mask=True),   # E = 4992: five copies exceed 60 KB
    "odd": dict(B=2, A=37, pts=5, cams=3, L=3, G=1, wh=False, mask=False),        # E = 45, odd: unstaged backward
}
NO_VISIBLE, ALL_DROPPED, DROPPED_GROUP = 0, 1, 0   # anchors with the planted conditions; anchors 2 .. hold the edge points

# camera c looks along (cos, sin, 0) of an exact rational rotation about the vertical axis, from a point near the origin
_DIRS = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (0.6, 0.8), (-0.8, 0.6)]
_IMG_W, _IMG_H = 64.0, 32.0
_KX, _KY = 0.25, 0.5   # u = 1/2 + _KX xc / zc, v = 1/2 + _KY yc / zc in camera coordinates: 127 degrees wide, cameras overlap


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _ints(rng, shape, bits, scale):
    """integers of `bits` bits times a power of two: exactly representable float32"""
    return (rng.integers(-2 ** bits, 2 ** bits, shape) * scale).astype(np.float32)


def _cameras(B, cams, wh):
    """projection matrices [B, cams, 4, 4] (K [R | -R p]) and image_wh [B, cams, 2]; without image_wh the division by the image
    size is folded into the rows (powers of two: exact)"""
    M = np.zeros((B, cams, 4, 4))
    for b in range(B):
        for c in range(cams):
            cs, sn = _DIRS[c]
            d, r, down = np.array([cs, sn, 0.0]), np.array([sn, -cs, 0.0]), np.array([0.0, 0.0, -1.0])
            p = np.array([0.25 * (c % 3) - 0.25, 0.125 * c - 0.25, 0.5 + 0.25 * b])     # the camera's position
            R = np.stack([_IMG_W * (_KX * r + 0.5 * d), _IMG_H * (_KY * down + 0.5 * d), d])
            if not wh:
                R = R / np.array([[_IMG_W], [_IMG_H], [1.0]])
            M[b, c, :3, :3] = R
            M[b, c, :3, 3] = -R @ p
            M[b, c, 3, 3] = 1.0
    image_wh = np.tile(np.array([_IMG_W, _IMG_H]), (B, cams, 1)) if wh else None
    return M.astype(np.float32), None if image_wh is None else image_wh.astype(np.float32)


def _uv(kp, M, image_wh):
    """(u, v, visible) of every (key point, camera) pair in float64: what the kernels compute in float32"""
    B, A, pts = kp.shape[:3]
    X = np.concatenate([kp.astype(np.float64), np.ones((B, A, pts, 1))], -1)
    p = np.einsum("bcij,bapj->bapci", M.astype(np.float64), X)
    zc = np.maximum(p[..., 2], 1e-5)
    u, v = p[..., 0] / zc, p[..., 1] / zc
    if image_wh is not None:
        u, v = u / image_wh[:, None, None, :, 0], v / image_wh[:, None, None, :, 1]
    return u, v, (p[..., 2] > 1e-5) & (u > 0) & (u < 1) & (v > 0) & (v < 1), p[..., 2]


def _key_points(rng, B, A, pts, M, levels):
    """anchors scattered around the cameras; anchor NO_VISIBLE far above every camera's image; anchors 2 .. hold, one key point
    each, points that camera 0 of batch element 0 sees in the first and the last half pixel of every level on all four sides"""
    centre = rng.integers(-96, 97, (B, A, 1, 3)) * np.array([1 / 8, 1 / 8, 1 / 64])
    kp = centre + rng.integers(-16, 17, (B, A, pts, 3)) / 16.0
    kp[:, NO_VISIBLE] = rng.integers(-8, 9, (B, pts, 3)) / 16.0 + np.array([0.0, 0.0, 100.0])
    d, r, down = np.array([1.0, 0.0, 0.0]), np.array([0.0, -1.0, 0.0]), np.array([0.0, 0.0, -1.0])
    p0 = np.array([-0.25, -0.25, 0.5])
    plants = []
    for h, w in levels:
        plants += [(0.25 / w, 0.4), (1 - 0.25 / w, 0.6), (0.3, 0.25 / h), (0.7, 1 - 0.25 / h)]
    for i, (u, v) in enumerate(plants):
        zc = 4.0
        kp[0, 2 + i // pts, i % pts] = p0 + zc * d + (u - 0.5) / _KX * zc * r + (v - 0.5) / _KY * zc * down
    assert 2 + (len(plants) - 1) // pts < A
    return kp.astype(np.float32)


def _off_the_gate(kp, M, image_wh):
    """key points with a pair within 1e-4 of the visibility gate (in front of the camera: a depth of exactly 0 is behind the gate in
    float32 too) are moved, by (3, 5, 7) / 128 per turn, until none is: float32 and the float64 of the facts below then decide every pair alike"""
    for _ in range(8):
        u, v, _, z = _uv(kp, M, image_wh)
        near = (((np.abs(np.minimum.reduce([u, 1 - u, v, 1 - v])) < 1e-4) & (z > 1e-4)) | ((z > 2e-6) & (z <= 1e-4))).any(-1)
        if not near.any():
            return kp
        kp[near] += np.array([3, 5, 7], dtype=np.float32) / 128
    raise AssertionError("a pair sits on the visibility gate")


def _edge_facts(u, v, vis, levels):
    """every level has visible pairs whose cell hangs over each of the four image sides: ok1 .. ok4 each false somewhere and both
    clamps of both axes active (margins of a fifth of a pixel, so float32 decides alike)"""
    for h, w in levels:
        him, wim = v * h - 0.5, u * w - 0.5
        for name, hit in (("top", him < -0.2), ("bottom", him > h - 1 + 0.2), ("left", wim < -0.2), ("right", wim > w - 1 + 0.2)):
            assert (hit & vis).any(), (h, w, name)


def fused_inputs(name):
    c = FUSED[name]
    B, A, pts, cams, levels, G, C = c["B"], c["A"], c["pts"], c["cams"], c["levels"], c["G"], c["C"]
    L = len(levels)
    rng = np.random.default_rng(sorted(FUSED).index(name) + 31)
    M, wh = _cameras(B, cams, c["wh"])
    kp = _off_the_gate(_key_points(rng, B, A, pts, M, levels), M, wh)
    num_feat = sum(h * w for h, w in levels)
    d = dict(kp=kp, M=M, wh=wh,
             feat=_ints(rng, (B, cams, num_feat, C), 12, 2.0 ** -11),
             raw=_ints(rng, (B, A, cams, L, pts, G), 20, 2.0 ** -19),
             raw_anchor=_ints(rng, (B, A, L, pts, G), 20, 2.0 ** -19),
             raw_cam=_ints(rng, (B, cams, L, pts, G), 20, 2.0 ** -20),
             grad_out=_ints(rng, (B, A, C), 12, 2.0 ** -11),
             mask=rng.integers(0, 100, (B, A, cams, L, pts, G)) >= 15,
             spatial_shape=np.array(levels, dtype=np.int32),
             scale_start=np.cumsum([0] + [h * w for h, w in levels[:-1]]).astype(np.int32))
    d["mask"][0, ALL_DROPPED, :, :, :, DROPPED_GROUP] = False
    # ---- what the case is there for, from its inputs
    u, v, vis, _ = _uv(kp, M, wh)
    assert not vis[:, NO_VISIBLE].any()                       # nvis = 0
    assert vis[0, ALL_DROPPED].any()                          # a visible pair, and the mask drops its whole group: s = 0, inv = 0
    assert not d["mask"][0, ALL_DROPPED, :, :, :, DROPPED_GROUP].any()
    _edge_facts(u[0], v[0], vis[0], levels)
    nvis = vis.reshape(B, A, -1).sum(-1)
    d["facts"] = dict(npair=pts * cams, LG=L * G, lanes_per_row=C // 8, nvis_max=int(nvis.max()))
    return c, d


def _fused_facts(name, c, f):
    if name == "straddle":
        assert c["B"] > 1 and c["A"] % 4 == 1               # workgroup A // 4 holds anchors of both batch elements
        assert 64 < f["npair"] <= 128                          # two passes of the pair loop
        assert 64 % f["LG"] == 0                               # stepped entry walk
        assert c["A"] % 16 == 5                                # 4 waves x 4 anchors per workgroup: a ragged last chunk
        assert f["nvis_max"] > 4                               # four lane groups, a second pair each
        J = c["cams"] * len(c["levels"]) * c["pts"] * c["G"]
        per_wave = 9 * f["npair"] + J // c["cams"] + f["npair"] * f["LG"]
        assert 4 * (2 * J + 4 * per_wave + 2) <= 160 * 1024    # ... four waves do fit
    elif name == "division":
        assert 64 % f["LG"] != 0                               # division walk
        assert f["lanes_per_row"] == 8 and f["nvis_max"] > 8   # eight lane groups, one of them takes a second pair
    else:
        assert f["LG"] == 1 and f["lanes_per_row"] == 4


def compute_fused(name):
    """{output: digest} of one fused case on the GPU: split and unsplit logits, masked and unmasked"""
    from gaussianformer_amd.deformable_prepare import deformable_fused, deformable_fused_forward
    c, d = fused_inputs(name)
    _fused_facts(name, c, d["facts"])
    dev = torch.device("cuda:0")
    t = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    out = {}
    for split in (False, True):
        for masked in (False, True):
            tag = ("split" if split else "full") + (".masked" if masked else "")
            kp = t["kp"].clone().requires_grad_(True)
            feat = t["feat"].clone().requires_grad_(True)
            logits = [t[k].clone().requires_grad_(True) for k in (("raw_anchor", "raw_cam") if split else ("raw",))]
            kw = dict(raw_anchor=logits[0], raw_cam=logits[1]) if split else dict(raw_weights=logits[0])
            y = deformable_fused(kp, t["M"], t["wh"], feat, t["spatial_shape"], t["scale_start"],
                                 weight_mask=t["mask"] if masked else None, **kw)
            if not masked:   # the inference entry point runs the same kernel
                with torch.no_grad():
                    y0 = deformable_fused_forward(t["kp"], t["M"], t["wh"], t["feat"], t["spatial_shape"], t["scale_start"],
                                                  **{k: v.detach() for k, v in kw.items()})
                assert torch.equal(y0, y.detach())
            y.backward(t["grad_out"])
            assert not y[:, NO_VISIBLE].any()                       # no visible pair: a zero row
            out[f"{tag}.out"] = _sha(y)
            out[f"{tag}.grad_key_points"] = _sha(kp.grad)
            out[f"{tag}.grad_raw_anchor" if split else f"{tag}.grad_raw_weights"] = _sha(logits[0].grad)
            assert feat.grad is not None and (not split or logits[1].grad is not None)   # computed, summed by atomics: not recorded
    return out


def prepare_inputs(name):
    c = PREPARE[name]
    B, A, pts, cams, L, G = c["B"], c["A"], c["pts"], c["cams"], c["L"], c["G"]
    rng = np.random.default_rng(sorted(PREPARE).index(name) + 57)
    M, wh = _cameras(B, cams, c["wh"])
    kp = _off_the_gate(_key_points(rng, B, A, pts, M, []), M, wh)
    d = dict(kp=kp, M=M, wh=wh, raw=_ints(rng, (B, A, cams, L, pts, G), 20, 2.0 ** -19),
             mask=(rng.integers(0, 100, (B, A, cams, L, pts, G)) >= 15) if c["mask"] else None,
             grad_points=_ints(rng, (B, A * pts, cams, 2), 12, 2.0 ** -11),
             grad_weights=_ints(rng, (B, A * pts, cams, L, G), 12, 2.0 ** -11))
    u, v, vis, _ = _uv(kp, M, wh)
    assert not vis[:, NO_VISIBLE].any() and vis.any(-1).any(-1).sum() > B * A // 2     # an all-miss anchor among seen ones
    # ---- the route, from the launch conditions of gf_daf_prepare / gf_daf_prepare_backward (torch's allocations are aligned)
    E = pts * cams * L * G
    fwd_staged, bwd_staged = 5 * 4 * E <= 60 * 1024, E % 4 == 0 and 5 * 4 * E <= 48 * 1024
    assert (fwd_staged, bwd_staged) == {"unstaged": (False, False), "odd": (True, False)}.get(name, (True, True)), (E, fwd_staged, bwd_staged)
    assert A % 4 == 1 and B > 1                                   # a ragged last workgroup, anchors of both batch elements
    return c, d


def compute_prepare(name):
    """{output: digest} of one prepare case on the GPU"""
    from gaussianformer_amd.deformable_prepare import deformable_prepare
    c, d = prepare_inputs(name)
    dev = torch.device("cuda:0")
    t = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    kp, raw = t["kp"].clone().requires_grad_(True), t["raw"].clone().requires_grad_(True)
    p, w = deformable_prepare(kp, t["M"], t["wh"], raw, t["mask"])
    torch.autograd.backward([p, w], [t["grad_points"], t["grad_weights"]])
    assert not w.view(c["B"], c["A"], -1)[:, NO_VISIBLE].any()
    return {"points_2d": _sha(p), "weights": _sha(w), "grad_raw_weights": _sha(raw.grad), "grad_key_points": _sha(kp.grad)}


def _check(case, got):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(got) if got[k] != want[k]]
    assert not differ, (f"{case}: the bits of {differ} are not the recorded ones.  The deformable block's arithmetic changed.  Regenerate "
                        "tests/golden/daf_block_digests.json (tools/make_golden_daf_block_digests.py) ONLY if that change is intended.")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FUSED))
def test_fused_block_bits_are_the_recorded_ones(gpu, name):
    _check("fused." + name, compute_fused(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PREPARE))
def test_prepare_bits_are_the_recorded_ones(gpu, name):
    _check("prepare." + name, compute_prepare(name))
