"""The chained training step of tools/bench_step.py (BASELINE config [2]) against its float64 restatement (tests/step_ref.py),
LEAF BY LEAF and ROW BY ROW.

At the benchmark's shape (25 600 anchors, 200 x 200 x 16 grid, six cameras, the DAF_LEVELS pyramid) the native step runs once,
forward and backward; the restatement runs in float64 (the truth) and in float32 (the yardstick of plain float32 arithmetic).
Every quantity is bounded row by row with the rule of ``util.assert_daf_rows_close``: err <= max(rtol x max(|ref row|, median
floor), 4 x the float32 restatement's error on that row), rtol 1e-4 for forward outputs and 1e-3 (GRAD_RTOL) for gradients.
Rows no stage can reach are exactly 0 (pyramid pixels no tap touches, voxels no box covers), or -- prob head -- exactly the
uniform row.

Float32 rounding may flip a few discrete outcomes; each is handled explicitly and counted, no tolerance is loosened:
- the visibility window and the depth cut: anchors with a key point whose float32 and float64 projections disagree on a camera,
  or that lie within GATE_MARGIN of the window or the cut, are redrawn before the run (none may remain);
- pixel-centre crossings: the restatement samples each tap on the cell the product's float32 projection (gf_daf_prepare) chose, and
  an anchor with a visible tap within EDGE_SLACK pixels of a cell edge is exempt on columns 0:6 of its anchor gradient (means,
  scales: their location derivative jumps there, and the fused kernels project on their own) -- only those columns;
- the prob cut (probability sum > 1e-9): voxels within 1e-4 relative of it are exempt from the logits bound, and the Gaussians
  whose boxes cover such a voxel from their anchors' gradient bounds."""
import os
import sys

import pytest
import torch

import daf_fused_ref as dref
import step_ref
from util import GRAD_RTOL, assert_daf_rows_close

pytestmark = pytest.mark.gpu
FWD_RTOL = 1e-4
GATE_MARGIN = 1e-6
EDGE_SLACK = 1e-4
EDGE_CAP = 3000           # exempt anchors (columns 0:6) at the benchmark's shape: 1470 measured, 2x margin
CUT_SLACK = 1e-4
CASES = [("three_step", "plain"), ("fused", "plain"), ("three_step", "empty"), ("fused", "prob")]


def _bench_step():
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import bench_step
    return bench_step


def _key_points(named, const, dtype):
    """Per block: key points [1, A, pts, 3] of the restatement's definition, in ``dtype``."""
    anchor = named["anchor"].detach().to(dtype)
    means, scales, _, _ = step_ref._front(anchor, const)
    return [step_ref._kp(means, scales, b["key_offsets"].detach().to(dtype)) for b in named["blocks"]]


def _gate_flags(named, const):
    """[A] bool: anchors with a key point whose visibility on some camera float32 and float64 judge differently, or that lies
    within GATE_MARGIN of the strict (0, 1) window or of the depth cut."""
    flags = 0
    for k32, k64 in zip(_key_points(named, const, torch.float32), _key_points(named, const, torch.float64)):
        uv64, vis64 = dref.project(k64, const["pm"].double(), const["wh"].double())
        _, vis32 = dref.project(k32, const["pm"], const["wh"])
        hom = torch.cat([k64, torch.ones_like(k64[..., :1])], -1)
        z = torch.einsum("bcij,bapj->bapc", const["pm"].double()[:, :, 2:3], hom)
        near = ((uv64.abs() < GATE_MARGIN) | ((uv64 - 1).abs() < GATE_MARGIN)).any(-1) | ((z - dref.DEPTH_EPS).abs() < GATE_MARGIN)
        flags = flags | (near | (vis64 != vis32)).any(-1).any(-1)[0]
    return flags.bool()


def _redraw_gates(s):
    """Rewrites (no_grad, deterministic generator) the anchors :func:`_gate_flags` marks until none is left; returns how many
    rows were redrawn."""
    anchor = s.named["anchor"]
    g = torch.Generator(device="cpu").manual_seed(1234)
    redrawn = 0
    for _ in range(20):
        bad = _gate_flags(s.named, s.const)
        n = int(bad.sum())
        if n == 0:
            break
        redrawn += n
        with torch.no_grad():
            anchor[0, bad] = torch.randn(n, anchor.shape[-1], generator=g).to(anchor.device)
    return redrawn


def _path_word(s, outs):
    from gaussianformer_amd import _lib
    if s.const["head"] == "prob":
        state = s.prob_state
    else:
        state = s.agg.last_state
    return _lib.SplatState.of(state).path


def _edge_anchors(kps, const, ss):
    """[A] bool: anchors with a visible tap within EDGE_SLACK pixels of a cell edge at some level, in some block."""
    flags = 0
    for kp in kps:
        uv, _ = dref.project(kp, const["pm"].double(), const["wh"].double())
        B, A, P, cams = uv.shape[:4]
        e = dref.edge_pairs(uv.reshape(B, A * P, cams, 2), ss, EDGE_SLACK).reshape(B, A, P, cams)
        flags = flags | e.any(-1).any(-1)[0]
    return flags.bool()


def _touched_pixels(kps, const, ss, st, num_feat):
    hit = 0
    for kp in kps:
        uv, _ = dref.project(kp, const["pm"].double(), const["wh"].double())
        B, A, P, cams = uv.shape[:4]
        hit = hit | dref.touched_rows(ss, st, uv.reshape(B, A * P, cams, 2), num_feat, slack=2e-3)
    return hit.bool()


@pytest.mark.parametrize("daf,head", CASES, ids=[f"{d}-{h}" for d, h in CASES])
def test_step_against_float64(gpu, daf, head):
    from gaussianformer_amd import _lib
    from gaussianformer_amd.deformable_prepare import deformable_prepare
    from gaussianformer_amd.gaussian_prepare import gaussian_prepare
    bs = _bench_step()
    s = bs.build(25600, daf, head)
    const, named = s.const, s.named
    redrawn = _redraw_gates(s)
    assert int(_gate_flags(named, const).sum()) == 0

    # the integer decisions the restatement takes as inputs are the product's
    dec = step_ref.decisions(named, const)
    assert torch.equal(s.blocks[0].spconv.voxel_indices(named["anchor"].detach()), dec["voxels"])
    with torch.no_grad():
        means, scales, rots, _ = step_ref._front(named["anchor"].detach(), const)
        mode = _lib.GF_RADII_SCALAR_CLAMPED if head == "prob" else _lib.GF_RADII_SCALAR
        mi, radii, _ = gaussian_prepare(means[0], scales[0], rots[0], const["pc_range"][:3], const["cell"], const["scale_multiplier"],
                                        *const["grid"], mode, 1)
    A = means.shape[1]
    assert torch.equal(mi, dec["means_int"][:A]) and torch.equal(radii, dec["radii"][:A])
    # the taps' cells as the product's projection (gf_daf_prepare) puts them: a tap within float32 rounding of a pixel centre
    # may land on either side, and torch's float32 projection does not round as the kernel does
    cams, L, P = const["pm"].shape[1], len(const["levels"]), const["key_pts"]
    moved = 0
    with torch.no_grad():
        for bi, b in enumerate(named["blocks"]):
            kp32 = step_ref._kp(means, scales, b["key_offsets"].detach())
            loc, _ = deformable_prepare(kp32, const["pm"], const["wh"], kp32.new_zeros(1, A, cams, L, P, const["groups"]))
            cells = loc.reshape(1, A, P, cams, 2)
            seen = ((cells > 0) & (cells < 1)).all(-1)
            for h, w in const["levels"]:
                for a_, n in ((1, h), (0, w)):
                    moved += int(((torch.floor(cells[..., a_] * n - 0.5) != torch.floor(dec["cells"][bi][..., a_] * n - 0.5))
                                  & seen).sum())
            dec["cells"][bi] = cells
    if head == "empty":
        assert dec["means_int"][A].tolist() == [100, 100, 8] and int(dec["radii"][A]) == 600

    # the native step, once
    for t in s.leaves:
        t.grad = None
    loss, outs = s.forward()
    if head == "prob":
        s.prob_state = outs[0].grad_fn.saved_tensors[0].clone()
    loss.backward()
    torch.cuda.synchronize()
    path = _path_word(s, outs)

    ref, rgrad = step_ref.step(named, const, dec, torch.float64)
    ref32, rgrad32 = step_ref.step(named, const, dec, torch.float32)
    print(f"\n[{daf} + {head}] splat path word {path}, gate redraws {redrawn} (remaining 0), tap cells where the kernel's "
          f"projection and torch's float32 one differ: {moved}")

    H, W, D = const["grid"]
    N = H * W * D
    lo, hi = step_ref.box_bounds(dec["means_int"], dec["radii"], H, W, D)
    cover = torch.zeros(H + 1, W + 1, D + 1, dtype=torch.int32, device=lo.device)       # boxes -> covered voxels (3-D prefix sums)
    for ix, x in ((0, 1), (1, -1)):
        for iy, y in ((0, 1), (1, -1)):
            for iz, z in ((0, 1), (1, -1)):
                c = torch.stack([(hi if ix else lo)[:, 0], (hi if iy else lo)[:, 1], (hi if iz else lo)[:, 2]], 1)
                ok = ((hi - lo) > 0).all(1)
                cover.index_put_((c[ok, 0], c[ok, 1], c[ok, 2]), torch.full_like(c[ok, 0], x * y * z, dtype=torch.int32),
                                 accumulate=True)
    covered = (cover.cumsum(0).cumsum(1).cumsum(2)[:H, :W, :D] > 0).reshape(N)
    dt = lambda x: x.detach()

    check = lambda got, r, r32, what, rows, rtol=GRAD_RTOL, **kw: assert_daf_rows_close(dt(got), r, r32, f"{head}/{what}", rows, rtol, **kw)
    check(loss.reshape(1, 1), ref["loss"].reshape(1, 1), ref32["loss"].reshape(1, 1), "loss", 1, FWD_RTOL)
    cut_anchor = torch.zeros(A, dtype=torch.bool, device=lo.device)
    if head == "prob":
        ps = ref["prob_sum"]
        near = ((ps - step_ref.CUT).abs() <= CUT_SLACK * step_ref.CUT)
        nv = torch.nonzero(near).squeeze(1)
        if nv.numel():
            vx, vy, vz = nv // (W * D), (nv // D) % W, nv % D
            v3 = torch.stack([vx, vy, vz], 1)
            inside = ((v3[:, None] >= lo[None]) & (v3[:, None] < hi[None])).all(-1).any(0)
            cut_anchor = inside[:A]
        print(f"  prob cut: {int(near.sum())} voxels within {CUT_SLACK:g} relative of it exempt, {int(cut_anchor.sum())} anchors")
        assert int(near.sum()) <= 10
        uncovered = ~covered
        assert bool((outs[0][uncovered] == step_ref.uniform_row(18, torch.float32, lo.device)).all()), "uncovered voxels: uniform row"
        check(outs[0], ref["logits"], ref32["logits"], "logits", 1, FWD_RTOL, exempt=near)
        for k, o in zip(("bin_logits", "density"), outs[1:]):
            check(o.reshape(N, 1), ref[k].reshape(N, 1), ref32[k].reshape(N, 1), k, 1, FWD_RTOL, touched=covered)
    else:
        check(outs[0], ref["logits"], ref32["logits"], "logits", 1, FWD_RTOL, touched=covered)

    # the leaves
    kps = ref["kp"]
    ss = torch.tensor(const["levels"], device=lo.device)
    st = torch.cat([ss.new_zeros(1), torch.cumsum(ss[:, 0] * ss[:, 1], 0)[:-1]])
    num_feat = int((ss[:, 0] * ss[:, 1]).sum())
    edge = _edge_anchors(kps, const, ss)
    n_edge = int(edge.sum())
    print(f"  pixel-centre crossings: {n_edge} anchors exempt on anchor-gradient columns 0:6 (cap {EDGE_CAP}); "
          f"prob-cut anchors {int(cut_anchor.sum())}")
    assert n_edge <= EDGE_CAP
    ga, ra, ra32 = named["anchor"].grad, rgrad["anchor"], rgrad32["anchor"]
    check(ga[..., :6], ra[..., :6], ra32[..., :6], "anchor grad [0:6]", 2, exempt=(edge | cut_anchor)[None])
    check(ga[..., 6:], ra[..., 6:], ra32[..., 6:], "anchor grad [6:11]", 2, exempt=cut_anchor[None])
    check(named["sem_raw"].grad, rgrad["sem_raw"], rgrad32["sem_raw"], "sem_raw grad", 2, exempt=cut_anchor[None])
    check(named["feat0"].grad, rgrad["feat0"], rgrad32["feat0"], "feat0 grad", 2, exempt=cut_anchor[None])
    touched = _touched_pixels(kps, const, ss, st, num_feat)
    for li, (m, r, r32) in enumerate(zip(named["maps"], rgrad["maps"], rgrad32["maps"])):
        h, w = const["levels"][li]
        tl = touched[:, :, int(st[li]):int(st[li]) + h * w].reshape(1, -1, h, w)
        perm = lambda x: x.permute(0, 1, 3, 4, 2)                                       # rows: (camera, pixel)
        check(perm(m.grad), perm(r), perm(r32), f"map{li} grad", 4, touched=tl)
    for bi, (b, r, r32) in enumerate(zip(named["blocks"], rgrad["blocks"], rgrad32["blocks"])):
        check(b["spconv"].grad, r["spconv"], r32["spconv"], f"block{bi} spconv weight grad", 2)
        check(b["fc_weight"].grad, r["fc_weight"], r32["fc_weight"], f"block{bi} weights_fc weight grad", 1)
        check(b["fc_bias"].grad.reshape(-1, 1), r["fc_bias"].reshape(-1, 1), r32["fc_bias"].reshape(-1, 1),
              f"block{bi} weights_fc bias grad", 1)
        check(b["key_offsets"].grad, r["key_offsets"], r32["key_offsets"], f"block{bi} key_offsets grad", 1)
    if head == "empty":
        check(named["empty_scalar"].grad.reshape(1, 1), rgrad["empty_scalar"].reshape(1, 1), rgrad32["empty_scalar"].reshape(1, 1),
              "empty_scalar grad", 1)
