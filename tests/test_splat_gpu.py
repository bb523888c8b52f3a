"""GPU parity of the splat (forward + backward, base / prob / prob_fast) against the CPU
oracle, through the C ABI.  Tolerances: see tests/util.py."""
import numpy as np
import pytest

import oracle
from gaussianformer_amd.synthetic import make_splat_inputs

from util import (GRAD_RTOL, assert_grad_close, assert_grad_rows_close, assert_logits_abs, assert_logits_close,
                  assert_prob_grad_rows_close, grad_row_errors, hip_splat_backward, hip_splat_forward, prep, print_grad_rows,
                  splat_truth_grads, whole_grid_rows)

pytestmark = pytest.mark.gpu

GRAD_NAMES = ("means3D_grad", "opacity_grad", "semantics_grad", "cov3D_grad")

SMALL = [
    # config, P, H, W, D, per_axis
    ("nuscenes_gs25600_solid", 300, 24, 20, 16, False),
    ("nuscenes_gs25600_solid", 257, 23, 21, 16, False),   # H, W not multiples of the 4x4 tile
    ("nuscenes_gs25600_solid", 200, 20, 20, 10, False),   # D not a multiple of 4 (scalar row stores)
    ("nuscenes_gs25600_solid", 200, 20, 20, 40, False),   # D > 16: several z-brick groups per tile
    ("nuscenes_gs144000", 1000, 40, 44, 16, False),
    ("prob_gs6400", 120, 24, 20, 16, False),
    ("prob_gs6400", 120, 24, 20, 16, True),               # localagg_prob_fast: per-axis radii
]


def _oracle_fwd(si, pi, mi, radii, cov6):
    return oracle.splat_forward(si.variant, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6,
                                si.H, si.W, si.D)


def _truth(si, pi, mi, radii, cov6):
    """fp64 dense evaluation (small cases only)."""
    import torch
    from oracle import dense_ref
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    out = dense_ref.splat_dense(si.variant, t(si.pts), torch.tensor(pi), t(si.means3D), torch.tensor(mi),
                                t(si.opacities), t(si.semantics), torch.tensor(radii), t(cov6), si.H, si.W, si.D)
    return [o.numpy() for o in out]


def _check_fwd(got, ref, variant, truth=None):
    if variant != "prob" or truth is None:
        assert_logits_close(got["logits"], ref["logits"], tol=1e-4 if variant != "prob" else 1e-3)
    if variant == "prob":
        # The Prob config's scale range (0.01 .. 3.2 m) makes -1/2 d^T Sigma^-1 d a sum of
        # terms ~1e3 that cancel to ~1e0, so ANY fp32 evaluation of density / probability is
        # only good to ~1e-4 relative (the CUDA reference included: nvcc's FMA contraction
        # differs from both gcc and hipcc).  The prob outputs are therefore judged
        # against the fp64 truth: the HIP result may not be further from it than twice the
        # oracle's own fp32 error (or the plain 1e-4 bound, whichever is larger).
        for i, k in enumerate(("logits", "bin_logits", "density", "probability")):
            if truth is None:
                if k != "logits":
                    assert_logits_close(got[k], ref[k], what=k, tol=1e-3)
                continue
            tr = truth[i]
            scale = np.maximum(1.0, np.abs(tr))
            e_hip = np.abs(got[k] - tr) / scale
            e_orc = np.abs(ref[k] - tr) / scale
            assert np.all(e_hip <= np.maximum(2 * e_orc.max(), 1e-4)), (k, e_hip.max(), e_orc.max())


@pytest.mark.parametrize("config,P,H,W,D,per_axis", SMALL)
def test_forward_dense_small(gpu, config, P, H, W, D, per_axis):
    si = make_splat_inputs(config, seed=3, P=P, H=H, W=W, D=D)
    pi, mi, radii, cov6 = prep(si, per_axis)
    ref = _oracle_fwd(si, pi, mi, radii, cov6)
    truth = _truth(si, pi, mi, radii, cov6) if si.variant == "prob" else None
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    _check_fwd(got, ref, si.variant, truth)
    # the trusted-dense and forced-general paths must agree with the automatic one
    from gaussianformer_amd import _lib
    for flags in (_lib.GF_PTS_ASSUME_DENSE, _lib.GF_PTS_GENERAL):
        got2, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=flags)
        _check_fwd(got2, ref, si.variant, truth)


@pytest.mark.parametrize("config,per_axis", [("nuscenes_gs25600_solid", False), ("prob_gs6400", True)])
def test_forward_arbitrary_points(gpu, config, per_axis):
    """Random query points: several per voxel, most voxels empty (model/head/localagg/debug.py
    shape: N random pts)."""
    si = make_splat_inputs(config, seed=4, P=150, H=20, W=24, D=16, dense_pts=False, N=5000)
    pi, mi, radii, cov6 = prep(si, per_axis)
    ref = _oracle_fwd(si, pi, mi, radii, cov6)
    truth = _truth(si, pi, mi, radii, cov6) if si.variant == "prob" else None
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    _check_fwd(got, ref, si.variant, truth)


def test_forward_permuted_grid_falls_back(gpu):
    """N == H*W*D but points are NOT in canonical voxel order: the dense kernel must
    detect it on the device and the general kernel must produce the result."""
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=5, P=200, H=20, W=20, D=16)
    perm = np.random.default_rng(0).permutation(si.pts.shape[0])
    si.pts = np.ascontiguousarray(si.pts[perm])
    pi, mi, radii, cov6 = prep(si)
    ref = _oracle_fwd(si, pi, mi, radii, cov6)
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    _check_fwd(got, ref, si.variant)


def test_voxel_membership_bit_exact(gpu):
    """Integer path: with Sigma^-1 = 0, opacity = 1, semantics = 1 every covered voxel
    receives exactly 1.0 per covering Gaussian, so logits == per-voxel Gaussian count --
    compared bit-exactly with the oracle; plus tiles_touched / num_rendered
    (src/forward.cu:9-28, src/aggregator_impl.cu:193-197)."""
    import torch
    from gaussianformer_amd.local_aggregate import splat_box_volumes
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=6, P=2000, H=40, W=36, D=16)
    pi, mi, radii, cov6 = prep(si)
    si.opacities[:] = 1.0
    si.semantics[:] = 1.0
    cov6 = np.zeros_like(cov6)
    ref = _oracle_fwd(si, pi, mi, radii, cov6)
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    assert np.array_equal(got["logits"], ref["logits"])
    touched_ref, _, R_ref = oracle.box_offsets(mi, radii, si.H, si.W, si.D)
    touched, R = splat_box_volumes(torch.from_numpy(mi).to(gpu), torch.from_numpy(radii).to(gpu), si.H, si.W, si.D)
    assert np.array_equal(touched.cpu().numpy().astype(np.uint32), touched_ref)
    assert R == R_ref == ref["num_rendered"]


def test_forward_edge_cases(gpu):
    """Empty Gaussian set; a single whole-grid Gaussian; Gaussians whose centre lies
    outside the grid (the reference asserts; we clip the box like getRect does)."""
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=7, P=0, H=12, W=12, D=8)  # only the empty Gaussian
    pi, mi, radii, cov6 = prep(si)
    ref = _oracle_fwd(si, pi, mi, radii, cov6)
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    _check_fwd(got, ref, si.variant)
    # P = 0
    import torch
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import splat_forward
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=gpu)
    pts = torch.from_numpy(si.pts).to(gpu)
    pint = torch.from_numpy(pi).to(gpu)
    logits, *_ = splat_forward(_lib.GF_SPLAT_BASE, pts, pint, z(0, 3), z(0, 3, dt=torch.int32), z(0), z(0, 18),
                               z(0, dt=torch.int32), z(0, 6), si.H, si.W, si.D)
    assert float(logits.abs().max()) == 0.0
    lp, bl, de, pr, _ = splat_forward(_lib.GF_SPLAT_PROB, pts, pint, z(0, 3), z(0, 3, dt=torch.int32), z(0), z(0, 18),
                                      z(0, dt=torch.int32), z(0, 6), si.H, si.W, si.D)
    assert torch.allclose(lp[:, :17], torch.full_like(lp[:, :17], 1.0 / 17)) and float(lp[:, 17].abs().max()) == 0.0
    assert float(bl.abs().max()) == 0.0 and float(de.abs().max()) == 0.0 and float(pr.abs().max()) == 0.0
    # centres outside the grid
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=8, P=100, H=16, W=16, D=8)
    si.means3D[:50] += np.float32(3.0)
    pi, mi, radii, cov6 = prep(si)
    ref = _oracle_fwd(si, pi, mi, radii, cov6)
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    _check_fwd(got, ref, si.variant)


def test_forward_crowded_tile(gpu):
    """Thousands of Gaussians in one supertile: exercises the candidate sub-pass path and
    the LDS list flush (lists far longer than the LDS capacity)."""
    si = make_splat_inputs("nuscenes_gs144000", seed=9, P=6000, H=20, W=20, D=16)
    pi, mi, radii, cov6 = prep(si)
    ref = _oracle_fwd(si, pi, mi, radii, cov6)
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    _check_fwd(got, ref, si.variant)


@pytest.mark.parametrize("config,P,H,W,D,per_axis", SMALL)
def test_backward_small(gpu, config, P, H, W, D, per_axis):
    si = make_splat_inputs(config, seed=11, P=P, H=H, W=W, D=D)
    pi, mi, radii, cov6 = prep(si, per_axis)
    rng = np.random.default_rng(12)
    N = si.pts.shape[0]
    g = rng.standard_normal((N, 18)).astype(np.float32)
    gb = rng.standard_normal(N).astype(np.float32) if si.variant == "prob" else None
    gd = rng.standard_normal(N).astype(np.float32) if si.variant == "prob" else None
    fwd = _oracle_fwd(si, pi, mi, radii, cov6)
    ref = oracle.splat_backward(si.variant, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6,
                                si.H, si.W, si.D, g, fwd=fwd, bin_grad=gb, density_grad=gd)
    _, t, state, fwd_t = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    got = hip_splat_backward(gpu, si, t, state, fwd_t, g, gb, gd)
    for name, a, b in zip(GRAD_NAMES, got, ref):
        assert_grad_close(a, b, what=name)
    # row by row: every Gaussian against its own magnitude (tests/util.py) -- the base variant against the oracle, the prob
    # variant (whose fp32 quadratic form cancels, in the oracle as in any fp32 evaluation) against float64 autograd with the
    # oracle's own error on the row as the yardstick
    print()
    if si.variant == "prob":
        for name, a, b, tr in zip(GRAD_NAMES, got, ref, splat_truth_grads(si, pi, mi, radii, cov6, g, gb, gd)):
            assert_prob_grad_rows_close(a, tr, b, what=f"{name} [{config} per_axis={per_axis}]")
    else:
        whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
        for name, a, b in zip(GRAD_NAMES, got, ref):
            print_grad_rows(f"{name} [{config} P={P} {H}x{W}x{D}]", assert_grad_rows_close(a, b, whole, what=name, rtol=GRAD_RTOL))


def test_backward_arbitrary_points(gpu):
    """Duplicate-voxel points: only the highest-index point of a voxel feeds the gradient
    (voxel2pts semantics, backward.cu:18-19, made deterministic)."""
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=13, P=150, H=20, W=24, D=16, dense_pts=False, N=20000)
    pi, mi, radii, cov6 = prep(si)
    g = np.random.default_rng(14).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    ref = oracle.splat_backward("base", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6,
                                si.H, si.W, si.D, g)
    _, t, state, fwd_t = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    got = hip_splat_backward(gpu, si, t, state, fwd_t, g)
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    print()
    for name, a, b in zip(GRAD_NAMES, got, ref):
        assert_grad_close(a, b, what=name)
        print_grad_rows(f"{name} [arbitrary points]", assert_grad_rows_close(a, b, whole, what=name, rtol=GRAD_RTOL))


@pytest.mark.parametrize("per_axis", [False, True])
def test_backward_arbitrary_points_prob(gpu, per_axis):
    """The prob variant's backward (localagg_prob / localagg_prob_fast) on random query points: several per voxel, only the
    highest-index point of a voxel feeds the gradient (voxel2pts), most voxels empty; with bin_grad and density_grad.  Judged row
    by row against float64 autograd with the oracle's own error on the row as the yardstick (tests/util.py).

    The seed is the first from 37 on at which the oracle ALONE qualifies for both radius flavours (chosen on the CPU, no HIP result
    involved; 37, 38 do not, 39, 42 and 45 do): its forward is finite, each of its gradients is within 1e-2 of the truth
    tensor-wide (the sweep's criterion) and at most 5 % of the rows are on the fp32 term.  Seed 39 (gradients: seed 40), P = 120,
    oracle vs float64, (means3D, opacity, semantics, cov3D):
      scalar radii    tensor-wide 4.0e-5, 9.9e-5, 2.6e-4, 5e-6; rows on the fp32 term 1.7 %, 0.8 %, 0.8 %, 0
      per-axis radii  tensor-wide 4.4e-5, 5.7e-5, 1.0e-4, 5e-6; rows on the fp32 term 0.8 %, 2.5 %, 0.8 %, 0"""
    si = make_splat_inputs("prob_gs6400", seed=39, P=120, H=20, W=24, D=16, dense_pts=False, N=5000)
    pi, mi, radii, cov6 = prep(si, per_axis)
    rng = np.random.default_rng(40)
    N = si.pts.shape[0]
    g = rng.standard_normal((N, 18)).astype(np.float32)
    gb = rng.standard_normal(N).astype(np.float32)
    gd = rng.standard_normal(N).astype(np.float32)
    fwd = _oracle_fwd(si, pi, mi, radii, cov6)
    assert all(np.isfinite(v).all() for v in fwd.values() if isinstance(v, np.ndarray))
    ref = oracle.splat_backward("prob", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6,
                                si.H, si.W, si.D, g, fwd=fwd, bin_grad=gb, density_grad=gd)
    truth = splat_truth_grads(si, pi, mi, radii, cov6, g, gb, gd)
    for name, b, tr in zip(GRAD_NAMES, ref, truth):     # the oracle qualifies (the figures of the docstring)
        assert np.isfinite(b).all() and np.abs(b - tr).max() <= 1e-2 * max(np.abs(tr).max(), 1e-6), name
    got_f, t, state, fwd_t = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    _check_fwd(got_f, fwd, "prob", _truth(si, pi, mi, radii, cov6))
    got = hip_splat_backward(gpu, si, t, state, fwd_t, g, gb, gd)
    print()
    for name, a, b, tr in zip(GRAD_NAMES, got, ref, truth):
        assert_prob_grad_rows_close(a, tr, b, what=f"{name} [prob, arbitrary points, per_axis={per_axis}]")


def test_module_autograd_matches_oracle(gpu):
    """Through the drop-in ``local_aggregate.LocalAggregator`` module + autograd, including
    the [0,4,8,1,5,2] gather of the 3x3 inverse covariance
    (model/head/localagg/local_aggregate/__init__.py:143)."""
    import torch
    import local_aggregate
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=15, P=300, H=24, W=20, D=16)
    agg = local_aggregate.LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size).to(gpu)
    assert "pc_min" in agg.state_dict()
    tt = lambda a, g=False: torch.from_numpy(a).to(gpu)[None].requires_grad_(g)
    means, opa, sem, cov = tt(si.means3D, True), tt(si.opacities, True), tt(si.semantics, True), tt(si.cov3D, True)
    logits = agg(tt(si.pts), means, opa, sem, tt(si.scales), cov)
    gout = np.random.default_rng(16).standard_normal(tuple(logits.shape)).astype(np.float32)
    logits.backward(torch.from_numpy(gout).to(gpu))
    pi, mi, radii, cov6 = prep(si)
    ref = _oracle_fwd(si, pi, mi, radii, cov6)
    assert_logits_close(logits.detach().cpu().numpy(), ref["logits"])
    rg = oracle.splat_backward("base", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6,
                               si.H, si.W, si.D, gout)
    assert_grad_close(means.grad[0].cpu().numpy(), rg[0], "means3D.grad")
    assert_grad_close(opa.grad[0].cpu().numpy(), rg[1], "opacities.grad")
    assert_grad_close(sem.grad[0].cpu().numpy(), rg[2], "semantics.grad")
    cg = cov.grad[0].cpu().numpy().reshape(-1, 9)
    assert_grad_close(cg[:, [0, 4, 8, 1, 5, 2]], rg[3], "cov3D.grad (packed entries)")
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    print()
    for name, a, b in zip(("means3D.grad", "opacities.grad", "semantics.grad", "cov3D.grad (packed entries)"),
                          (means.grad[0].cpu().numpy(), opa.grad[0].cpu().numpy(), sem.grad[0].cpu().numpy(), cg[:, [0, 4, 8, 1, 5, 2]]), rg):
        print_grad_rows(f"{name} [module]", assert_grad_rows_close(a, b, whole, what=name, rtol=GRAD_RTOL))
    assert np.abs(cg[:, [3, 6, 7]]).max() == 0.0  # lower triangle receives nothing


@pytest.mark.parametrize("config", ["nuscenes_gs25600_solid", "nuscenes_gs144000"])
def test_forward_full_size(gpu, config):
    """BASELINE.json configs at full size (200x200x16, P = 25 601 / 144 000) vs the oracle."""
    si = make_splat_inputs(config, seed=0)
    pi, mi, radii, cov6 = prep(si)
    ref = _oracle_fwd(si, pi, mi, radii, cov6)
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    _check_fwd(got, ref, si.variant)
    a = assert_logits_abs(got["logits"], ref["logits"], what=f"logits vs the oracle, ABSOLUTE [{config}]")
    print(f"\n[{config}] max ABSOLUTE logits err vs the oracle {a:.3e} (max|logit| {np.abs(ref['logits']).max():.3e})")
    # size-independent properties: linearity in semantics and in opacity
    si2 = make_splat_inputs(config, seed=0)
    si2.semantics *= np.float32(2.0)
    got2, *_ = hip_splat_forward(gpu, si2, pi, mi, radii, cov6)
    # (default flags = the matrix-core kernel: its f16 operand split is linear up to the last bit of the lo term)
    assert np.allclose(got2["logits"], np.float32(2.0) * got["logits"], rtol=2e-6, atol=1e-6)
    # deterministic: same bits on a second run
    from gaussianformer_amd import _lib
    again, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    assert np.array_equal(again["logits"], got["logits"])
    # the exact-fp32 tile kernel: power-of-two scaling is exact in fp32 except where a product lands in the denormal
    # range, and the arbitrary-points kernel (same ascending Gaussian order per voxel) reproduces it bit for bit
    exact, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_EXACT_FP32)
    _check_fwd(exact, ref, si.variant)
    exact2, *_ = hip_splat_forward(gpu, si2, pi, mi, radii, cov6, flags=_lib.GF_EXACT_FP32)
    assert np.allclose(exact2["logits"], np.float32(2.0) * exact["logits"], rtol=0, atol=1e-35)
    general, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PTS_GENERAL)
    assert np.array_equal(general["logits"], exact["logits"])
    assert_logits_close(got["logits"], exact["logits"], what="matrix-core vs exact-fp32 kernel", tol=1e-4)


@pytest.mark.parametrize("config", ["nuscenes_gs25600_solid", "nuscenes_gs144000"])
def test_backward_full_size(gpu, config):
    si = make_splat_inputs(config, seed=0)
    pi, mi, radii, cov6 = prep(si)
    g = np.random.default_rng(1).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    ref = oracle.splat_backward("base", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6,
                                si.H, si.W, si.D, g)
    _, t, state, fwd_t = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    got = hip_splat_backward(gpu, si, t, state, fwd_t, g)
    # row by row: every Gaussian against its own magnitude (floor: the median ordinary row); the whole-grid "empty"
    # Gaussian, whose row is 1e4 times an ordinary one at gs25600, is judged by itself (tests/util.py)
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    for name, a, b in zip(("means3D_grad", "opacity_grad", "semantics_grad", "cov3D_grad"), got, ref):
        e = assert_grad_rows_close(a, b, whole, what=f"{name} [{config}]")
        print(f"\n[{config}] {name} vs the oracle: worst ordinary row {e['ordinary']:.3e} (floor {e['floor']:.3e}), "
              f"whole-grid row {e['whole_grid']:.3e}, tensor-wide {e['tensor']:.3e}")


@pytest.mark.parametrize("mode", ["exact", "fast", "libm", "comp"])
def test_exp_modes(gpu, mode):
    """The three exp() flavours of the exact-fp32 kernels (include/gf_hip.h) all meet the logits tolerance;
    GF_EXACT_FP32 alone is the log2(e)-prescaled v_exp_f32 (GF_FAST_EXP)."""
    from gaussianformer_amd import _lib
    flags = {"exact": _lib.GF_EXACT_FP32, "fast": _lib.GF_FAST_EXP, "libm": _lib.GF_LIBM_EXP, "comp": _lib.GF_COMP_EXP}[mode]
    for config in ("nuscenes_gs25600_solid", "nuscenes_gs144000"):
        si = make_splat_inputs(config, seed=17, P=3000, H=48, W=40, D=16)
        pi, mi, radii, cov6 = prep(si)
        ref = _oracle_fwd(si, pi, mi, radii, cov6)
        got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=flags)
        assert_logits_close(got["logits"], ref["logits"], tol=2e-5)  # 5x margin on the 1e-4 bound
        gen, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=flags | _lib.GF_PTS_GENERAL)
        assert np.array_equal(gen["logits"], got["logits"])


def test_backward_channel_major_gradient(gpu):
    """The gradient autograd produces when the loss consumed logits[None].transpose(1, 2)
    ([1,18,N], gaussian_head.py:176) is a transposed (non-contiguous) view; the wrapper must
    handle it and give the same result as a contiguous [N,18] gradient."""
    import torch
    import local_aggregate
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=19, P=400, H=24, W=24, D=16)
    agg = local_aggregate.LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size).to(gpu)
    tt = lambda a, g=False: torch.from_numpy(a).to(gpu)[None].requires_grad_(g)
    wgt = torch.from_numpy(np.random.default_rng(20).standard_normal((1, 18, si.pts.shape[0])).astype(np.float32)).to(gpu)
    grads = []
    for transposed in (True, False):
        means, opa, sem, cov = tt(si.means3D, True), tt(si.opacities, True), tt(si.semantics, True), tt(si.cov3D, True)
        logits = agg(tt(si.pts), means, opa, sem, tt(si.scales), cov)
        if transposed:
            (logits[None].transpose(1, 2) * wgt).sum().backward()      # grad arrives as a [N,18] view of [18,N]
        else:
            logits.backward(wgt[0].t().contiguous())
        grads.append([t.grad.clone() for t in (means, opa, sem, cov)])
    pi, mi, radii, cov6 = prep(si)
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    print()
    for name, a, b in zip(GRAD_NAMES, *grads):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))
        # ... and row by row: |a - b| <= 1e-6 * max|row| + 1e-5 * |b|, the row's maximum floored at the median ordinary row's
        a2, b2 = (x[0].reshape(b.shape[1], -1).double().cpu().numpy() for x in (a, b))
        rowmax = np.abs(b2).max(axis=1)
        floor = float(np.median(rowmax[~whole]))
        excess = np.abs(a2 - b2) - (1e-6 * np.maximum(rowmax, floor)[:, None] + 1e-5 * np.abs(b2))
        e = grad_row_errors(a2, b2, whole)
        print_grad_rows(f"{name} [transposed vs contiguous gradient]", e)
        assert excess.max() <= 0.0, (name, int(excess.max(axis=1).argmax()), float(excess.max()))


def test_random_shapes_sweep(gpu):
    """Randomised sweep over grid shapes, Gaussian counts, variants and radius flavours: forward
    and backward against the oracle (dense grid and arbitrary points).  The prob variant's
    gradient divides by 1 - exp(.) + 1e-9 (localagg_prob/src/backward.cu:93), so a point that
    happens to sit next to a mean amplifies one-ulp differences in exp(); there both the HIP
    path and the oracle are judged against fp64 autograd instead of against each other."""
    import os
    rng = np.random.default_rng(int(os.environ.get("GF_SWEEP_SEED", "2025")))
    fwd_skipped, prob_trials, grad_skipped = [], 0, []        # what the sweep did NOT check: counted, printed, bounded
    print()
    for trial in range(int(os.environ.get("GF_SWEEP_TRIALS", "14"))):
        config = ["nuscenes_gs25600_solid", "nuscenes_gs144000", "prob_gs6400"][trial % 3]
        prob = config == "prob_gs6400"
        hi = 25 if prob else 45
        H, W, D = int(rng.integers(5, hi)), int(rng.integers(5, hi)), int(rng.integers(1, 25 if prob else 34))
        P = int(rng.integers(1, 120 if prob else 700))
        per_axis = prob and bool(rng.integers(0, 2))
        dense = bool(rng.integers(0, 4))  # mostly the dense grid, sometimes random points
        si = make_splat_inputs(config, seed=1000 + trial, P=P, H=H, W=W, D=D, dense_pts=dense,
                               N=None if dense else int(rng.integers(1, 3000)))
        pi, mi, radii, cov6 = prep(si, per_axis)
        ref = _oracle_fwd(si, pi, mi, radii, cov6)
        truth = _truth(si, pi, mi, radii, cov6) if prob else None
        if not all(np.isfinite(v).all() for v in ref.values() if isinstance(v, np.ndarray)):
            # prob config, scales down to 0.01 m: det(Sigma^-1) can round to a negative fp32 and
            # the reference's powf(deter, 0.5) (localagg_prob/src/forward.cu:78) is then NaN --
            # no defined result to compare against
            fwd_skipped.append(trial)
            continue
        got, t, state, fwd_t = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
        try:
            _check_fwd(got, ref, si.variant, truth)
            N = si.pts.shape[0]
            g = rng.standard_normal((N, 18)).astype(np.float32)
            gb = rng.standard_normal(N).astype(np.float32) if prob else None
            gd = rng.standard_normal(N).astype(np.float32) if prob else None
            refg = oracle.splat_backward(si.variant, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6,
                                         si.H, si.W, si.D, g, fwd=ref, bin_grad=gb, density_grad=gd)
            gotg = hip_splat_backward(gpu, si, t, state, fwd_t, g, gb, gd)
            names = GRAD_NAMES
            if not prob:
                whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
                for name, a, b in zip(names, gotg, refg):
                    assert_grad_close(a, b, what=name)
                    print_grad_rows(f"trial {trial} {name} [{config} P={P} {H}x{W}x{D} dense={dense}]",
                                    assert_grad_rows_close(a, b, whole, what=name, rtol=GRAD_RTOL))
            else:
                prob_trials += 1
                for name, a, b, tr in zip(names, gotg, refg, splat_truth_grads(si, pi, mi, radii, cov6, g, gb, gd)):
                    scale = max(np.abs(tr).max(), 1e-6)
                    e_orc = np.abs(b - tr).max() / scale
                    if not np.isfinite(b).all() or e_orc > 1e-2:    # (reads the oracle and the truth only)
                        grad_skipped.append((trial, name))
                        continue  # the reference's own fp32 formula breaks down on this input
                    e_hip = np.abs(a - tr).max() / scale
                    assert e_hip <= max(3 * e_orc, 1e-3), f"{name}: HIP err {e_hip:.2e}, oracle err {e_orc:.2e} (vs fp64)"
        except AssertionError as e:
            raise AssertionError(f"trial {trial}: {config} P={P} grid {H}x{W}x{D} per_axis={per_axis} dense={dense}: {e}")
    print(f"  sweep: forward not compared in trials {fwd_skipped} (oracle not finite); prob gradient tensors not compared: "
          f"{len(grad_skipped)} of {4 * prob_trials} {grad_skipped}")
    # default seed, 14 trials: 4 of 16, all in trial 2 (P=13, 21x14x8, arbitrary points -- test_backward_arbitrary_points_prob
    # covers that path on an input the oracle can judge)
    assert 4 * len(grad_skipped) <= 4 * prob_trials, f"the sweep skipped {len(grad_skipped)} of {4 * prob_trials} prob gradient tensors: {grad_skipped}"


def test_forward_pipeline_two_streams(gpu):
    """Two frames in flight on two streams (SplatForwardPipeline) give the bits of a plain call."""
    import torch
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import SplatForwardPipeline
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=31, P=5000, H=64, W=48, D=16)
    pi, mi, radii, cov6 = prep(si)
    ref, t, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    pipe = SplatForwardPipeline(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D)
    outs = [pipe.submit() for _ in range(6)]
    for logits, ev in outs[-2:]:
        ev.synchronize()
        assert np.array_equal(logits.cpu().numpy(), ref["logits"])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_forward_is_graph_capturable(gpu):
    """The forward C-ABI call only enqueues work on the given stream (no allocation, no synchronisation, no host
    read), so it can be captured into a HIP graph (torch.cuda.CUDAGraph on ROCm) and replayed."""
    import torch
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import SplatForwardPlan
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=23, P=2000, H=48, W=40, D=16)
    pi, mi, radii, cov6 = oracle.prepare_splat_inputs(si.pts, si.means3D, si.scales, si.cov3D, si.pc_min, si.grid_size,
                                                      si.scale_multiplier)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6)]
    plan = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=_lib.GF_PTS_AUTO)
    eager = plan.run().clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):      # warm-up on the capture stream, as torch recommends
        plan.run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.run()
    for _ in range(3):
        plan.logits.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(plan.logits, eager)


def test_module_backward_with_strided_and_fp64_inputs(gpu):
    """Autograd saves the caller's tensors: strided views (``semantics = output[..., 10:]``-style slices,
    means as an anchor slice) and fp64 inputs must give the gradients of the contiguous fp32 call -- the
    backward coerces its arguments like the forward does (the reference: ``.contiguous().data<float>()`` on
    every backward argument, local_aggregate.cu:116-127)."""
    import torch
    import local_aggregate
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=33, P=300, H=24, W=20, D=16)
    agg = local_aggregate.LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size).to(gpu)
    P = si.means3D.shape[0]
    g = torch.from_numpy(np.random.default_rng(34).standard_normal((si.pts.shape[0], 18)).astype(np.float32)).to(gpu)
    tt = lambda a: torch.from_numpy(a).to(gpu)

    def run(make):
        packed = torch.zeros(1, P, 3 + 5 + 18, device=gpu, dtype=make)      # anchor-like row: mean | pad | semantics
        packed[0, :, :3] = tt(si.means3D).to(make)
        packed[0, :, 8:] = tt(si.semantics).to(make)
        packed.requires_grad_(True)
        opa = tt(si.opacities).to(make)[None].requires_grad_(True)
        cov = tt(si.cov3D).to(make)[None].requires_grad_(True)
        means, sem = packed[..., :3], packed[..., 8:]                       # non-contiguous views
        assert not sem.is_contiguous()
        logits = agg(tt(si.pts)[None], means, opa, sem, tt(si.scales)[None], cov)
        logits.backward(g)
        return logits.detach(), packed.grad.float(), opa.grad.float(), cov.grad.float()

    base = run(torch.float32)
    # contiguous fp32 reference call
    m, o, s_, c = (tt(a)[None].requires_grad_(True) for a in (si.means3D, si.opacities, si.semantics, si.cov3D))
    ref_logits = agg(tt(si.pts)[None], m, o, s_, tt(si.scales)[None], c)
    ref_logits.backward(g)
    assert torch.equal(base[0], ref_logits.detach())
    # gradients of boxes split over several waves are combined with float atomics: equal up to summation order
    close = lambda a, b: torch.allclose(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))
    assert close(base[1][0, :, :3], m.grad[0]) and close(base[1][0, :, 8:], s_.grad[0])
    assert float(base[1][0, :, 3:8].abs().max()) == 0.0
    assert close(base[2], o.grad) and close(base[3], c.grad)
    dbl = run(torch.float64)
    for a, b in zip(dbl[1:], base[1:]):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))


def test_backward_without_points(gpu):
    """N == 0 with P > 0: zero gradients, no fault (the kernels read row 0 of pts / logits_grad unconditionally)."""
    import torch
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import splat_backward
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=35, P=50, H=12, W=12, D=8)
    pi, mi, radii, cov6 = prep(si)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in
         (si.pts[:0], pi[:0], si.means3D, mi, si.opacities, si.semantics, radii, cov6)]
    grads = splat_backward(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, torch.zeros(0, 18, device=gpu))
    torch.cuda.synchronize()
    assert all(float(x.abs().max()) == 0.0 for x in grads)


def test_module_range_asserts_like_the_reference(gpu):
    """The reference asserts in-grid points / centres and radii >= 1 on every call
    (local_aggregate/__init__.py:138-142); the drop-in keeps that by default."""
    import torch
    import local_aggregate
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=36, P=40, H=12, W=12, D=8)
    agg = local_aggregate.LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size).to(gpu)
    tt = lambda a: torch.from_numpy(a).to(gpu)[None]
    args = [tt(si.pts), tt(si.means3D), tt(si.opacities), tt(si.semantics), tt(si.scales), tt(si.cov3D)]
    agg(*args)
    bad = [a.clone() for a in args]
    bad[1][0, 3, 0] += 100.0                      # a centre outside the grid
    with pytest.raises(AssertionError):
        agg(*bad)
    bad = [a.clone() for a in args]
    bad[0][0, 5, 2] -= 50.0                       # a query point outside the grid
    with pytest.raises(AssertionError):
        agg(*bad)
    quiet = local_aggregate.LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size,
                                            check_inputs=False).to(gpu)
    bad = [a.clone() for a in args]
    bad[1][0, 3, 0] += 100.0
    quiet(*bad)                                    # opt-out: boxes are clipped like getRect
    torch.cuda.synchronize()
