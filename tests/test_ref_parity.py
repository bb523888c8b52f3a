"""Parity against the REFERENCE's own kernels (``oracle/_ref``: the reference's CUDA sources compiled for
gfx950 by ``oracle/ref_build.py`` and executed on this GPU).

Two things are pinned here:

1. the C restatement ``oracle/gf_oracle.c`` (the checker every other test uses) against the reference:
   the binning bit for bit (``tiles_touched``, the inclusive scan, ``num_rendered``, the per-Gaussian key
   list of ``duplicateWithKeys`` and the radix-sorted per-voxel lists), values and gradients within the
   rounding of a different FMA contraction;
2. the HIP product path, through the C ABI, directly against the reference: integer outputs bit-exact,
   logits ``|err| <= 1e-4 * max(1, |ref|)``, gradients ``<= 1e-3`` of the tensor's largest magnitude and, base variant,
   of every Gaussian's own row (prob: row by row against float64 autograd, the reference held to the same bound) —
   small shapes with the edge cases and all three BASELINE shapes at full size.
"""
import numpy as np
import pytest

import oracle
from oracle import ref
from gaussianformer_amd.synthetic import make_daf_inputs, make_splat_inputs

from util import (GRAD_RTOL, assert_grad_close, assert_grad_rows_close, assert_logits_abs, assert_logits_close,
                  assert_prob_grad_rows_close, grad_row_errors, hip_splat_backward, hip_splat_forward, prep, print_grad_rows,
                  prob_row_errors, splat_truth_grads, to_dev, whole_grid_rows)

pytestmark = pytest.mark.gpu

GRAD_NAMES = ("means3D_grad", "opacity_grad", "semantics_grad", "cov3D_grad")


@pytest.fixture(scope="module")
def reflib(gpu):
    if not ref.available():
        pytest.skip("oracle/_ref not built (python -m oracle.ref_build, needs /root/reference)")
    return ref


def _args(si, pi, mi, radii, cov6):
    return (si.variant, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, si.H, si.W, si.D)


def _rand_grads(si, seed):
    rng = np.random.default_rng(seed)
    N = si.pts.shape[0]
    g = rng.standard_normal((N, 18)).astype(np.float32)
    if si.variant == "prob":
        return g, rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    return g, None, None


def _expected_keys(mi, radii, H, W, D):
    """Per-Gaussian voxel keys in the order duplicateWithKeys writes them (aggregator_impl.cu:55-86):
    box from getRect (auxiliary.h:8-20), x outer / z inner, key = x*W*D + y*D + z."""
    keys = []
    r3 = radii if radii.ndim == 2 else np.repeat(radii[:, None], 3, axis=1)
    dims = np.array([H, W, D])
    lo = np.minimum(dims, np.maximum(0, mi - r3))
    hi = np.minimum(dims, np.maximum(0, mi + r3 + 1))
    for g in range(mi.shape[0]):
        xs, ys, zs = (np.arange(lo[g, a], hi[g, a], dtype=np.int64) for a in range(3))
        if len(xs) * len(ys) * len(zs) == 0:
            continue
        k = (xs[:, None, None] * W + ys[None, :, None]) * D + zs[None, None, :]
        keys.append((k.reshape(-1), np.full(k.size, g, np.int64)))
    if not keys:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate([k for k, _ in keys]), np.concatenate([g for _, g in keys])


# ------------------------------------------------------------------------------------------------
# 1. the restatement (oracle/gf_oracle.c) against the reference
# ------------------------------------------------------------------------------------------------

SMALL = [
    ("nuscenes_gs25600_solid", 300, 24, 20, 16, False),
    ("nuscenes_gs25600_solid", 257, 23, 21, 16, False),
    ("nuscenes_gs144000", 1000, 40, 44, 16, False),
    ("prob_gs6400", 120, 24, 20, 16, False),
    ("prob_gs6400", 120, 24, 20, 16, True),
]


@pytest.mark.parametrize("config,P,H,W,D,per_axis", SMALL)
def test_binning_bit_exact_vs_reference(reflib, config, P, H, W, D, per_axis):
    """tiles_touched / scan / num_rendered / duplicateWithKeys / radix sort / ranges of the reference against
    the restated integer path, and the HIP path's own integer outputs against the reference."""
    import torch
    from gaussianformer_amd.local_aggregate import splat_box_volumes
    si = make_splat_inputs(config, seed=41, P=P, H=H, W=W, D=D)
    pi, mi, radii, cov6 = prep(si, per_axis)
    r = reflib.splat_forward(*_args(si, pi, mi, radii, cov6), with_binning=True)
    touched, offsets, R = oracle.box_offsets(mi, radii, H, W, D)
    assert r["num_rendered"] == R
    assert np.array_equal(r["tiles_touched"], touched)
    assert np.array_equal(r["point_offsets"], offsets)
    keys, gids = _expected_keys(mi, radii, H, W, D)
    assert np.array_equal(r["keys_unsorted"].astype(np.int64), keys)
    # the sort is stable: per voxel, Gaussians in ascending index (the summation order every kernel here reproduces)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(r["point_list"].astype(np.int64), gids[order])
    counts = np.bincount(keys, minlength=H * W * D)
    ends = np.cumsum(counts)
    rg = r["ranges"].astype(np.int64)
    nz = counts > 0
    assert np.array_equal(rg[nz, 0], (ends - counts)[nz]) and np.array_equal(rg[nz, 1], ends[nz])
    assert not rg[~nz].any()
    # HIP integer outputs against the reference
    vols, R_hip = splat_box_volumes(torch.from_numpy(mi).to("cuda"), torch.from_numpy(radii).to("cuda"), H, W, D)
    assert R_hip == r["num_rendered"]
    assert np.array_equal(vols.cpu().numpy().astype(np.uint32), r["tiles_touched"])


@pytest.mark.parametrize("config,P,H,W,D,per_axis", SMALL)
def test_oracle_restatement_vs_reference(reflib, config, P, H, W, D, per_axis):
    si = make_splat_inputs(config, seed=43, P=P, H=H, W=W, D=D)
    pi, mi, radii, cov6 = prep(si, per_axis)
    g, gb, gd = _rand_grads(si, 44)
    rf, rgrads, _ = reflib.splat_forward_backward(*_args(si, pi, mi, radii, cov6), g, gb, gd)
    of = oracle.splat_forward(*_args(si, pi, mi, radii, cov6))
    assert of["num_rendered"] == rf["num_rendered"]
    prob = si.variant == "prob"
    for k in (("logits", "bin_logits", "density", "probability") if prob else ("logits",)):
        # the prob config's quadratic form cancels ~1e3 -> ~1e0: contraction moves the fp32 result by ~1e-4
        assert_logits_close(of[k], rf[k], what=f"oracle {k} vs reference", tol=1e-3 if prob else 2e-6)
    ograds = oracle.splat_backward(*_args(si, pi, mi, radii, cov6), g, fwd=of, bin_grad=gb, density_grad=gd)
    for name, a, b in zip(GRAD_NAMES, ograds, rgrads):
        assert_grad_close(a, b, what=f"oracle {name} vs reference", rtol=2e-2 if prob else 1e-5)


def test_oracle_daf_vs_reference(reflib):
    d = make_daf_inputs(num_pts=3000, seed=45, levels=((27, 50), (14, 25), (7, 13), (4, 7)))
    loc = d["sampling_location"]
    loc[0, 0, 0] = [0.0, 0.5]
    loc[0, 1, 0] = [0.999, 0.001]
    loc[0, 2, 0] = [1.0, 1.0]
    out_r = reflib.daf_forward(**d)
    out_o = oracle.daf_forward(**d)
    assert_logits_close(out_o, out_r, what="oracle daf vs reference", tol=2e-6)
    g = np.random.default_rng(46).standard_normal(out_r.shape).astype(np.float32)
    gr = reflib.daf_backward(d["mc_ms_feat"], d["spatial_shape"], d["scale_start_index"], d["sampling_location"], d["weights"], g)
    go = oracle.daf_backward(d["mc_ms_feat"], d["spatial_shape"], d["scale_start_index"], d["sampling_location"], d["weights"], g)
    for name, a, b in zip(("grad_mc_ms_feat", "grad_sampling_location", "grad_weights"), go, gr):
        assert_grad_close(a, b, what=f"oracle {name} vs reference", rtol=2e-5)   # float atomics: order only


# ------------------------------------------------------------------------------------------------
# 2. the HIP path against the reference
# ------------------------------------------------------------------------------------------------

def _rows_vs_ref(si, per_axis, grads, rgrads, what):
    """Every Gaussian's gradient row against the reference's, by its own magnitude (tests/util.py); printed."""
    _, mi, radii, _ = prep(si, per_axis)
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    print()
    for name, a, b in zip(GRAD_NAMES, grads, rgrads):
        print_grad_rows(f"HIP {name} vs reference ({what})",
                        assert_grad_rows_close(a, b, whole, what=f"HIP {name} vs reference ({what})", rtol=GRAD_RTOL))


def _hip_vs_ref(gpu, reflib, si, per_axis, seed, flags=0, logit_tol=1e-4):
    pi, mi, radii, cov6 = prep(si, per_axis)
    g, gb, gd = _rand_grads(si, seed)
    rf, rgrads, v2p = reflib.splat_forward_backward(*_args(si, pi, mi, radii, cov6), g, gb, gd)
    got, t, state, fwd_t = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=flags)
    stats = {}
    for k in (("logits", "bin_logits", "density", "probability") if si.variant == "prob" else ("logits",)):
        assert_logits_close(got[k], rf[k], what=f"HIP {k} vs reference", tol=logit_tol)
        stats[k] = float((np.abs(got[k].astype(np.float64) - rf[k]) / np.maximum(1.0, np.abs(rf[k]))).max())
    grads = hip_splat_backward(gpu, si, t, state, fwd_t, g, gb, gd, flags=flags)
    return rf, rgrads, grads, stats


@pytest.mark.parametrize("config,P,H,W,D,per_axis", SMALL + [
    ("nuscenes_gs25600_solid", 200, 20, 20, 10, False),
    ("nuscenes_gs25600_solid", 200, 20, 20, 40, False),
    ("nuscenes_gs144000", 6000, 20, 20, 16, False),      # crowded tiles
])
def test_hip_small_vs_reference(gpu, reflib, config, P, H, W, D, per_axis):
    si = make_splat_inputs(config, seed=47, P=P, H=H, W=W, D=D)
    prob = si.variant == "prob"
    # north_star's bounds for every variant: fp32 outputs within 1e-4, gradients within 1e-3 of the tensor's maximum
    # (base variant, default flags: the matrix-core kernel renders the forward)
    rf, rgrads, grads, _ = _hip_vs_ref(gpu, reflib, si, per_axis, 48, logit_tol=1e-4)
    for name, a, b in zip(GRAD_NAMES, grads, rgrads):
        if prob and not np.isfinite(b).all():
            continue
        assert_grad_close(a, b, what=f"HIP {name} vs reference", rtol=1e-3)
    if not prob:
        _rows_vs_ref(si, per_axis, grads, rgrads, f"{config} P={P} {H}x{W}x{D}")
        return
    # prob: the reference's fp32 quadratic form cancels like any other, so the truth is float64 autograd and the yardstick the
    # oracle's own error on the row (tests/util.py); the reference is held to the same bound as the HIP path.  Seed 47 does not
    # qualify for that judgement by the oracle alone -- oracle vs float64 there: means3D tensor-wide 3.9e-2 (scalar radii) and
    # 1.4e-2 (per-axis), past the sweep's 1e-2; rows on the fp32 term 15.8 / 61.7 / 65.0 / 11.7 % and 5.8 / 35.0 / 30.0 / 4.2 % --
    # so its rows are printed, and the rows that are judged are those of test_backward_small's input (seeds 11 / 12), which
    # tests/test_grad_rows_judge.py pins on the CPU: at most 2.5 % of its rows on the fp32 term.
    for seed, gseed, judged in ((47, 48, False), (11, 12, True)):
        sj = make_splat_inputs(config, seed=seed, P=P, H=H, W=W, D=D)
        pi, mi, radii, cov6 = prep(sj, per_axis)
        g, gb, gd = _rand_grads(sj, gseed)
        if judged:
            _, rgrads, _ = reflib.splat_forward_backward(*_args(sj, pi, mi, radii, cov6), g, gb, gd)
            _, t, state, fwd_t = hip_splat_forward(gpu, sj, pi, mi, radii, cov6)
            grads = hip_splat_backward(gpu, sj, t, state, fwd_t, g, gb, gd)
        ograds = oracle.splat_backward(*_args(sj, pi, mi, radii, cov6), g, fwd=oracle.splat_forward(*_args(sj, pi, mi, radii, cov6)),
                                       bin_grad=gb, density_grad=gd)
        print()
        for name, a, b, o, tr in zip(GRAD_NAMES, grads, rgrads, ograds, splat_truth_grads(sj, pi, mi, radii, cov6, g, gb, gd)):
            for who, x in (("HIP", a), ("reference", b)):
                what = f"{who} {name} vs float64 (seed {seed}, per_axis={per_axis})"
                if judged:
                    assert_prob_grad_rows_close(x, tr, o, what=what)
                elif np.isfinite(o).all():
                    e = prob_row_errors(x, tr, o, GRAD_RTOL)
                    print(f"  {what:40s} NOT JUDGED: worst row {e['row']}: err / bound {e['ratio']:.3f} ({e['term']}), rows on the "
                          f"fp32 term {e['fp32_rows']} ({e['fp32_share']:.3f})")


def test_hip_arbitrary_points_vs_reference(gpu, reflib):
    """Random query points, at most one per voxel (with several per voxel the reference's voxel2pts scatter is a
    race, backward.cu:18-19; here the choice is pinned to the highest index, tested elsewhere)."""
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=49, P=200, H=20, W=24, D=16)
    keep = np.sort(np.random.default_rng(50).permutation(si.pts.shape[0])[:3000])
    jitter = (np.random.default_rng(51).random((len(keep), 3)).astype(np.float32) - 0.5) * np.float32(0.4)
    si.pts = np.ascontiguousarray(si.pts[keep] + jitter)
    rf, rgrads, grads, _ = _hip_vs_ref(gpu, reflib, si, False, 52)
    for name, a, b in zip(GRAD_NAMES, grads, rgrads):
        assert_grad_close(a, b, what=f"HIP {name} vs reference")
    _rows_vs_ref(si, False, grads, rgrads, "arbitrary points")


def test_hip_edge_cases_vs_reference(gpu, reflib):
    # only the whole-grid "empty" Gaussian (gaussian_head.py:90-102)
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=53, P=0, H=12, W=12, D=8)
    rf, rgrads, grads, _ = _hip_vs_ref(gpu, reflib, si, False, 54)
    for name, a, b in zip(GRAD_NAMES, grads, rgrads):
        assert_grad_close(a, b, what=f"HIP {name} vs reference (empty Gaussian only)")
    _rows_vs_ref(si, False, grads, rgrads, "empty Gaussian only")
    # centres outside the grid: the wrapper asserts (local_aggregate/__init__.py:140); the kernels clip like getRect
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=55, P=100, H=16, W=16, D=8)
    si.means3D[:50] += np.float32(3.0)
    rf, rgrads, grads, _ = _hip_vs_ref(gpu, reflib, si, False, 56)
    for name, a, b in zip(GRAD_NAMES, grads, rgrads):
        assert_grad_close(a, b, what=f"HIP {name} vs reference (outside centres)")
    _rows_vs_ref(si, False, grads, rgrads, "outside centres")
    # membership: Sigma^-1 = 0, opacity = semantics = 1 -> logits are integer Gaussian counts, bit-exact
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=57, P=2000, H=40, W=36, D=16)
    pi, mi, radii, cov6 = prep(si)
    si.opacities[:] = 1.0
    si.semantics[:] = 1.0
    cov6 = np.zeros_like(cov6)
    r = reflib.splat_forward(*_args(si, pi, mi, radii, cov6))
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    assert np.array_equal(got["logits"], r["logits"])


@pytest.mark.parametrize("config", ["nuscenes_gs25600_solid", "nuscenes_gs144000"])
def test_hip_full_size_vs_reference(gpu, reflib, config):
    """BASELINE.json configs [1]-[3] at full size: 200x200x16, P = 25 601 (with the empty Gaussian) / 144 000."""
    import torch
    from gaussianformer_amd.local_aggregate import splat_box_volumes
    si = make_splat_inputs(config, seed=0)
    rf, rgrads, grads, stats = _hip_vs_ref(gpu, reflib, si, False, 1)
    print(f"\n[{config}] HIP vs reference: max scaled logits err {stats['logits']:.3e}")
    pi, mi, radii, cov6 = prep(si)
    # north_star's bounds, literally: ABSOLUTE 1e-4 on the logits; gradients row by row -- every Gaussian against its
    # own magnitude (floor: the median ordinary row), the whole-grid "empty" Gaussian judged by itself
    got, t, state, fwd_t = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    a = assert_logits_abs(got["logits"], rf["logits"], what=f"HIP logits vs reference [{config}]")
    print(f"[{config}] max ABSOLUTE logits err {a:.3e} (max|logit| {np.abs(rf['logits']).max():.3e})")
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    assert int(whole.sum()) == (1 if config == "nuscenes_gs25600_solid" else 0)
    for name, a, b in zip(GRAD_NAMES, grads, rgrads):
        e = assert_grad_rows_close(a, b, whole, what=f"HIP {name} vs reference [{config}]")
        print(f"[{config}] {name}: worst ordinary row {e['ordinary']:.3e} (floor {e['floor']:.3e}, absolute {e['abs']:.3e}), "
              f"whole-grid row {e['whole_grid']:.3e}, tensor-wide {e['tensor']:.3e}")
    vols, R = splat_box_volumes(torch.from_numpy(mi).to(gpu), torch.from_numpy(radii).to(gpu), si.H, si.W, si.D)
    assert R == rf["num_rendered"]
    # the restatement at full size, so the full-size oracle comparisons elsewhere are pinned too
    of = oracle.splat_forward(*_args(si, pi, mi, radii, cov6))
    assert_logits_close(of["logits"], rf["logits"], what="oracle logits vs reference (full size)", tol=5e-6)


@pytest.mark.parametrize("per_axis", [False, True])
def test_hip_prob_full_size_vs_reference(gpu, reflib, per_axis):
    """BASELINE.json config [0] shape (Prob-64: P = 6 400, scales 0.01-3.2 m, radii up to 26, R ~ 1.7e8 pairs),
    localagg_prob and localagg_prob_fast, forward and backward."""
    si = make_splat_inputs("prob_gs6400", seed=0)
    pi, mi, radii, cov6 = prep(si, per_axis)
    g, gb, gd = _rand_grads(si, 2)
    rf, rgrads, _ = reflib.splat_forward_backward(*_args(si, pi, mi, radii, cov6), g, gb, gd)
    got, t, state, fwd_t = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    finite = np.isfinite(rf["logits"]).all(axis=1) & np.isfinite(rf["probability"])
    # the reference itself is NaN where det(Sigma^-1) rounds negative in fp32 (forward.cu:77-78); those voxels
    # have no defined result
    print(f"\n[prob per_axis={per_axis}] R = {rf['num_rendered']}, reference non-finite voxels: {(~finite).sum()}")
    for k in ("logits", "bin_logits", "density", "probability"):
        a, b = got[k][finite], rf[k][finite]
        err = np.abs(a.astype(np.float64) - b) / np.maximum(1.0, np.abs(b))
        print(f"   {k}: max scaled err {err.max():.3e}")
        assert err.max() <= 1e-4, (k, err.max())
        # Where the reference is not finite the HIP path is not finite either, element for element: the default
        # reproduces the reference's fp32 determinant (gf_common.hpp: prob_det32), NaN of a negative rounding included;
        # GF_PROB_EXACT_DET is the flag that removes them (tested below).
        fin_ref = np.isfinite(rf[k])
        assert np.array_equal(np.isfinite(got[k]), fin_ref), (k, int((np.isfinite(got[k]) != fin_ref).sum()))
    grads = hip_splat_backward(gpu, si, t, state, fwd_t, g, gb, gd)
    for name, a, b in zip(GRAD_NAMES, grads, rgrads):
        ok = np.isfinite(b)
        if ok.ndim > 1:
            ok = ok.all(axis=1)
        scale = max(np.abs(b[ok]).max(), 1e-6)
        err = np.abs(a[ok].astype(np.float64) - b[ok]).max() / scale
        print(f"   {name}: max err / max|ref| {err:.3e} ({(~ok).sum()} non-finite reference rows)")
        er = grad_row_errors(a[ok], b[ok])    # reported, not asserted: the reference's own fp32 quadratic form cancels
        print(f"   {name}: row by row: worst {er['ordinary']:.3e} (floor {er['floor']:.3e}, absolute {er['abs']:.3e})")
        assert np.isfinite(a[ok]).all() and err <= 1e-3, (name, err)
    if not per_axis:
        # the fp64 determinant (GF_PROB_EXACT_DET) leaves no non-finite voxel and agrees with the reference wherever
        # the reference is finite and its own determinant is not dominated by cancellation noise (loose bound)
        from gaussianformer_amd import _lib
        exact, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PROB_EXACT_DET)
        for k in ("logits", "bin_logits", "density", "probability"):
            assert np.isfinite(exact[k]).all(), k
        for k in ("bin_logits", "density"):     # independent of the determinant
            e = np.abs(exact[k][finite].astype(np.float64) - rf[k][finite]) / np.maximum(1.0, np.abs(rf[k][finite]))
            assert e.max() <= 1e-4, (k, e.max())


# ------------------------------------------------------------------------------------------------
# deformable aggregation
# ------------------------------------------------------------------------------------------------

def _daf_hip(gpu, d, g=None):
    import torch
    from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF
    feat, ss, st, loc, w = to_dev(gpu, d["mc_ms_feat"], d["spatial_shape"], d["scale_start_index"],
                                  d["sampling_location"], d["weights"])
    if g is None:
        return DAF.apply(feat, ss, st, loc, w).cpu().numpy(), None
    feat.requires_grad_(True); loc.requires_grad_(True); w.requires_grad_(True)
    out = DAF.apply(feat, ss, st, loc, w)
    out.backward(torch.from_numpy(g).to(gpu))
    return out.detach().cpu().numpy(), (feat.grad.cpu().numpy(), loc.grad.cpu().numpy(), w.grad.cpu().numpy())


def test_daf_hip_vs_reference_gs25600(gpu, reflib):
    """The full 230 400 sample points of nuscenes_gs25600_solid on the nuScenes pyramid, forward and backward."""
    d = make_daf_inputs(num_pts=230400, seed=61)
    want = reflib.daf_forward(**d)
    g = np.random.default_rng(62).standard_normal(want.shape).astype(np.float32)
    out, grads = _daf_hip(gpu, d, g)
    assert_logits_close(out, want, what="HIP daf output vs reference")
    gr = reflib.daf_backward(d["mc_ms_feat"], d["spatial_shape"], d["scale_start_index"], d["sampling_location"], d["weights"], g)
    for name, a, b in zip(("grad_mc_ms_feat", "grad_sampling_location", "grad_weights"), grads, gr):
        assert_grad_close(a, b, what=f"HIP {name} vs reference")


def test_daf_hip_vs_reference_gs144000(gpu, reflib):
    """1 296 000 sample points (nuscenes_gs144000), forward and backward."""
    d = make_daf_inputs(num_pts=1296000, seed=63)
    want = reflib.daf_forward(**d)
    g = np.random.default_rng(64).standard_normal(want.shape).astype(np.float32)
    out, grads = _daf_hip(gpu, d, g)
    assert_logits_close(out, want, what="HIP daf output vs reference (gs144000)")
    gr = reflib.daf_backward(d["mc_ms_feat"], d["spatial_shape"], d["scale_start_index"], d["sampling_location"], d["weights"], g)
    for name, a, b in zip(("grad_mc_ms_feat", "grad_sampling_location", "grad_weights"), grads, gr):
        assert_grad_close(a, b, what=f"HIP {name} vs reference (gs144000)")


def test_daf_hip_small_vs_reference(gpu, reflib):
    for i, case in enumerate([
        dict(num_pts=777, B=1, cams=6, C=128, G=4, levels=((27, 50), (14, 25), (7, 13), (4, 7))),
        dict(num_pts=300, B=2, cams=3, C=32, G=4, levels=((6, 9), (3, 5))),
        dict(num_pts=200, B=1, cams=2, C=24, G=4, levels=((5, 4),)),
        dict(num_pts=300, B=1, cams=3, C=256, G=8, levels=((6, 9), (3, 5))),
    ]):
        d = make_daf_inputs(seed=70 + i, **case)
        loc = d["sampling_location"]
        loc[0, 0, 0] = [0.0, 0.5]
        loc[0, 1, 0] = [0.999, 0.001]
        loc[0, 2, 0] = [1.0, 1.0]
        loc[0, 3, 0] = [1e-4, 0.9999]
        want = reflib.daf_forward(**d)
        g = np.random.default_rng(80 + i).standard_normal(want.shape).astype(np.float32)
        out, grads = _daf_hip(gpu, d, g)
        assert_logits_close(out, want, what=f"HIP daf output vs reference (case {i})")
        gr = reflib.daf_backward(d["mc_ms_feat"], d["spatial_shape"], d["scale_start_index"], d["sampling_location"], d["weights"], g)
        for name, a, b in zip(("grad_mc_ms_feat", "grad_sampling_location", "grad_weights"), grads, gr):
            assert_grad_close(a, b, what=f"HIP {name} vs reference (case {i})")
