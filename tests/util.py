"""Shared helpers for the parity tests: run the same seeded inputs through the CPU oracle
and through the HIP path (via the C ABI), and compare with the tolerances of SURVEY.md §8c /
north_star: integer path bit-exact; fp32 logits within 1e-4 -- ``assert_logits_close`` bounds the
scaled error |err| / max(1, |ref|), ``assert_logits_abs`` the ABSOLUTE error (what north_star says;
used at the BASELINE shapes against oracle/_ref); gradients <= 1e-3 -- ``assert_grad_close``
relative to the tensor's largest magnitude (small shapes), ``assert_grad_rows_close`` ROW BY ROW
(every Gaussian against its own magnitude, with a floor taken from the ordinary rows and the
whole-grid "empty" Gaussian, gaussian_head.py:90-102, judged separately: at nuscenes_gs25600_solid
its row is 1e4 times an ordinary one and would make a tensor-wide scale vacuous).

The small-shape tests (the kernels' layout edges) judge ROW BY ROW as well, next to their tensor-wide lines: with the whole-grid
Gaussian present the tensor-wide 1e-3 let EVERY ordinary Gaussian's cov3D_grad row be zero (tests/test_grad_rows_judge.py pins
that on the CPU, and pins the oracle to float64 autograd row by row: worst ordinary row 6.7e-6, worst whole-grid row 6.5e-5).
Row by row a zeroed row passes only if its magnitude is below 1e-3 of the median row's.  Measured on an MI355X over every touched
small-shape test (profiles/parity_rows_small.txt): worst ordinary row 7.3e-5, worst whole-grid row 9.0e-5, bound 1e-3.

The prob variant's fp32 quadratic form cancels (terms ~1e3 to a result ~1e0), in the oracle as in every fp32 evaluation: on the
``SMALL`` prob inputs the oracle's own worst row is 6.4e-3 from the truth.  Its rows are therefore judged against float64 autograd of
oracle/dense_ref.splat_dense (``splat_truth_grads``) by ``assert_prob_grad_rows_close``: row r within max(1e-3 * max(|truth_r|,
median row), 4 * the oracle's own error on r), and at most 5 % of the rows on the second term -- a share computed from the oracle
and the truth alone, so an input on which fp32 breaks down fails the test instead of excusing the kernel (measured: at most 2.5 %
of the rows, HIP error / bound at most 0.251)."""
import numpy as np

import oracle
from gaussianformer_amd.synthetic import make_splat_inputs

LOGIT_TOL = 1e-4
GRAD_RTOL = 1e-3


def prep(si, per_axis=False):
    radii_min = 1 if si.variant == "prob" else None
    pi, mi, radii, cov6 = oracle.prepare_splat_inputs(si.pts, si.means3D, si.scales, si.cov3D, si.pc_min,
                                                      si.grid_size, si.scale_multiplier, per_axis=per_axis,
                                                      radii_min=radii_min)
    return pi, mi, radii, cov6


def assert_logits_close(got, ref, what="logits", tol=LOGIT_TOL):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() <= tol, f"{what}: max scaled err {err.max():.3e} > {tol} at {np.unravel_index(err.argmax(), err.shape)}"


def assert_grad_close(got, ref, what="grad", rtol=GRAD_RTOL):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    scale = max(np.abs(ref).max(), 1e-6)
    err = np.abs(got - ref).max() / scale
    assert err <= rtol, f"{what}: max err / max|ref| = {err:.3e} > {rtol}"


def assert_logits_abs(got, ref, what="logits", tol=LOGIT_TOL):
    """north_star: "fp32 logits within 1e-4" -- the absolute error, no scaling by |ref|."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = np.abs(got - ref)
    assert err.max() <= tol, (f"{what}: max ABSOLUTE err {err.max():.3e} > {tol} at "
                              f"{np.unravel_index(err.argmax(), err.shape)} (max|ref| {np.abs(ref).max():.3e})")
    return float(err.max())


def whole_grid_rows(mi, radii, H, W, D):
    """Mask of the Gaussians whose integer box (auxiliary.h:8-20) is the whole grid -- the appended "empty"
    Gaussian of gaussian_head.py:90-102 (scale [100, 100, 8] -> radius 600)."""
    mi = np.asarray(mi, dtype=np.int64)
    r3 = np.asarray(radii, dtype=np.int64)
    if r3.ndim == 1:
        r3 = np.repeat(r3[:, None], 3, axis=1)
    dims = np.array([H, W, D], dtype=np.int64)
    lo = np.minimum(dims, np.maximum(0, mi - r3))
    hi = np.minimum(dims, np.maximum(0, mi + r3 + 1))
    return (lo == 0).all(axis=1) & (hi == dims).all(axis=1)


def grad_row_errors(got, ref, whole=None):
    """Per-row gradient errors.  Returns a dict: ``ordinary`` = max over the ordinary rows g of
    |err_g| / max(max|ref_g|, floor) with floor = the MEDIAN of the ordinary rows' max|ref_g| (so that a row whose
    terms cancel is held to the typical row's magnitude, not to zero, and never to the whole-grid row's);
    ``whole_grid`` = the same for the whole-grid rows against their own magnitude; ``floor``; ``abs`` = the largest
    absolute error of an ordinary row; ``tensor`` = the old tensor-wide figure max|err| / max|ref|."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    P = ref.shape[0]
    g2, r2 = got.reshape(P, -1), ref.reshape(P, -1)
    whole = np.zeros(P, bool) if whole is None else np.asarray(whole, bool)
    rowerr = np.abs(g2 - r2).max(axis=1) if P else np.zeros(0)
    rowmax = np.abs(r2).max(axis=1) if P else np.zeros(0)
    out = {"ordinary": 0.0, "whole_grid": 0.0, "floor": 0.0, "abs": 0.0, "worst_row": -1,
           "tensor": float(rowerr.max() / max(rowmax.max(), 1e-30)) if P else 0.0}
    o = ~whole
    if o.any():
        floor = max(float(np.median(rowmax[o])), 1e-30)
        rel = rowerr[o] / np.maximum(rowmax[o], floor)
        out.update(ordinary=float(rel.max()), floor=floor, abs=float(rowerr[o].max()),
                   worst_row=int(np.flatnonzero(o)[rel.argmax()]))
    if whole.any():
        out["whole_grid"] = float((rowerr[whole] / np.maximum(rowmax[whole], 1e-30)).max())
    return out


def assert_grad_rows_close(got, ref, whole=None, what="grad", rtol=GRAD_RTOL):
    """Row-by-row gradient bound (see the module docstring); returns the error record."""
    assert np.asarray(got).shape == np.asarray(ref).shape, (what, np.asarray(got).shape, np.asarray(ref).shape)
    assert np.isfinite(np.asarray(got)).all(), f"{what}: non-finite values"
    e = grad_row_errors(got, ref, whole)
    assert e["ordinary"] <= rtol, (f"{what}: row {e['worst_row']}: err / max(|ref row|, floor {e['floor']:.3e}) = "
                                   f"{e['ordinary']:.3e} > {rtol} (absolute {e['abs']:.3e})")
    assert e["whole_grid"] <= rtol, f"{what}: whole-grid row: err / max|ref row| = {e['whole_grid']:.3e} > {rtol}"
    return e


def daf_row_errors(got, ref, ref32, row_dims, rtol, touched=None, exempt=None):
    """Row-by-row error record of a deformable-aggregation result against its float64 restatement ``ref``, with the float32 run of
    the same restatement ``ref32`` as the yardstick of plain float32 arithmetic (torch tensors, any device).  A row is one index of
    the first ``row_dims`` dimensions.  Row r is bounded by max(rtol * max(max|ref_r|, floor), 4 * max|ref32_r - ref_r|), floor =
    the median of max|ref_r| over the touched rows.  ``touched`` (bool, one per row; None = every row): the other rows must be
    exactly 0.  ``exempt`` (bool, one per row): touched rows the bound does not judge (the caller says why)."""
    import torch
    R = int(np.prod(ref.shape[:row_dims]))
    g2, r2, f2 = (t.reshape(R, -1).to(torch.float64) for t in (got, ref, ref32))
    err = (g2 - r2).abs().amax(dim=1)
    err32 = (f2 - r2).abs().amax(dim=1)
    rowmax = r2.abs().amax(dim=1)
    touched = torch.ones(R, dtype=torch.bool, device=r2.device) if touched is None else touched.reshape(R).to(r2.device)
    judged = touched if exempt is None else touched & ~exempt.reshape(R).to(r2.device)
    out = {"rows": R, "touched": int(touched.sum()), "exempt": int((touched & ~judged).sum()),
           "untouched_nonzero": int(((g2[~touched] != 0).any(dim=1)).sum()) if bool((~touched).any()) else 0,
           "tensor": float(err.max() / rowmax.max().clamp(min=1e-30)), "ratio": 0.0, "row": -1, "err": 0.0, "bound": 0.0,
           "rel": 0.0, "term": "-", "fp32_rel": 0.0}
    if bool(judged.any()):
        floor = float(rowmax[touched].median().clamp(min=1e-30))
        scale = rowmax.clamp(min=floor)
        tol_term, f32_term = rtol * scale, 4.0 * err32
        bound = torch.maximum(tol_term, f32_term)
        ratio = torch.where(judged, err / bound.clamp(min=1e-300), torch.zeros_like(err))
        i = int(ratio.argmax())
        out.update(floor=floor, ratio=float(ratio[i]), row=i, err=float(err[i]), bound=float(bound[i]),
                   rel=float((torch.where(judged, err / scale, torch.zeros_like(err))).max()),
                   fp32_rel=float((torch.where(judged, err32 / scale, torch.zeros_like(err))).max()),
                   term="fp32" if float(f32_term[i]) > float(tol_term[i]) else f"{rtol:g} x row")
    return out


def assert_daf_rows_close(got, ref, ref32, what, row_dims, rtol=GRAD_RTOL, touched=None, exempt=None):
    """:func:`daf_row_errors`, asserted and printed (worst row, its bound and the term that set it); returns the record."""
    assert tuple(got.shape) == tuple(ref.shape) == tuple(ref32.shape), (what, tuple(got.shape), tuple(ref.shape), tuple(ref32.shape))
    assert bool(got.isfinite().all()), f"{what}: non-finite values"
    e = daf_row_errors(got, ref, ref32, row_dims, rtol, touched, exempt)
    print(f"  {what:28s} rows {e['touched']:>9d}/{e['rows']:<9d} worst row {e['row']:>9d}: err {e['err']:.2e} <= bound "
          f"{e['bound']:.2e} ({e['term']}), ratio {e['ratio']:.3f} | max row err / max(|ref row|, floor) {e['rel']:.2e} "
          f"(fp32 restatement {e['fp32_rel']:.2e}) | tensor-wide {e['tensor']:.2e} | exempt {e['exempt']}")
    assert e["untouched_nonzero"] == 0, f"{what}: {e['untouched_nonzero']} rows no visible tap touches are not exactly 0"
    assert e["ratio"] <= 1.0, (f"{what}: row {e['row']}: err {e['err']:.3e} > bound {e['bound']:.3e} ({e['term']}) "
                               f"= max({rtol:g} x max(|ref row|, floor {e.get('floor', 0):.3e}), 4 x fp32 restatement's error)")
    return e


PROB_FP32_SHARE_CAP = 0.05


def prob_row_errors(got, truth, oracle32, rtol):
    """Row-by-row error record of a prob-variant splat gradient against its float64 truth (:func:`splat_truth_grads`), with the
    fp32 restatement ``oracle32`` (oracle.splat_backward on the same inputs) as the yardstick of plain float32 arithmetic -- the
    idiom of :func:`daf_row_errors` on numpy arrays, one row per Gaussian.  Row r is bounded by
    max(rtol * max(max|truth_r|, floor), 4 * max|oracle32_r - truth_r|), floor = the median of max|truth_r|.  A row on which the
    restatement itself is not finite has no bound (infinite) and counts as a row on the fp32 term.  ``fp32_share`` = the share
    of rows whose bound came from the fp32 term: it reads the restatement and the truth only, never ``got``."""
    got, truth, oracle32 = (np.asarray(a, dtype=np.float64) for a in (got, truth, oracle32))
    P = truth.shape[0]
    g2, t2, o2 = got.reshape(P, -1), truth.reshape(P, -1), oracle32.reshape(P, -1)
    out = {"rows": P, "ratio": 0.0, "row": -1, "err": 0.0, "bound": 0.0, "rel": 0.0, "term": "-", "fp32_rel": 0.0,
           "fp32_share": 0.0, "fp32_rows": 0, "floor": 0.0, "tensor": 0.0}
    if P == 0:
        return out
    rowmax = np.abs(t2).max(axis=1)
    defined = np.isfinite(o2).all(axis=1)
    err32 = np.where(defined, np.abs(np.where(np.isfinite(o2), o2, 0.0) - t2).max(axis=1), np.inf)
    floor = max(float(np.median(rowmax)), 1e-30)
    scale = np.maximum(rowmax, floor)
    tol_term, f32_term = rtol * scale, 4.0 * err32
    on_fp32 = f32_term > tol_term
    bound = np.maximum(tol_term, f32_term)
    with np.errstate(invalid="ignore"):
        err = np.where(defined, np.abs(g2 - t2).max(axis=1), 0.0)
    err = np.where(np.isnan(err), np.inf, err)           # a non-finite result on a row the restatement defines
    ratio = err / bound
    i = int(ratio.argmax())
    out.update(floor=floor, ratio=float(ratio[i]), row=i, err=float(err[i]), bound=float(bound[i]),
               rel=float((err / scale).max()), fp32_rel=float((err32[defined] / scale[defined]).max()) if defined.any() else 0.0,
               term="fp32" if on_fp32[i] else f"{rtol:g} x row", fp32_share=float(on_fp32.mean()), fp32_rows=int(on_fp32.sum()),
               tensor=float(err.max() / max(rowmax.max(), 1e-30)))
    return out


def assert_prob_grad_rows_close(got, truth, oracle32, what="grad", rtol=GRAD_RTOL, cap=PROB_FP32_SHARE_CAP):
    """:func:`prob_row_errors`, printed and asserted: every row within its bound, and at most ``cap`` of the rows on the fp32 term
    (so the fp32 term cannot quietly become the whole check).  Returns the record."""
    assert np.asarray(got).shape == np.asarray(truth).shape == np.asarray(oracle32).shape, \
        (what, np.asarray(got).shape, np.asarray(truth).shape, np.asarray(oracle32).shape)
    e = prob_row_errors(got, truth, oracle32, rtol)
    print(f"  {what:40s} rows {e['rows']:>5d} worst row {e['row']:>5d}: err {e['err']:.2e} <= bound {e['bound']:.2e} ({e['term']}), "
          f"ratio {e['ratio']:.3f} | max row err / max(|truth row|, floor) {e['rel']:.2e} (fp32 restatement {e['fp32_rel']:.2e}) | "
          f"rows on the fp32 term {e['fp32_rows']} ({e['fp32_share']:.3f}) | tensor-wide {e['tensor']:.2e}")
    assert e["fp32_share"] <= cap, (f"{what}: {e['fp32_rows']} of {e['rows']} rows ({e['fp32_share']:.3f}) are judged by the fp32 "
                                    f"restatement's own error, more than {cap:g}")
    assert e["ratio"] <= 1.0, (f"{what}: row {e['row']}: err {e['err']:.3e} > bound {e['bound']:.3e} ({e['term']}) "
                               f"= max({rtol:g} x max(|truth row|, floor {e['floor']:.3e}), 4 x fp32 restatement's error)")
    return e


def print_grad_rows(what, e):
    """One line of a row-by-row record of :func:`assert_grad_rows_close` (the figures of profiles/parity_rows_small.txt)."""
    print(f"  {what:40s} worst ordinary row {e['ordinary']:.2e} (row {e['worst_row']}, floor {e['floor']:.2e}, absolute "
          f"{e['abs']:.2e}) | whole-grid row {e['whole_grid']:.2e} | tensor-wide {e['tensor']:.2e}")


def splat_truth_grads(si, pi, mi, radii, cov6, g, gb=None, gd=None):
    """fp64 autograd gradients of the dense formulation oracle/dense_ref.splat_dense (small cases: O(N P) work).  With several
    points per voxel only the highest-index point of a voxel feeds the backward (voxel2pts)."""
    import torch
    from oracle import dense_ref
    t = lambda a, grad=False: torch.tensor(a, dtype=torch.float64, requires_grad=grad)
    key = (pi[:, 0].astype(np.int64) * si.W + pi[:, 1]) * si.D + pi[:, 2]
    last = {}
    for n, k in enumerate(key):
        last[int(k)] = n
    winner = np.zeros(len(key))
    winner[list(last.values())] = 1.0
    m, o, s, c = t(si.means3D, True), t(si.opacities, True), t(si.semantics, True), t(cov6, True)
    out = dense_ref.splat_dense(si.variant, t(si.pts), torch.tensor(pi), m, torch.tensor(mi), o, s, torch.tensor(radii), c,
                                si.H, si.W, si.D)
    w = t(winner)
    if si.variant == "prob":
        ((out[0] * t(g) * w[:, None]).sum() + (out[1] * t(gb) * w).sum() + (out[2] * t(gd) * w).sum()).backward()
    else:
        (out * t(g) * w[:, None]).sum().backward()
    return [x.grad.numpy() for x in (m, o, s, c)]


def to_dev(dev, *arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def hip_splat_forward(dev, si, pi, mi, radii, cov6, flags=0):
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import splat_forward
    variant = _lib.GF_SPLAT_PROB if si.variant == "prob" else _lib.GF_SPLAT_BASE
    t = to_dev(dev, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6)
    logits, bl, de, pr, state = splat_forward(variant, *t, si.H, si.W, si.D, flags=flags)
    out = {"logits": logits.cpu().numpy()}
    if bl is not None:
        out.update(bin_logits=bl.cpu().numpy(), density=de.cpu().numpy(), probability=pr.cpu().numpy())
    return out, t, state, (logits, bl, de, pr)


def hip_splat_backward(dev, si, t, state, fwd_t, out_grad, bin_grad=None, dens_grad=None, flags=0):
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import splat_backward
    variant = _lib.GF_SPLAT_PROB if si.variant == "prob" else _lib.GF_SPLAT_BASE
    g, bg, dg = to_dev(dev, out_grad, bin_grad, dens_grad)
    grads = splat_backward(variant, *t, si.H, si.W, si.D, g, fwd_outputs=fwd_t if variant else None,
                           bin_logits_grad=bg, density_grad=dg, state=state, flags=flags)
    return [x.cpu().numpy() for x in grads]
