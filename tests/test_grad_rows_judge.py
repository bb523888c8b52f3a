"""The row-by-row gradient judgement itself, on the CPU: (1) it rejects what the tensor-wide bound lets through -- mutants of the
oracle's gradients at the base ``SMALL`` shapes of test_splat_gpu.py (a covariance gradient lost on every ordinary Gaussian, one
Gaussian's row lost, scaled by 1 + 5e-3, two rows swapped); (2) the yardstick it is used with -- the fp32 restatement
oracle.splat_backward -- is pinned row by row to float64 autograd of oracle/dense_ref.splat_dense at all seven shapes, so a row
within 1e-3 of the restatement is within 1.1e-3 of the truth."""
import numpy as np
import pytest

import oracle
from gaussianformer_amd.synthetic import make_splat_inputs

from util import (GRAD_RTOL, assert_grad_close, assert_grad_rows_close, assert_prob_grad_rows_close, prep, print_grad_rows,
                  splat_truth_grads, whole_grid_rows)

# the shapes and seeds of test_splat_gpu.py::test_backward_small
SMALL = [
    ("nuscenes_gs25600_solid", 300, 24, 20, 16, False),
    ("nuscenes_gs25600_solid", 257, 23, 21, 16, False),
    ("nuscenes_gs25600_solid", 200, 20, 20, 10, False),
    ("nuscenes_gs25600_solid", 200, 20, 20, 40, False),
    ("nuscenes_gs144000", 1000, 40, 44, 16, False),
    ("prob_gs6400", 120, 24, 20, 16, False),
    ("prob_gs6400", 120, 24, 20, 16, True),
]
BASE = [c for c in SMALL if c[0] != "prob_gs6400"]
NAMES = ("means3D_grad", "opacity_grad", "semantics_grad", "cov3D_grad")
_cache = {}


def _case(case):
    """(oracle gradients, float64 truth, whole-grid mask) of one shape, computed once and never written to."""
    if case not in _cache:
        config, P, H, W, D, per_axis = case
        si = make_splat_inputs(config, seed=11, P=P, H=H, W=W, D=D)
        pi, mi, radii, cov6 = prep(si, per_axis)
        rng = np.random.default_rng(12)
        N = si.pts.shape[0]
        g = rng.standard_normal((N, 18)).astype(np.float32)
        gb = rng.standard_normal(N).astype(np.float32) if si.variant == "prob" else None
        gd = rng.standard_normal(N).astype(np.float32) if si.variant == "prob" else None
        fwd = oracle.splat_forward(si.variant, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, H, W, D)
        ref = oracle.splat_backward(si.variant, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, H, W, D, g,
                                    fwd=fwd, bin_grad=gb, density_grad=gd)
        ref = [np.asarray(r).reshape(si.means3D.shape[0], -1) for r in ref]
        truth = [t.reshape(r.shape) for t, r in zip(splat_truth_grads(si, pi, mi, radii, cov6, g, gb, gd), ref)]
        for a in ref + truth:
            a.setflags(write=False)
        _cache[case] = (ref, truth, whole_grid_rows(mi, radii, H, W, D))
    return _cache[case]


def _median_row(ref, whole):
    """The ordinary row whose magnitude is the median of the ordinary rows' (the lower one of an even count)."""
    rowmax = np.abs(ref).max(axis=1)
    o = np.flatnonzero(~whole)
    return int(o[np.argsort(rowmax[o], kind="stable")[(len(o) - 1) // 2]])


def _rejected(mut, ref, whole, what):
    with pytest.raises(AssertionError):
        assert_grad_rows_close(mut, ref, whole, what=what, rtol=GRAD_RTOL)


@pytest.mark.parametrize("case", BASE, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}x{c[4]}")
def test_row_judgement_rejects_what_the_tensor_wide_bound_accepts(case):
    ref, _, whole = _case(case)
    ordinary = np.flatnonzero(~whole)
    assert len(ordinary) >= 2
    for name, r in zip(NAMES, ref):
        assert_grad_rows_close(r, r, whole, what=name)                      # the unmutated gradient passes
    # (a) every ordinary Gaussian's covariance gradient lost
    cov = ref[3]
    mut = cov.copy()
    mut[ordinary] = 0.0
    _rejected(mut, cov, whole, "cov3D_grad, ordinary rows zeroed")
    if whole.any():      # pins the gap: next to a whole-grid row the tensor-wide 1e-3 does not see the ordinary rows at all
        assert_grad_close(mut, cov, what="cov3D_grad, ordinary rows zeroed (tensor-wide)", rtol=GRAD_RTOL)
    for name, r in zip(NAMES, ref):
        k = _median_row(r, whole)
        assert np.abs(r[k]).max() > 0.0
        # (b) the median row lost
        mut = r.copy()
        mut[k] = 0.0
        _rejected(mut, r, whole, f"{name}, row {k} zeroed")
        if whole.any() and name == "cov3D_grad":       # (the other tensors' median rows are visible tensor-wide too)
            assert_grad_close(mut, r, what=f"{name}, row {k} zeroed (tensor-wide)", rtol=GRAD_RTOL)
        # (c) the median row off by 5e-3 of itself
        mut = r.copy()
        mut[k] = r[k] * (1.0 + 5e-3)
        _rejected(mut, r, whole, f"{name}, row {k} scaled by 1 + 5e-3")
        # (d) the median row and the largest ordinary row swapped
        rowmax = np.abs(r).max(axis=1)
        j = int(ordinary[rowmax[ordinary].argmax()])
        assert j != k and np.abs(r[k] - r[j]).max() > 2 * GRAD_RTOL * rowmax[j]       # (two rows that do differ)
        mut = r.copy()
        mut[[k, j]] = r[[j, k]]
        _rejected(mut, r, whole, f"{name}, rows {k} and {j} swapped")


@pytest.mark.parametrize("case", SMALL, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}x{c[4]}{'-per_axis' if c[5] else ''}")
def test_oracle_rows_against_float64_truth(case):
    """Base: every row of the restatement within 1e-4 of the truth (a tenth of the GPU bound; measured: worst ordinary row
    6.7e-6, worst whole-grid row 6.5e-5, the opacity's).  Prob: the restatement's quadratic form cancels (worst row 6.4e-3), so it
    is the yardstick, not the truth -- what is pinned is that at most 5 % of the rows need it (measured: at most 2.5 %)."""
    ref, truth, whole = _case(case)
    print()
    for name, r, t in zip(NAMES, ref, truth):
        if case[0] == "prob_gs6400":
            assert_prob_grad_rows_close(r, t, r, what=f"oracle {name} vs float64")
        else:
            print_grad_rows(f"oracle {name} vs float64", assert_grad_rows_close(r, t, whole, what=name, rtol=1e-4))
