"""The wave kernel computes what depends on the lane alone (where its pieces of a unit's output rows go) once per wave, and gives
units inside the grid a store path without bounds: the routes through it -- the default forward, the GF_PREPARE_BACKWARD
instantiation, the labels instantiation -- and the tile matrix-core kernel must still agree BIT FOR BIT, on grids whose units lie
inside (16 x 16 x 16), cross the edge in x and y (12 x 20 x 8) and end below the upper brick (8 x 8 x 4), with groups that are
full, partial and a single Gaussian long.  The exact-fp32 kernel bounds them all (1e-4 scaled, the matrix-core tests' tolerance)."""
import numpy as np
import pytest
import torch

from gaussianformer_amd.synthetic import cov_inverse, make_splat_inputs

from util import assert_logits_close, prep, to_dev

pytestmark = pytest.mark.gpu

GRIDS = [(16, 16, 16), (12, 20, 8), (8, 8, 4)]
# Gaussians drawn (the config appends the whole-grid one: P + 1 in all).  Every box covers the whole grid, so every unit takes
# all of them: 2 = one group of two; 32 = exactly one full group; 34 = a full group and a partial one of two; 201 = six full
# groups and one of nine; 65 = the second bitmask word holds a single Gaussian (and the third group a single row).
COUNTS = [1, 31, 33, 200, 64]


def _inputs(P, H, W, D):
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=100 + P, P=P, H=H, W=W, D=D)
    rng = np.random.default_rng(7 * P + H)
    # scales of 3..5 m (6..10 voxels; the box reaches scale_multiplier times that): every Gaussian covers the grid, so a unit has
    # P + 1 hits; the covariances are those of the new scales, which keeps the exponents far inside the matrix-core range
    si.scales[:P] = (3.0 + 2.0 * rng.random((P, 3))).astype(np.float32)
    si.cov3D[:P] = cov_inverse(si.scales[:P], rng.standard_normal((P, 4))).astype(np.float32)
    si.semantics[-1, 2] = -0.5       # a negative semantic value (the whole-grid Gaussian: seen by every voxel)
    si.semantics[0, 5] = -1.25
    if P > 1:
        si.opacities[1] = 0.0         # a Gaussian that contributes nothing
    return si


@pytest.mark.parametrize("H,W,D", GRIDS)
@pytest.mark.parametrize("P", COUNTS)
def test_wave_routes_and_tile_kernel_agree_bit_for_bit(gpu, P, H, W, D):
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import splat_forward, splat_forward_labels
    si = _inputs(P, H, W, D)
    pi, mi, radii, cov6 = prep(si)
    assert (np.asarray(radii).reshape(P + 1, -1).min(axis=1) >= max(H, W, D)).all(), "every box covers the grid"
    t = to_dev(gpu, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6)
    V = _lib.GF_SPLAT_BASE

    def run(flags):
        logits, _, _, _, state = splat_forward(V, *t, H, W, D, flags=flags)
        return logits.cpu().numpy(), _lib.SplatState.of(state)

    wave, wstate = run(0)
    assert (wstate.not_dense, wstate.path, wstate.verdict) == (False, _lib.GF_PATH_MATRIX_CORE_WAVE, 0), wstate
    assert np.isfinite(wave).all()
    with _lib.option("splat.mfma_tile_kernel", 1):
        tile, tstate = run(_lib.GF_MFMA_SPLAT)
    assert tstate.path == _lib.GF_PATH_MATRIX_CORE, tstate
    prepared, pstate = run(_lib.GF_PREPARE_BACKWARD)
    assert pstate.path == _lib.GF_PATH_MATRIX_CORE_WAVE, pstate
    bits = lambda x: x.view(np.int32)
    assert np.array_equal(bits(wave), bits(tile)), "wave kernel vs tile kernel"
    assert np.array_equal(bits(wave), bits(prepared)), "default vs GF_PREPARE_BACKWARD"

    # the labels instantiation: with the logits kept (the same bits, and their argmax) and without (labels only)
    labels, kept = splat_forward_labels(V, *t, H, W, D, keep_logits=True)
    assert np.array_equal(bits(kept.cpu().numpy()), bits(wave)), "labels instantiation's logits"
    want = wave.argmax(axis=1)   # (the first of equal maxima, like the kernel)
    assert np.array_equal(labels.cpu().numpy(), want)
    only = splat_forward_labels(V, *t, H, W, D)
    assert np.array_equal(only.cpu().numpy(), want)

    exact, estate = run(_lib.GF_EXACT_FP32)
    assert estate.path not in (_lib.GF_PATH_MATRIX_CORE_WAVE, _lib.GF_PATH_MATRIX_CORE), estate
    assert_logits_close(wave, exact, tol=1e-4)
