"""The wave kernel computes what depends on the lane alone (where its pieces of a unit's output rows go) once per wave, and gives
units inside the grid a store path without bounds: the routes through it -- the default forward, the GF_PREPARE_BACKWARD
instantiation, the labels instantiation -- and the tile matrix-core kernel must still agree BIT FOR BIT, on grids whose units lie
inside (16 x 16 x 16), cross the edge in x and y (12 x 20 x 8) and end below the upper brick (8 x 8 x 4), with groups that are
full, partial and a single Gaussian long.  The exact-fp32 kernel bounds them all (1e-4 scaled, the matrix-core tests' tolerance)."""
import pytest

from splat_cases import all_routes_agree, covering_scene

pytestmark = pytest.mark.gpu

GRIDS = [(16, 16, 16), (12, 20, 8), (8, 8, 4)]
# Gaussians drawn (the config appends the whole-grid one: P + 1 in all).  Every box covers the whole grid, so every unit takes
# all of them: 2 = one group of two; 32 = exactly one full group; 34 = a full group and a partial one of two; 201 = six full
# groups and one of nine; 65 = the second bitmask word holds a single Gaussian (and the third group a single row).
COUNTS = [1, 31, 33, 200, 64]


@pytest.mark.parametrize("H,W,D", GRIDS)
@pytest.mark.parametrize("P", COUNTS)
def test_wave_routes_and_tile_kernel_agree_bit_for_bit(gpu, P, H, W, D):
    """The labels instantiation with the logits kept (the same bits, and their argmax) and without (labels only)."""
    si, prepped = covering_scene(P, H, W, D, seed=100 + P, rng_seed=7 * P + H)
    all_routes_agree(gpu, si, prepped, exact_tol=1e-4, labels_only=True)
