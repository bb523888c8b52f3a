"""The wave kernel fetches every record once per group: lane (n, h) of a group brings pieces 4 h .. 4 h + 3 of Gaussian n into four
planes of the wave's slot, and both half-lanes read what they need from what the two of them fetched (the tile kernel keeps its
six pieces per lane).  No value changes: everywhere the wave kernel equals the tile kernel (``splat.mfma_tile_kernel``) bit for
bit, and both are within the matrix-core tests' 1e-4 of the exact-fp32 kernel.

1. Piece -> channel mapping: every box covers the grid, all 18 semantic values of every Gaussian are distinct and sign-mixed and the
   opacities distinct, so a swapped piece, half-lane or Gaussian changes bits.  Default, GF_PREPARE_BACKWARD and labels routes, and
   the long-row instantiation at the smallest P the route gives it.
2. A launch with more units than the 2 048 resident waves (96 x 96 x 32), where later units take their supertile's list from its
   unit 0 and go straight to the records: two frames on one workspace, eagerly and under one captured graph.
3. The same shape with a crowded supertile whose list is never published, next to ordinary ones, so that one wave meets units
   that find a list and units that do not; also through GF_PREPARE_BACKWARD and the matrix-core backward."""
import numpy as np
import pytest

from gaussianformer_amd import _lib
from gaussianformer_amd.synthetic import make_splat_inputs

from splat_cases import (SHORT_ROW_P, WAVE, WAVE_LONG, all_routes_agree, alternate_frames, bwd, covering_scene, crowded_supertile_scene,
                         plans, plans_agree, render_kernel, same_bits, tensors, units)
from util import assert_grad_rows_close, hip_splat_forward, prep, whole_grid_rows

pytestmark = pytest.mark.gpu


# ---- 1. piece -> channel mapping ------------------------------------------------------------------------------------------------
def _check_mapping(gpu, P, H, W, D):
    """P drawn Gaussians (+ the whole-grid one) that cover the grid, with 18 distinct, sign-mixed semantic values and a distinct
    opacity each (splat_cases.covering_scene): every route agrees, and no channel carries another channel's values."""
    si, prepped = covering_scene(P, H, W, D, seed=300 + P % 1000, rng_seed=11 * P + H, distinct=True)
    wave = all_routes_agree(gpu, si, prepped, exact_tol=1e-4)
    # channels 8, 9 (written by both half-lanes) and 16, 17 (the record's last piece) are nobody else's values
    for c in (8, 9, 16, 17):
        for d in range(18):
            assert d == c or not np.array_equal(wave[:, c], wave[:, d]), (c, d)


@pytest.mark.parametrize("H,W,D", [(12, 20, 8), (16, 16, 16)])
@pytest.mark.parametrize("P", [1, 31, 33, 64])
def test_every_piece_reaches_its_channel(gpu, P, H, W, D):
    _check_mapping(gpu, P, H, W, D)


def test_every_piece_reaches_its_channel_with_long_rows(gpu):
    """The smallest P the route renders with the long-row instantiation (one Gaussian more than the longest short row holds), every
    box covering a 16 x 16 x 16 grid: every unit consumes all of them, in several passes of its list."""
    H = W = D = 16
    assert render_kernel(SHORT_ROW_P, (H, W, D)) == WAVE and render_kernel(SHORT_ROW_P + 1, (H, W, D)) == WAVE_LONG
    _check_mapping(gpu, SHORT_ROW_P, H, W, D)   # (+ the whole-grid Gaussian)


# ---- 2. and 3.: launches with more units than resident waves ------------------------------------------------------------------------
def test_units_that_take_their_list_across_frames_and_graph_replays(gpu):
    """96 x 96 x 32: 2 304 units on 2 048 waves, the last 256 claimed long after every unit 0 has published.  Units took lists; two
    frames alternate through one workspace, eagerly and under one captured graph replayed, and every result is the frame's own on
    a workspace of its own."""
    fa = make_splat_inputs("nuscenes_gs25600_solid", seed=61, P=3000, H=96, W=96, D=32)
    fb = make_splat_inputs("nuscenes_gs25600_solid", seed=62, P=3000, H=96, W=96, D=32)
    assert units((fa.H, fa.W, fa.D)) == 2304
    took = plans_agree(gpu, fa)
    print("units that took a list:", took, "of", 2304)
    assert took > 0
    want = [plans(gpu, f)[1].run().cpu().numpy() for f in (fa, fb)]
    assert not np.array_equal(want[0], want[1])
    t, plan, _, _ = plans(gpu, fa)
    frames = ([x.clone() for x in t], tensors(gpu, fb))
    alternate_frames(plan, t, frames, want, eager_order=(0, 1), replay_order=(1, 0))


def test_units_next_to_a_list_that_is_not_published(gpu):
    """splat_cases.crowded_supertile_scene: the waves that claim the crowded supertile's units build their own lists from
    1 500-candidate rows, and claim a unit of a far supertile, whose list they take, before or after (the claims of an XCD go
    supertile by supertile)."""
    si, claimed, may_take = crowded_supertile_scene(seed=63, rng_seed=64)
    took = plans_agree(gpu, si)
    print("units that took a list:", took, "of", claimed, "claimed units;", may_take, "of them in supertiles whose list is published")
    assert 0 < took <= may_take

    # the same launch as GF_PREPARE_BACKWARD, then the matrix-core backward on what it left, against the exact backward
    pi, mi, radii, cov6 = prep(si)
    g = np.random.default_rng(65).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    prepared, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PREPARE_BACKWARD)
    words = _lib.SplatState.of(state)
    assert words.path == _lib.GF_PATH_MATRIX_CORE_WAVE and words.rows_ready, words
    got = bwd(gpu, si, t, state, g, flags=_lib.GF_MFMA_SPLAT | _lib.GF_RECORDS_VALID)
    plain, t0, state0, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    same_bits(prepared["logits"], plain["logits"], "GF_PREPARE_BACKWARD vs default")
    exact = bwd(gpu, si, t0, state0, g, flags=_lib.GF_EXACT_FP32)
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    for a, c, what in zip(got, exact, ("means", "opacity", "semantics", "cov")):
        assert_grad_rows_close(a, c.reshape(a.shape), whole, what=what)
