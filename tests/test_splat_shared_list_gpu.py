"""The short-row wave kernel shares a supertile's candidate list inside one launch: unit 0 of every supertile publishes the list it
built (ids and packed boxes, with the call's tag in the length word), and a later unit of the supertile that finds the tagged word
takes the list by LDS-DMA instead of scanning the bitmask row and fetching the boxes.  Nobody waits for anybody, so every result has
to be the same bits whether a unit found the list or not: against the tile kernel (bit for bit) and the exact-fp32 kernel (1e-4).

A unit can only find a list if it is claimed after its supertile's unit 0 has published, i.e. when the launch has more units
(H/4 * W/4 * ceil(D/8)) than the 2 048 resident waves.  The kernel counts the units that took a list in word 32 of each XCD's
forward-counter block of the flag section (kFwdCounters + 64 x + 32); the tests read that count."""
import numpy as np
import pytest

import oracle
from gaussianformer_amd import _lib
from gaussianformer_amd.synthetic import make_splat_inputs

from splat_cases import RESIDENT_WAVES, alternate_frames, crowded_supertile_scene, plans, plans_agree, tensors, units
from util import hip_splat_backward, hip_splat_forward, prep, whole_grid_rows

pytestmark = pytest.mark.gpu


def test_smallest_consuming_shape(gpu):
    """96 x 96 x 32: 144 supertiles x 16 units = 2 304 units on 2 048 waves -- the last 256 units are claimed by waves that have
    finished a unit, long after every unit 0 has published."""
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=51, P=3000, H=96, W=96, D=32)
    assert units((si.H, si.W, si.D)) == 2304
    took = plans_agree(gpu, si)
    print("units that took a list:", took, "of", 2304)
    assert took > 0


@pytest.mark.parametrize("shape", [(100, 92, 64), (40, 36, 16)])
def test_grid_edges_and_a_grid_of_one_round(gpu, shape):
    """100 x 92 x 64: the last supertile row and column are partly outside the grid (their quarters 1 and 3 do not exist), 13 x 12
    supertiles x 32 units = 4 992 > 2 048.  40 x 36 x 16: 200 units on as many waves, one round: only a wave whose first index
    lies outside the grid claims a second one (a handful may find a list, most find none), same bits."""
    H, W, D = shape
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=52, P=2500, H=H, W=W, D=D)
    took = plans_agree(gpu, si)
    print("units that took a list:", took, "of", units(shape))
    if units(shape) > RESIDENT_WAVES:
        assert took > 0
    else:
        assert took < units(shape) // 8


def test_a_list_that_is_not_published(gpu):
    """A crowded supertile whose later units all LOOK for the list and do not find one (splat_cases.crowded_supertile_scene).  At
    most 256 - 15 units take a list -- the scene counts, on the CPU, the claimed units of the supertiles whose list is short enough:
    no more than those may --, those of the far supertiles do, and the bits are the tile kernel's: a truncated list under a tagged
    word, or a reader that accepted such a word, would show in the crowded supertile's voxels."""
    si, claimed, may_take = crowded_supertile_scene(seed=53, rng_seed=54)
    took = plans_agree(gpu, si)
    print("units that took a list:", took, "of", claimed, "claimed units;", may_take, "of them in supertiles whose list is published")
    assert 0 < took <= may_take


def test_two_frames_on_one_workspace_eager_and_replayed(gpu):
    """Frames A and B alternate through ONE plan (one workspace, the lists of the previous call still in it): every result equals
    the frame's result on a workspace of its own, so a list of another call is never taken -- the records pass clears the length
    words and the tag follows the device-side call counter.  The same under a replayed HIP graph, where the host sees no call."""
    fa = make_splat_inputs("nuscenes_gs25600_solid", seed=55, P=3000, H=96, W=96, D=32)
    fb = make_splat_inputs("nuscenes_gs25600_solid", seed=56, P=3000, H=96, W=96, D=32)
    want = [plans(gpu, f)[1].run().cpu().numpy() for f in (fa, fb)]
    assert not np.array_equal(want[0], want[1])
    t, plan, _, _ = plans(gpu, fa)
    frames = ([x.clone() for x in t], tensors(gpu, fb))
    alternate_frames(plan, t, frames, want, eager_order=(0, 1, 1, 0, 1), replay_order=(1, 0, 0, 1))


def test_prepared_forward_then_backward(gpu):
    """GF_PREPARE_BACKWARD on a launch with more units than waves (96 x 96 x 32: 2 304, so units took lists -- counted on this
    shape by test_smallest_consuming_shape; the shared stream workspace of this call path is not the test's to read): the lists
    the backward takes now carry the call's tag in the upper half of their length words.  Gradients equal, bit for bit, those
    behind an unprepared forward (the backward then scans the rows itself), and the oracle's within the suite's bound."""
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=57, P=2000, H=96, W=96, D=32)
    pi, mi, radii, cov6 = prep(si)
    g = np.random.default_rng(58).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    ref = oracle.splat_backward("base", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, si.H, si.W, si.D, g)
    outs = []
    for fflags in (0, _lib.GF_PREPARE_BACKWARD):
        fwd, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=fflags)
        words = _lib.SplatState.of(state)
        assert words.path == _lib.GF_PATH_MATRIX_CORE_WAVE and bool(words.rows_ready) == bool(fflags)
        outs.append((fwd["logits"], hip_splat_backward(gpu, si, t, state, None, g)))
    assert np.array_equal(outs[0][0], outs[1][0])
    # (the whole-grid Gaussian has more rows than the row buffer sums in one workgroup: its gradients are accumulated with atomics,
    # in an order that changes from run to run -- with the lists or without; every other row is the same bits)
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    assert whole.sum() == 1
    for a, b, c in zip(outs[1][1], outs[0][1], ref):
        print("whole-grid row equal:", np.array_equal(a[whole], b[whole]), "max difference", np.abs(a[whole] - b[whole]).max())
        assert np.isfinite(a).all() and np.array_equal(a[~whole], b[~whole])
        assert np.abs(a - c.reshape(a.shape)).max() <= 2e-4 * max(np.abs(c).max(), 1e-30)
