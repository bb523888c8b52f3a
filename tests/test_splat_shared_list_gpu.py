"""The short-row wave kernel shares a supertile's candidate list inside one launch: unit 0 of every supertile publishes the list it
built (ids and packed boxes, with the call's tag in the length word), and a later unit of the supertile that finds the tagged word
takes the list by LDS-DMA instead of scanning the bitmask row and fetching the boxes.  Nobody waits for anybody, so every result has
to be the same bits whether a unit found the list or not: against the tile kernel (bit for bit) and the exact-fp32 kernel (1e-4).

A unit can only find a list if it is claimed after its supertile's unit 0 has published, i.e. when the launch has more units
(H/4 * W/4 * ceil(D/8)) than the 2 048 resident waves.  The kernel counts the units that took a list in word 32 of each XCD's
forward-counter block of the flag section (kFwdCounters + 64 x + 32); the tests read that count."""
import numpy as np
import pytest
import torch

import oracle
from gaussianformer_amd.synthetic import make_splat_inputs

from util import assert_logits_close, hip_splat_backward, hip_splat_forward, prep, to_dev, whole_grid_rows

pytestmark = pytest.mark.gpu

K_FWD_COUNTERS = 4608   # gf_common.hpp: kFwdCounters, one 64-word block per XCD; word 0 = next unit, word 32 = units that took a list


def _took(plan):
    torch.cuda.synchronize()
    w = plan.workspace[:32768].view(torch.int32)
    return int(sum(int(w[K_FWD_COUNTERS + 64 * x + 32]) for x in range(8)))


def _tensors(gpu, si):
    pi, mi, radii, cov6 = prep(si)
    return to_dev(gpu, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6)


def _plans(gpu, si, extra=0):
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import SplatForwardPlan
    t = _tensors(gpu, si)
    wave = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=extra)
    tile = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=extra)
    exact = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=extra | _lib.GF_EXACT_FP32)
    return t, wave, tile, exact


def _three_way(gpu, si):
    """wave kernel == tile kernel bit for bit, both within 1e-4 of the exact-fp32 kernel; returns (wave plan, units that took a list)."""
    from gaussianformer_amd import _lib
    t, wave, tile, exact = _plans(gpu, si)
    before = _took(wave)
    got = wave.run().cpu().numpy()
    took = _took(wave) - before
    assert wave.state_words()[1] == _lib.GF_PATH_MATRIX_CORE_WAVE
    with _lib.option("splat.mfma_tile_kernel", 1):
        ref = tile.run().cpu().numpy()
    assert tile.state_words()[1] == _lib.GF_PATH_MATRIX_CORE
    assert np.isfinite(got).all()
    assert np.array_equal(got, ref)
    assert_logits_close(got, exact.run().cpu().numpy(), tol=1e-4)
    return wave, took


def _units(si):
    return -(-si.H // 8) * -(-si.W // 8) * 4 * -(-si.D // 8)


def test_smallest_consuming_shape(gpu):
    """96 x 96 x 32: 144 supertiles x 16 units = 2 304 units on 2 048 waves -- the last 256 units are claimed by waves that have
    finished a unit, long after every unit 0 has published."""
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=51, P=3000, H=96, W=96, D=32)
    assert _units(si) == 2304
    _, took = _three_way(gpu, si)
    print("units that took a list:", took, "of", _units(si))
    assert took > 0


@pytest.mark.parametrize("shape", [(100, 92, 64), (40, 36, 16)])
def test_grid_edges_and_a_grid_of_one_round(gpu, shape):
    """100 x 92 x 64: the last supertile row and column are partly outside the grid (their quarters 1 and 3 do not exist), 13 x 12
    supertiles x 32 units = 4 992 > 2 048.  40 x 36 x 16: 200 units on as many waves, one round: only a wave whose first index
    lies outside the grid claims a second one (a handful may find a list, most find none), same bits."""
    H, W, D = shape
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=52, P=2500, H=H, W=W, D=D)
    _, took = _three_way(gpu, si)
    print("units that took a list:", took, "of", _units(si))
    if _units(si) > 2048:
        assert took > 0
    else:
        assert took < _units(si) // 8


def test_a_list_that_is_not_published(gpu):
    """A crowded supertile whose later units all LOOK for the list and do not find one.  96 x 96 x 32: 18 supertiles per XCD, 16
    units each; an XCD's indices are its 18 units 0, then 15 units per supertile, supertile by supertile; the first 256 indices are
    the waves' static first units (they never look), the other 32 are claimed later -- 256 units in all.  Supertile (10, 8), cells
    80..87 x 64..71, is s = 128: XCD 0, q = 16, its units 1..15 are indices 258..272, all claimed.  Fifteen hundred small Gaussians
    inside it: the list is longer than kBwdList = 256, unit 0 leaves the length word cleared, the fifteen read the cleared word
    and build their own lists.  (The boxes reach into the eight neighbouring supertiles, ~670 candidates each: their lists stay
    unpublished too, and five of them -- s = 127, 129, 139, 140, 141 -- have claimed units as well.)  So at most 256 - 15 units
    take a list -- the test counts, on the CPU, the claimed units of the supertiles whose list is short enough: no more than those
    may --, those of the far supertiles do, and the bits are the tile kernel's: a truncated list under a tagged word, or a reader
    that accepted such a word, would show in the crowded supertile's voxels."""
    H = W = 96
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=53, P=3000, H=H, W=W, D=32)
    nsy, per_super, srow, scol = W // 8, 16, 10, 8
    s = srow * nsy + scol
    nsuper_xcd = (H // 8) * nsy // 8
    first = nsuper_xcd + (s // 8) * (per_super - 1)             # XCD-local index of the supertile's unit 1
    claimed = _units(si) - 2048
    assert s % 8 == 0 and first >= 2048 // 8 and first + per_super - 1 <= _units(si) // 8 and claimed == 256
    rng = np.random.default_rng(54)
    lo = np.asarray(si.pc_min, dtype=np.float64)
    si.means3D[:1500, 0] = (lo[0] + (8 * srow + 8 * rng.random(1500)) * si.grid_size).astype(np.float32)
    si.means3D[:1500, 1] = (lo[1] + (8 * scol + 8 * rng.random(1500)) * si.grid_size).astype(np.float32)
    # the claimed units whose supertile's list is short enough to be published (boxes as auxiliary.h:8-20 clips them)
    pi, mi, radii, cov6 = prep(si)
    mi, r3 = np.asarray(mi, dtype=np.int64), np.asarray(radii, dtype=np.int64).reshape(len(mi), -1)
    blo, bhi = np.maximum(0, mi[:, :2] - r3[:, :1]), np.minimum([H, W], mi[:, :2] + r3[:, :1] + 1)
    may_take = 0
    for t in range((H // 8) * nsy):
        x0, y0 = 8 * (t // nsy), 8 * (t % nsy)
        ncand = int(((blo[:, 0] < x0 + 8) & (bhi[:, 0] > x0) & (blo[:, 1] < y0 + 8) & (bhi[:, 1] > y0)).sum())
        f = nsuper_xcd + (t // 8) * (per_super - 1)
        nclaimed = sum(1 for u in range(f, f + per_super - 1) if u >= 2048 // 8)
        if t == s:
            assert ncand > 256 and nclaimed == per_super - 1
        may_take += nclaimed if ncand <= 256 else 0
    assert 0 < may_take <= claimed - (per_super - 1)
    _, took = _three_way(gpu, si)
    print("units that took a list:", took, "of", claimed, "claimed units;", may_take, "of them in supertiles whose list is published")
    assert 0 < took <= may_take


def test_two_frames_on_one_workspace_eager_and_replayed(gpu):
    """Frames A and B alternate through ONE plan (one workspace, the lists of the previous call still in it): every result equals
    the frame's result on a workspace of its own, so a list of another call is never taken -- the records pass clears the length
    words and the tag follows the device-side call counter.  The same under a replayed HIP graph, where the host sees no call."""
    fa = make_splat_inputs("nuscenes_gs25600_solid", seed=55, P=3000, H=96, W=96, D=32)
    fb = make_splat_inputs("nuscenes_gs25600_solid", seed=56, P=3000, H=96, W=96, D=32)
    want = []
    for f in (fa, fb):
        _, fresh, _, _ = _plans(gpu, f)
        want.append(fresh.run().cpu().numpy())
    assert not np.array_equal(want[0], want[1])
    t, plan, _, _ = _plans(gpu, fa)
    ta, tb = [x.clone() for x in t], _tensors(gpu, fb)

    def load(src):
        for dst, s in zip(t, src):
            dst.copy_(s)

    before = _took(plan)
    for k in (0, 1, 1, 0, 1):
        load((ta, tb)[k])
        assert np.array_equal(plan.run().cpu().numpy(), want[k]), k
    assert _took(plan) > before
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.run(); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.run(stream=s.cuda_stream)
    before = _took(plan)
    for k in (1, 0, 0, 1):
        load((ta, tb)[k])
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(plan.logits.cpu().numpy(), want[k]), k
    assert _took(plan) > before


def test_prepared_forward_then_backward(gpu):
    """GF_PREPARE_BACKWARD on a launch with more units than waves (96 x 96 x 32: 2 304, so units took lists -- counted on this
    shape by test_smallest_consuming_shape; the shared stream workspace of this call path is not the test's to read): the lists
    the backward takes now carry the call's tag in the upper half of their length words.  Gradients equal, bit for bit, those
    behind an unprepared forward (the backward then scans the rows itself), and the oracle's within the suite's bound."""
    from gaussianformer_amd import _lib
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
