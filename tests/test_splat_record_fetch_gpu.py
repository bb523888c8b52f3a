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
import ctypes

import numpy as np
import pytest
import torch

from gaussianformer_amd.synthetic import cov_inverse, make_splat_inputs

from util import assert_grad_rows_close, assert_logits_close, hip_splat_backward, hip_splat_forward, prep, to_dev, whole_grid_rows

pytestmark = pytest.mark.gpu

K_FWD_COUNTERS = 4608   # gf_common.hpp: kFwdCounters, one 64-word block per XCD; word 32 = units that took a list
K_WROW = 618            # splat_fwd.hip: kWRow, the longest bitmask row (in words) the short-row instantiation holds in LDS
ROUTE_WAVE, ROUTE_WAVE_LONG = 3, 4   # word 0 of gf_debug_splat_route


def _bits(x):
    return x.view(np.int32)


def _took(plan):
    torch.cuda.synchronize()
    w = plan.workspace[:32768].view(torch.int32)
    return int(sum(int(w[K_FWD_COUNTERS + 64 * x + 32]) for x in range(8)))


def _route_kernel(P, H, W, D):
    from gaussianformer_amd import _lib
    fn = _lib.load().gf_debug_splat_route
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 8 + [ctypes.c_void_p, ctypes.c_int]
    out = (ctypes.c_int * 18)()
    assert fn(_lib.GF_SPLAT_BASE, _lib.GF_WORKSPACE_ZEROED, -1, P, H * W * D, H, W, D, out, 18) == 18
    return out[0]


# ---- 1. piece -> channel mapping ------------------------------------------------------------------------------------------------
def _covering_inputs(P, H, W, D):
    """P drawn Gaussians (the config appends the whole-grid one) whose boxes all cover the grid -- scales and covariances as in
    tests/test_splat_wave_invariants_gpu.py, which keeps the exponents inside the matrix-core range -- with 18 distinct, sign-mixed
    semantic values each and a distinct opacity each."""
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=300 + P % 1000, P=P, H=H, W=W, D=D)
    rng = np.random.default_rng(11 * P + H)
    si.scales[:P] = (3.0 + 2.0 * rng.random((P, 3))).astype(np.float32)
    si.cov3D[:P] = cov_inverse(si.scales[:P], rng.standard_normal((P, 4))).astype(np.float32)
    n = si.semantics.shape[0]
    # (both signs in every Gaussian, one sign per channel: a channel's sum over many Gaussians does not cancel, so the scaled 1e-4
    # against the exact kernel's own fp32 summation means the same at P = 1 and at long rows)
    sem = rng.uniform(0.25, 2.0, size=(n, 18)) * np.where(np.arange(18) % 2 == 1, -1.0, 1.0)
    si.semantics[:] = sem.astype(np.float32)
    si.opacities[:] = rng.permutation(np.linspace(0.05, 0.95, n)).astype(np.float32).reshape(si.opacities.shape)
    assert all(len(np.unique(row)) == 18 for row in si.semantics[:min(n, 128)])
    assert len(np.unique(si.opacities)) == n
    return si


def _check_mapping(gpu, si):
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import splat_forward, splat_forward_labels
    H, W, D = si.H, si.W, si.D
    pi, mi, radii, cov6 = prep(si)
    assert (np.asarray(radii).reshape(len(mi), -1).min(axis=1) >= max(H, W, D)).all(), "every box covers the grid"
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
    assert np.array_equal(_bits(wave), _bits(tile)), "wave kernel vs tile kernel"
    prepared, pstate = run(_lib.GF_PREPARE_BACKWARD)
    assert pstate.path == _lib.GF_PATH_MATRIX_CORE_WAVE, pstate
    assert np.array_equal(_bits(wave), _bits(prepared)), "default vs GF_PREPARE_BACKWARD"
    labels, kept = splat_forward_labels(V, *t, H, W, D, keep_logits=True)
    assert np.array_equal(_bits(kept.cpu().numpy()), _bits(wave)), "labels instantiation's logits"
    assert np.array_equal(labels.cpu().numpy(), wave.argmax(axis=1))
    exact, estate = run(_lib.GF_EXACT_FP32)
    assert estate.path not in (_lib.GF_PATH_MATRIX_CORE_WAVE, _lib.GF_PATH_MATRIX_CORE), estate
    assert_logits_close(wave, exact, tol=1e-4)
    # channels 8, 9 (written by both half-lanes) and 16, 17 (the record's last piece) are nobody else's values
    for c in (8, 9, 16, 17):
        for d in range(18):
            assert d == c or not np.array_equal(wave[:, c], wave[:, d]), (c, d)


@pytest.mark.parametrize("H,W,D", [(12, 20, 8), (16, 16, 16)])
@pytest.mark.parametrize("P", [1, 31, 33, 64])
def test_every_piece_reaches_its_channel(gpu, P, H, W, D):
    _check_mapping(gpu, _covering_inputs(P, H, W, D))


def test_every_piece_reaches_its_channel_with_long_rows(gpu):
    """The smallest P the route renders with the long-row instantiation (one Gaussian more than the longest short row holds), every
    box covering a 16 x 16 x 16 grid: every unit consumes all of them, in several passes of its list."""
    H = W = D = 16
    total = 64 * K_WROW + 1
    assert _route_kernel(total - 1, H, W, D) == ROUTE_WAVE and _route_kernel(total, H, W, D) == ROUTE_WAVE_LONG
    si = _covering_inputs(total - 1, H, W, D)   # (+ the whole-grid Gaussian)
    assert si.means3D.shape[0] == total
    _check_mapping(gpu, si)


# ---- 2. and 3.: launches with more units than resident waves ------------------------------------------------------------------------
def _tensors(gpu, si):
    pi, mi, radii, cov6 = prep(si)
    return to_dev(gpu, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6)


def _plans(gpu, si):
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import SplatForwardPlan
    t = _tensors(gpu, si)
    wave = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=0)
    tile = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=0)
    exact = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=_lib.GF_EXACT_FP32)
    return t, wave, tile, exact


def _three_way(gpu, si):
    """wave == tile bit for bit, both within 1e-4 of the exact-fp32 kernel; returns the units that took a list."""
    from gaussianformer_amd import _lib
    _, wave, tile, exact = _plans(gpu, si)
    before = _took(wave)
    got = wave.run().cpu().numpy()
    took = _took(wave) - before
    assert wave.state_words()[1] == _lib.GF_PATH_MATRIX_CORE_WAVE
    with _lib.option("splat.mfma_tile_kernel", 1):
        ref = tile.run().cpu().numpy()
    assert tile.state_words()[1] == _lib.GF_PATH_MATRIX_CORE
    assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(ref))
    assert_logits_close(got, exact.run().cpu().numpy(), tol=1e-4)
    return took


def _units(si):
    return -(-si.H // 8) * -(-si.W // 8) * 4 * -(-si.D // 8)


def test_units_that_take_their_list_across_frames_and_graph_replays(gpu):
    """96 x 96 x 32: 2 304 units on 2 048 waves, the last 256 claimed long after every unit 0 has published.  Units took lists; two
    frames alternate through one workspace, eagerly and under one captured graph replayed, and every result is the frame's own on
    a workspace of its own."""
    fa = make_splat_inputs("nuscenes_gs25600_solid", seed=61, P=3000, H=96, W=96, D=32)
    fb = make_splat_inputs("nuscenes_gs25600_solid", seed=62, P=3000, H=96, W=96, D=32)
    assert _units(fa) == 2304
    took = _three_way(gpu, fa)
    print("units that took a list:", took, "of", _units(fa))
    assert took > 0
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
    for k in (0, 1):
        load((ta, tb)[k])
        assert np.array_equal(_bits(plan.run().cpu().numpy()), _bits(want[k])), k
    assert _took(plan) > before
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.run(); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.run(stream=s.cuda_stream)
    before = _took(plan)
    for k in (1, 0):   # (one graph, replayed twice: the device-side call counter moves on without the host)
        load((ta, tb)[k])
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(plan.logits.cpu().numpy()), _bits(want[k])), k
    assert _took(plan) > before


def _crowded_inputs():
    """tests/test_splat_shared_list_gpu.py, test_a_list_that_is_not_published: 96 x 96 x 32, fifteen hundred small Gaussians inside
    supertile (10, 8) = s 128 (XCD 0, q = 16), whose units 1..15 are XCD-local indices 258..272: all claimed by waves that have
    finished a unit.  Its list is longer than kBwdList = 256 and is never published (nor are its eight neighbours', ~670
    candidates each), so the waves that claim those units build their own lists from 1 500-candidate rows, and claim a unit of a far
    supertile, whose list they take, before or after (the claims of an XCD go supertile by supertile).  Returns (inputs, claimed units, those of them in supertiles whose list is short enough to be published)."""
    H = W = 96
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=63, P=3000, H=H, W=W, D=32)
    nsy, per_super, srow, scol = W // 8, 16, 10, 8
    s = srow * nsy + scol
    nsuper_xcd = (H // 8) * nsy // 8
    first = nsuper_xcd + (s // 8) * (per_super - 1)
    claimed = _units(si) - 2048
    assert s % 8 == 0 and first >= 2048 // 8 and first + per_super - 1 <= _units(si) // 8 and claimed == 256
    rng = np.random.default_rng(64)
    lo = np.asarray(si.pc_min, dtype=np.float64)
    si.means3D[:1500, 0] = (lo[0] + (8 * srow + 8 * rng.random(1500)) * si.grid_size).astype(np.float32)
    si.means3D[:1500, 1] = (lo[1] + (8 * scol + 8 * rng.random(1500)) * si.grid_size).astype(np.float32)
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
    return si, claimed, may_take


def test_units_next_to_a_list_that_is_not_published(gpu):
    from gaussianformer_amd import _lib
    si, claimed, may_take = _crowded_inputs()
    took = _three_way(gpu, si)
    print("units that took a list:", took, "of", claimed, "claimed units;", may_take, "of them in supertiles whose list is published")
    assert 0 < took <= may_take

    # the same launch as GF_PREPARE_BACKWARD, then the matrix-core backward on what it left, against the exact backward
    pi, mi, radii, cov6 = prep(si)
    g = np.random.default_rng(65).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    prepared, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PREPARE_BACKWARD)
    words = _lib.SplatState.of(state)
    assert words.path == _lib.GF_PATH_MATRIX_CORE_WAVE and words.rows_ready, words
    got = hip_splat_backward(gpu, si, t, state, None, g, flags=_lib.GF_MFMA_SPLAT | _lib.GF_RECORDS_VALID)
    plain, t0, state0, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    assert np.array_equal(_bits(prepared["logits"]), _bits(plain["logits"]))
    exact = hip_splat_backward(gpu, si, t0, state0, None, g, flags=_lib.GF_EXACT_FP32)
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    for a, c, what in zip(got, exact, ("means", "opacity", "semantics", "cov")):
        assert_grad_rows_close(a, c.reshape(a.shape), whole, what=what)
