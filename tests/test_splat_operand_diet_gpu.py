"""The wave kernel's group operand phase without the work the result does not need: dead lanes of a partial group keep the record
of the group's first Gaussian (no `live` selects: their one-hot rows are -32768 everywhere, so their weights are exactly +0), theta's
three f16 terms are formed two values per conversion, and S' is split into f16 hi + lo before the transpose.  Nothing may change:
everywhere the wave kernel equals the tile kernel (``splat.mfma_tile_kernel``, which keeps the selects, ``split3`` and the split
behind the transpose) bit for bit -- the logits compared as int32, so +0 and -0 differ.

Every Gaussian here has radius 1 and its centre voxel in the interior of one unit (a double brick of 4 x 4 x 8 voxels), so it hits
exactly that unit; the hit counts are recounted on the CPU from ``oracle.prepare_splat_inputs`` and asserted."""
import numpy as np
import pytest
import torch

from gaussianformer_amd import _lib
from gaussianformer_amd.local_aggregate import SplatForwardPlan
from gaussianformer_amd.synthetic import cov_inverse, make_splat_inputs

from splat_cases import (SHORT_ROW_P, WAVE, WAVE_LONG, all_routes_agree, bwd, range_bounds, render_kernel, run_plan, same_bits, tensors,
                         wave_equals_tile)
from util import assert_grad_rows_close, hip_splat_forward, prep, whole_grid_rows

pytestmark = pytest.mark.gpu

COUNTS = (1, 31, 32, 33, 63)         # hits of a unit: the last group has 31, 1, 0, 31 and 1 dead rows
GRIDS = {
    # grid -> origins of the five counted units (a unit: 4 x 4 columns, 8 voxels deep)
    (16, 16, 16): [(0, 0, 0), (4, 0, 8), (0, 4, 0), (4, 4, 8), (0, 0, 8)],
    # 12 x 20 x 16: the last supertile row holds x = 8 .. 11 only, the last supertile column y = 16 .. 19 only
    (12, 20, 16): [(8, 16, 0), (8, 16, 8), (8, 12, 0), (4, 16, 8), (0, 0, 0)],
    # 24 x 36 x 16: 120 units -- from 64 workgroups on a GF_PREPARE_BACKWARD call runs the instantiation of its own (the render
    # launch finishes the backward's row layout; smaller grids prepare nothing and take the default instantiation)
    (24, 36, 16): [(16, 32, 0), (16, 32, 8), (20, 28, 0), (0, 0, 8), (12, 16, 0)],
}
PREPARING = (24, 36, 16)


def _placed_inputs(H, W, D, plan, seed):
    """One Gaussian per entry of ``plan`` = [(unit origin, centre offset inside the unit)], in that order: radius 1, centre voxel =
    origin + offset with offset in [1, 2] x [1, 2] x [1, 6], so its 3 x 3 x 3 box lies inside the unit.  Semantics: 18 distinct values,
    odd channels negative; distinct opacities; rotated covariances of 0.4 .. 0.9 m."""
    n = len(plan)
    si = make_splat_inputs("nuscenes_gs144000", seed=seed, P=n, H=H, W=W, D=D)   # (this config appends no whole-grid Gaussian)
    assert si.means3D.shape[0] == n
    rng = np.random.default_rng(seed)
    cell = np.array([[o[0] + d[0], o[1] + d[1], o[2] + d[2]] for o, d in plan], dtype=np.float64)
    lo = np.asarray(si.pc_min, dtype=np.float64)
    si.means3D[:] = (lo + (cell + 0.5 + rng.uniform(-0.3, 0.3, (n, 3))) * si.grid_size).astype(np.float32)
    si.scales[:] = np.float32(0.15)   # radius = ceil(0.15 * 3 / 0.5) = 1
    si.cov3D[:] = cov_inverse(rng.uniform(0.4, 0.9, (n, 3)), rng.standard_normal((n, 4))).astype(np.float32)
    sem = rng.uniform(0.25, 2.0, size=(n, 18)) * np.where(np.arange(18) % 2 == 1, -1.0, 1.0)
    si.semantics[:] = sem.astype(np.float32)
    si.opacities[:] = rng.permutation(np.linspace(0.05, 0.95, n)).astype(np.float32).reshape(si.opacities.shape)
    return si


def _unit_hits(si, mi, radii):
    """Hits of every unit, counted from the integer boxes: {unit origin: ascending Gaussian ids}."""
    mi, r = np.asarray(mi, dtype=np.int64), np.asarray(radii, dtype=np.int64).reshape(-1, 1)
    dims = np.array([si.H, si.W, si.D])
    blo, bhi = np.maximum(0, mi - r), np.minimum(dims, mi + r + 1)
    hits = {}
    for x0 in range(0, si.H, 4):
        for y0 in range(0, si.W, 4):
            for z0 in range(0, si.D, 8):
                o = np.array([x0, y0, z0])
                m = ((blo < o + [4, 4, 8]) & (bhi > o)).all(axis=1)
                if m.any():
                    hits[(x0, y0, z0)] = np.flatnonzero(m)
    return hits


def _random_plan(origins, counts, rng):
    plan = []
    for o, c in zip(origins, counts):
        plan += [(o, (int(rng.integers(1, 3)), int(rng.integers(1, 3)), int(rng.integers(1, 7)))) for _ in range(c)]
    order = rng.permutation(len(plan))   # (the units' Gaussians interleaved in id order, as in a scene)
    return [plan[i] for i in order]


def _counted_inputs(shape, seed=0, padding=()):
    """The five counted units of ``shape`` (+ ``padding`` = [(origin, count)] further units), counts asserted."""
    H, W, D = shape
    rng = np.random.default_rng(1000 + seed + H)
    origins = GRIDS[shape] + [o for o, _ in padding]
    counts = list(COUNTS) + [c for _, c in padding]
    si = _placed_inputs(H, W, D, _random_plan(origins, counts, rng), seed=500 + seed + H)
    pi, mi, radii, cov6 = prep(si)
    assert (np.asarray(radii) == 1).all()
    hits = _unit_hits(si, mi, radii)
    assert {o: len(h) for o, h in hits.items()} == dict(zip(origins, counts))
    return si, (pi, mi, radii, cov6)


def _forward_all_routes(gpu, si, prepped, exact_tol=1e-4):
    """splat_cases.all_routes_agree; a GF_PREPARE_BACKWARD call prepares on the ``PREPARING`` grid and on no other."""
    return all_routes_agree(gpu, si, prepped, exact_tol=exact_tol, rows_ready=(si.H, si.W, si.D) == PREPARING)


# ---- partial groups of every kind, channels 8 / 9 / 17, every short-row route ----------------------------------------------------
@pytest.mark.parametrize("shape", sorted(GRIDS))
def test_partial_groups_of_every_kind_on_every_route(gpu, shape):
    si, prepped = _counted_inputs(shape)
    wave = _forward_all_routes(gpu, si, prepped)
    vox = wave.reshape(si.H, si.W, si.D, 18)
    for (x0, y0, z0), c in zip(GRIDS[shape], COUNTS):
        unit = vox[x0:x0 + 4, y0:y0 + 4, z0:z0 + 8].reshape(-1, 18)
        assert (unit != 0).any(axis=0).all(), ((x0, y0, z0), c)
        # channels 8 and 9 (S' rows both half-lanes write), 16 and 17 (the second half-lane's last rows): nobody else's values
        for ch in (8, 9, 16, 17):
            for d in range(18):
                assert d == ch or not np.array_equal(unit[:, ch], unit[:, d]), ((x0, y0, z0), ch, d)
    # a unit nobody hits receives nothing at all: +0 in every bit
    counted = np.zeros((si.H, si.W, si.D), dtype=bool)
    for x0, y0, z0 in GRIDS[shape]:
        counted[x0:x0 + 4, y0:y0 + 4, z0:z0 + 8] = True
    assert not wave.view(np.int32).reshape(si.H, si.W, si.D, 18)[~counted].any()


# ---- a first Gaussian that would show a leak -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,count", [((16, 16, 16), 5), ((12, 20, 16), 37)])
def test_a_strong_thin_first_gaussian_does_not_leak_through_dead_rows(gpu, shape, count):
    """The first Gaussian of a partial group (27 dead rows; 5 live ones behind a full group: 27 dead rows again) has opacity x
    semantics of 20 .. 60 with both signs (the range verdict's limit is 64) and a rotated covariance whose accuracy bound is 1 100 of
    the theta verdict's 1 200; every other hit of the group is 1e-3 of an ordinary one.  The dead rows carry that record: through a
    weight that is not exactly +0 it would move the logits by far more than an ulp."""
    H, W, D = shape
    origin = GRIDS[shape][0]
    rng = np.random.default_rng(77 + count)
    si = _placed_inputs(H, W, D, _random_plan([origin], [count], rng), seed=70 + count)
    first = 32 * (count // 32)   # ids ascend in the queue: the first Gaussian of the unit's last group
    si.semantics[first:] *= np.float32(1e-3)
    si.opacities[first] = np.float32(1.0)
    si.semantics[first] = (rng.uniform(20.0, 60.0, 18) * np.where(np.arange(18) % 3 == 0, -1.0, 1.0)).astype(np.float32)
    pi, mi, radii, cov6 = prep(si)
    # thin, rotated, scaled so that the accuracy bound of range_of is 1 100
    A = cov_inverse(np.array([[0.05, 0.4, 0.2]]), rng.standard_normal((1, 4)))[0]
    c = np.array([A[0, 0], A[1, 1], A[2, 2], A[0, 1], A[1, 2], A[0, 2]])
    near = range_bounds(c[None].astype(np.float32), np.array([1]), H, W, D)[1][0]
    s = ((np.sqrt(1100.0 / 0.7213475204444817) - 4.3) / (np.sqrt(near / 0.7213475204444817) - 4.3)) ** 2
    cov6[first] = (c * s).astype(np.float32)
    b, nb = range_bounds(cov6, np.asarray(radii), H, W, D)
    assert (b < 3e4).all() and (nb < 1200).all() and 1050 < nb[first] < 1150
    assert np.abs(si.opacities[first] * si.semantics[first]).max() < 64 and np.abs(si.opacities[first] * si.semantics[first]).min() >= 20
    hits = _unit_hits(si, mi, radii)
    assert list(hits) == [origin] and len(hits[origin]) == count and hits[origin][first] == first
    wave = _forward_all_routes(gpu, si, (pi, mi, radii, cov6), exact_tol=None)
    x0, y0, z0 = origin
    unit = wave.reshape(H, W, D, 18)[x0:x0 + 4, y0:y0 + 4, z0:z0 + 8]
    assert np.abs(unit).max() > 1.0   # (the strong Gaussian is seen where it belongs)


# ---- voxels that receive only exact zeros ------------------------------------------------------------------------------------------------
def test_exact_zeros_next_to_negative_dead_rows_stay_plus_zero(gpu):
    """Three hits in one unit: Gaussian 0 in the unit's low corner (box x0 .. x0 + 2, z0 .. z0 + 2) with every channel negative and
    large; Gaussians 1 and 2 in its high corner with channels 3, 8 and 17 exactly zero.  At the unit's last voxel -- inside the boxes
    of 1 and 2, outside that of 0 -- those channels receive (+0) x w from the live rows 1 and 2 and (negative S') x (+0) = -0 from
    row 0 and from the 29 dead rows that carry record 0: the sum is the tile kernel's +0, all 32 bits.  Voxels outside every box
    receive nothing but such products in all 18 channels."""
    H = W = D = 16
    origin = (4, 4, 8)
    plan = [(origin, (1, 1, 1)), (origin, (2, 2, 6)), (origin, (2, 2, 6))]
    si = _placed_inputs(H, W, D, plan, seed=90)
    si.semantics[0] = -np.linspace(30.0, 47.0, 18).astype(np.float32)
    si.opacities[0] = np.float32(1.0)
    si.semantics[1:, [3, 8, 17]] = np.float32(0.0)
    prepped = prep(si)
    hits = _unit_hits(si, prepped[1], prepped[2])
    assert list(hits) == [origin] and list(hits[origin]) == [0, 1, 2]
    wave = _forward_all_routes(gpu, si, prepped)
    bits = wave.view(np.int32).reshape(H, W, D, 18)
    x0, y0, z0 = origin
    last = bits[x0 + 3, y0 + 3, z0 + 7]
    assert (last[[3, 8, 17]] == 0).all(), last
    assert (np.delete(last, [3, 8, 17]) != 0).all(), last                  # (the live rows do reach that voxel)
    assert not bits[x0 + 3, y0 + 3, z0 + 3].any() and not bits[x0, y0, z0 + 4].any()   # between the boxes: zeros only
    assert (wave.reshape(H, W, D, 18)[x0 + 1, y0 + 1, z0 + 1] < -1.0).all()          # (Gaussian 0 where it belongs)


# ---- long rows, and one call replayed from a captured graph ------------------------------------------------------------------------
def test_long_rows(gpu):
    """The smallest P the route renders with the long-row instantiation (default, labels and, on this grid, GF_PREPARE_BACKWARD): the
    five counted units as before, the rest of the Gaussians in the units of the supertiles that hold no counted unit (crowded:
    several passes of the list, each ending in a flush, which forms no partial group)."""
    shape = PREPARING
    total = SHORT_ROW_P + 1
    assert render_kernel(total - 1, shape) == WAVE and render_kernel(total, shape) == WAVE_LONG
    counted = {(x // 8, y // 8) for x, y, _ in GRIDS[shape]}
    others = [(x, y, z) for x in range(0, shape[0], 4) for y in range(0, shape[1], 4) for z in (0, 8) if (x // 8, y // 8) not in counted]
    rest = total - sum(COUNTS)
    padding = [(o, rest // len(others) + (1 if i < rest % len(others) else 0)) for i, o in enumerate(others)]
    si, prepped = _counted_inputs(shape, seed=3, padding=padding)
    assert si.means3D.shape[0] == total
    _forward_all_routes(gpu, si, prepped)


def test_one_workspace_eager_and_replayed_from_a_graph(gpu):
    si, prepped = _counted_inputs((12, 20, 16), seed=5)
    t = tensors(gpu, si, prepped)
    tile = run_plan(SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=0), tile=True)
    want = tile[0]
    plan = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=0)
    wave_equals_tile(run_plan(plan), tile)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.run(); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.run(stream=s.cuda_stream)
    for _ in range(2):
        plan.logits.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        same_bits(plan.logits.cpu().numpy(), want, "replayed vs tile kernel")


# ---- the prepared backward on what the new forward leaves -----------------------------------------------------------------------------
def test_prepared_backward_after_the_forward(gpu):
    si, prepped = _counted_inputs(PREPARING, seed=7)
    pi, mi, radii, cov6 = prepped
    g = np.random.default_rng(65).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    prepared, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PREPARE_BACKWARD)
    words = _lib.SplatState.of(state)
    assert words.path == _lib.GF_PATH_MATRIX_CORE_WAVE and words.rows_ready, words
    got = bwd(gpu, si, t, state, g, flags=_lib.GF_MFMA_SPLAT | _lib.GF_RECORDS_VALID)
    plain, t0, state0, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    same_bits(prepared["logits"], plain["logits"], "GF_PREPARE_BACKWARD vs default")
    exact = bwd(gpu, si, t0, state0, g, flags=_lib.GF_EXACT_FP32)
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    assert not whole.any()
    for a, c, what in zip(got, exact, ("means", "opacity", "semantics", "cov")):
        assert_grad_rows_close(a, c.reshape(a.shape), whole, what=what)
