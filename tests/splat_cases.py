"""TEST INFRASTRUCTURE shared by the splat forward's tests: the kernel constants they use, the route hook, the judges ("every
route gives the same bits"), the runners and the scenes.  Never imported by the product.

The rule.  The wave kernel, the tile kernel (``splat.mfma_tile_kernel``), the GF_PREPARE_BACKWARD and the labels instantiations
take a unit's hits in the same groups and run the same arithmetic on them, so their logits are compared ON BITS (``same_bits``:
int32 views, so +0 and -0 differ and equal NaNs are equal); all of them are held to the exact-fp32 kernel at the matrix-core tests'
1e-4 scaled (tests/util.py).  Seeds and shapes come in as arguments: every caller keeps its own inputs, and
tests/test_splat_cases.py pins the scenes to recorded digests and the constants to their source lines."""
import contextlib
import ctypes
import types

import numpy as np
import torch

import oracle
from gaussianformer_amd import _lib
from gaussianformer_amd.local_aggregate import SplatForwardPlan, splat_forward, splat_forward_labels
from gaussianformer_amd.synthetic import cov_inverse, make_splat_inputs

from util import assert_logits_close, hip_splat_backward, prep, to_dev

# ---- constants ------------------------------------------------------------------------------------------------------------------
CONSTANTS = {   # file under gaussianformer_amd/csrc -> its ``constexpr int <name> = <literal>;``
    "gf_common.hpp": dict(kSuper=8,             # a supertile is 8 x 8 voxel columns
                          kWRow=618,            # the longest bitmask row (in words) the short-row instantiation holds in LDS
                          kLongWords=4096,      # ... and the longest the long-row instantiation takes
                          kBwdList=256,         # entries of a candidate list a unit 0 publishes
                          kFwdCounters=4608),   # flag section: one 64-word block per XCD; word 0 = next unit, word 32 = units that took a list
    "splat_fwd.hip": dict(kRowLayoutBlocks=64,  # workgroups of the render launch that finish the backward's row layout
                          kLSumAt=3968),        # LDS dword offset of the long-row instantiation's summary row
}
K = types.SimpleNamespace(**{name: value for table in CONSTANTS.values() for name, value in table.items()})
SHORT_ROW_P = 64 * K.kWRow   # the most Gaussians (64 per word) a short row holds: one more takes the long-row instantiation
RESIDENT_WAVES = 2048         # 8 waves per compute unit x 256 compute units: units beyond them are claimed by waves that finished one

# the words of gf_debug_splat_route, in the order of gf::ForwardRoute, and the values of word 0 (enum RenderKernel)
WORDS = ("kernel", "labels", "prep_backward", "exp", "prep_waves", "prep_blocks", "prep_grid", "verify", "lattice", "prescale",
         "range_theta_here", "range_flags", "one_verdict", "summaries", "row_layout", "tile_counter_init", "bwd_counter_init",
         "render_grid")
EXACT_TILE, ARBITRARY, MFMA_TILE, WAVE, WAVE_LONG = range(5)
NO_LABELS = -1


# ---- route and geometry ---------------------------------------------------------------------------------------------------------
def splat_route(variant, flags, label_mode, P, N, grid):
    """What the library's decision function gives the call, as ``{word: value}``; launches nothing (no GPU needed)."""
    lib = _lib.load()
    fn = lib.gf_debug_splat_route
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 8 + [ctypes.c_void_p, ctypes.c_int]
    out = (ctypes.c_int * len(WORDS))()
    rc = fn(variant, flags, label_mode, P, N, *grid, out, len(WORDS))
    assert rc == len(WORDS), lib.gf_last_error()
    return dict(zip(WORDS, out))


def render_kernel(P, grid):
    """Word 0 of the route of a default call on the dense grid with a workspace handed over zeroed (``splat_forward``, a plan)."""
    return splat_route(_lib.GF_SPLAT_BASE, _lib.GF_WORKSPACE_ZEROED, NO_LABELS, P, grid[0] * grid[1] * grid[2], grid)["kernel"]


def units(grid):
    """Double bricks (4 x 4 x 8 voxels) of a grid: four per 8 x 8 supertile and 8 voxels of depth."""
    h, w, d = grid
    return -(-h // 8) * -(-w // 8) * 4 * -(-d // 8)


def took(plan):
    """Units that took their supertile's list from its unit 0, over all calls on the plan's workspace -- synchronises."""
    torch.cuda.synchronize()
    w = plan.workspace[:32768].view(torch.int32)
    return int(sum(int(w[K.kFwdCounters + 64 * x + 32]) for x in range(8)))


def range_bounds(cov6, radii, H, W, D, step=(0.5, 0.5, 0.5)):
    """numpy twin of ``range_of`` in gf_splat_prep_kernel: (overflow bound, accuracy bound) per Gaussian."""
    c = np.abs(cov6.astype(np.float64))
    sx, sy, sz = step
    ex, ey, ez = (np.minimum(radii, H) + 3) * sx, (np.minimum(radii, W) + 3) * sy, (np.minimum(radii, D) + 5) * sz
    bound = 0.7213475204444817 * (c[:, 0] + c[:, 1] + c[:, 2]) * (ex * ex + ey * ey + ez * ez)
    rx, ry, rz = 1.5 * sx, 1.5 * sy, 3.5 * sz
    Q = c[:, 0] * rx * rx + c[:, 1] * ry * ry + c[:, 2] * rz * rz + 2.0 * (c[:, 3] * rx * ry + c[:, 4] * ry * rz + c[:, 5] * rx * rz)
    return bound, 0.7213475204444817 * (4.3 + np.sqrt(Q)) ** 2


def integer_boxes(mi, radii, H, W, D):
    """[lo, hi) voxel box of every Gaussian (src/auxiliary.h getRect: mean +- radius, clipped to the grid), checked against the
    oracle's binning: the box volumes are its tiles_touched."""
    dims = np.array([H, W, D], dtype=np.int64)
    mi, r = np.asarray(mi, np.int64), np.asarray(radii, np.int64)[:, None]
    lo = np.minimum(dims, np.maximum(0, mi - r))
    hi = np.minimum(dims, np.maximum(0, mi + r + 1))
    touched, _, _ = oracle.box_offsets(mi, radii, H, W, D)
    assert np.array_equal(np.prod(hi - lo, axis=1).astype(np.uint32), touched)
    return lo, hi


# ---- running --------------------------------------------------------------------------------------------------------------------
def tensors(gpu, si, prepped=None):
    """The eight inputs of a call on the device; ``prepped`` = (pts_int, means_int, radii, cov6), default ``prep(si)``."""
    pi, mi, radii, cov6 = prep(si) if prepped is None else prepped
    return to_dev(gpu, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6)


def plans(gpu, si, flags=0):
    """``(t, wave, tile, exact)``: three plans, each with a workspace of its own, on one set of tensors (run ``tile`` under the option)."""
    t = tensors(gpu, si)
    wave = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=flags)
    tile = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=flags)
    exact = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=flags | _lib.GF_EXACT_FP32)
    return t, wave, tile, exact


def _kernel(tile):
    return _lib.option("splat.mfma_tile_kernel", 1) if tile else contextlib.nullcontext()


def run_route(t, si, flags, tile=False):
    """One base-variant forward on the stream's workspace (``tile``: under ``splat.mfma_tile_kernel``): (logits, SplatState)."""
    with _kernel(tile):
        logits, _, _, _, state = splat_forward(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=flags)
        return logits.cpu().numpy(), _lib.SplatState.of(state)


def run_plan(plan, tile=False):
    """One run of a plan (``tile``: under ``splat.mfma_tile_kernel``): (logits, SplatState)."""
    with _kernel(tile):
        logits = plan.run().cpu().numpy()
        return logits, _lib.SplatState.of(plan.state_words())


def bwd(gpu, si, t, state, g, flags=0):
    """The base variant's backward behind a forward's tensors and state block: the four gradients as numpy arrays."""
    return hip_splat_backward(gpu, si, t, state, None, g, flags=flags)


def alternate_frames(plan, t, frames, want, eager_order, replay_order):
    """Frames (each a list of tensors like ``t``, the tensors ``plan`` is bound to) alternate through ONE plan: eagerly in
    ``eager_order``, then under one captured graph replayed in ``replay_order`` (the device-side call counter moves on without the
    host).  Every result is ``want[k]``'s bits, and units took lists in both phases."""
    def load(src):
        for dst, s in zip(t, src):
            dst.copy_(s)

    before = took(plan)
    for k in eager_order:
        load(frames[k])
        same_bits(plan.run().cpu().numpy(), want[k], f"eager, frame {k}")
    assert took(plan) > before
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.run(); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.run(stream=s.cuda_stream)
    before = took(plan)
    for k in replay_order:
        load(frames[k])
        g.replay()
        torch.cuda.synchronize()
        same_bits(plan.logits.cpu().numpy(), want[k], f"replayed, frame {k}")
    assert took(plan) > before


# ---- judges ---------------------------------------------------------------------------------------------------------------------
def _bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.int32), x.dtype
    return x.view(np.int32)


def same_bits(a, b, what, signed_zero_ok=False):
    """``a`` and ``b`` (float32, or int32 views of it) have one shape and the same bits; ``signed_zero_ok``: the same values, and
    the same bits wherever the value is not zero.  Reports the first differing index with both values in hex."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    differ = _bits(a) != _bits(b)
    if signed_zero_ok:
        differ &= ~((_bits(a).view(np.float32) == 0) & (_bits(b).view(np.float32) == 0))
    if differ.any():
        at = tuple(int(i) for i in np.argwhere(differ)[0])
        raise AssertionError(f"{what}: {int(differ.sum())} values of {differ.size} differ, the first at {at}: "
                             f"0x{int(_bits(a)[at]) & 0xFFFFFFFF:08x} vs 0x{int(_bits(b)[at]) & 0xFFFFFFFF:08x}")


def wave_equals_tile(wave, tile, exact=None, exact_tol=1e-4):
    """The two-route judge on finished runs, each ``(logits, SplatState)``: the wave kernel rendered the one, the tile kernel the
    other, the logits are finite and the same bits; ``exact`` (logits of the exact-fp32 kernel): within ``exact_tol`` scaled."""
    (got, gstate), (ref, rstate) = wave, tile
    assert gstate.path == _lib.GF_PATH_MATRIX_CORE_WAVE, gstate
    assert rstate.path == _lib.GF_PATH_MATRIX_CORE, rstate
    assert np.isfinite(_bits(got).view(np.float32)).all()
    same_bits(got, ref, "wave kernel vs tile kernel")
    if exact is not None:
        assert_logits_close(got, exact, tol=exact_tol)


def plans_agree(gpu, si):
    """``wave_equals_tile`` on three fresh plans, held to the exact-fp32 kernel at 1e-4; returns the units that took a list."""
    _, wave, tile, exact = plans(gpu, si)
    before = took(wave)
    got = run_plan(wave)
    n = took(wave) - before
    wave_equals_tile(got, run_plan(tile, tile=True), exact=exact.run().cpu().numpy())
    return n


def all_routes_agree(gpu, si, prepped, exact_tol=1e-4, rows_ready=None, labels_only=False):
    """default == tile == GF_PREPARE_BACKWARD == labels instantiation's logits, bit for bit; labels = argmax (the first of equal
    maxima, like the kernel; ``labels_only``: also from the call that keeps no logits); the default run is dense, on the wave kernel
    and without a verdict; ``rows_ready``: what the prepared run's state block must say (None: not pinned); within ``exact_tol`` of
    the exact-fp32 kernel, which must not be a matrix-core one (``exact_tol=None``: not compared -- for inputs at the thin end of the
    theta verdict, where the exact kernel's own fp32 quadratic form cancels from terms of several hundred).  Returns the wave
    kernel's logits."""
    t = tensors(gpu, si, prepped)
    V, grid = _lib.GF_SPLAT_BASE, (si.H, si.W, si.D)
    wave, wstate = run_route(t, si, 0)
    assert (wstate.not_dense, wstate.path, wstate.verdict) == (False, _lib.GF_PATH_MATRIX_CORE_WAVE, 0), wstate   # "matrix cores"
    wave_equals_tile((wave, wstate), run_route(t, si, _lib.GF_MFMA_SPLAT, tile=True))
    prepared, pstate = run_route(t, si, _lib.GF_PREPARE_BACKWARD)
    assert pstate.path == _lib.GF_PATH_MATRIX_CORE_WAVE and (rows_ready is None or pstate.rows_ready == rows_ready), pstate
    same_bits(wave, prepared, "default vs GF_PREPARE_BACKWARD")
    labels, kept = splat_forward_labels(V, *t, *grid, keep_logits=True)
    same_bits(kept.cpu().numpy(), wave, "labels instantiation's logits")
    want = wave.argmax(axis=1)
    assert np.array_equal(labels.cpu().numpy(), want)
    if labels_only:
        assert np.array_equal(splat_forward_labels(V, *t, *grid).cpu().numpy(), want)
    if exact_tol is not None:
        exact, estate = run_route(t, si, _lib.GF_EXACT_FP32)
        assert estate.path not in (_lib.GF_PATH_MATRIX_CORE_WAVE, _lib.GF_PATH_MATRIX_CORE), estate
        assert_logits_close(wave, exact, tol=exact_tol)
    return wave


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def covering_scene(P, H, W, D, seed, rng_seed, distinct=False):
    """P drawn Gaussians (the config appends the whole-grid one: P + 1 in all) whose boxes all cover the grid, so every unit takes
    all of them: scales of 3..5 m (6..10 voxels; the box reaches scale_multiplier times that) and the covariances of those scales,
    which keeps the exponents far inside the matrix-core range.  Plain: a negative semantic value in the whole-grid Gaussian and
    in Gaussian 0, and a Gaussian of opacity 0.  ``distinct``: 18 distinct semantic values per Gaussian, both signs in each and
    one sign per channel (a channel's sum over many Gaussians does not cancel, so the scaled 1e-4 against the exact kernel's own
    fp32 summation means the same at P = 1 and at long rows), and a distinct opacity each -- a swapped piece, half-lane or Gaussian
    changes bits.  Returns (inputs, prepared inputs)."""
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=seed, P=P, H=H, W=W, D=D)
    rng = np.random.default_rng(rng_seed)
    si.scales[:P] = (3.0 + 2.0 * rng.random((P, 3))).astype(np.float32)
    si.cov3D[:P] = cov_inverse(si.scales[:P], rng.standard_normal((P, 4))).astype(np.float32)
    n = si.means3D.shape[0]
    assert n == P + 1
    if distinct:
        sem = rng.uniform(0.25, 2.0, size=(n, 18)) * np.where(np.arange(18) % 2 == 1, -1.0, 1.0)
        si.semantics[:] = sem.astype(np.float32)
        si.opacities[:] = rng.permutation(np.linspace(0.05, 0.95, n)).astype(np.float32).reshape(si.opacities.shape)
        assert all(len(np.unique(row)) == 18 for row in si.semantics[:min(n, 128)])
        assert len(np.unique(si.opacities)) == n
    else:
        si.semantics[-1, 2] = -0.5       # (the whole-grid Gaussian: seen by every voxel)
        si.semantics[0, 5] = -1.25
        if P > 1:
            si.opacities[1] = 0.0         # a Gaussian that contributes nothing
    prepped = prep(si)
    assert (np.asarray(prepped[2]).reshape(n, -1).min(axis=1) >= max(H, W, D)).all(), "every box covers the grid"
    return si, prepped


def crowded_supertile_scene(seed, rng_seed):
    """96 x 96 x 32: 18 supertiles per XCD, 16 units each; an XCD's indices are its 18 units 0, then 15 units per supertile,
    supertile by supertile; the first 256 indices are the waves' static first units (they never look for a list), the other 32 are
    claimed later -- 256 units in all.  Supertile (10, 8), cells 80..87 x 64..71, is s = 128: XCD 0, q = 16, its units 1..15 are
    indices 258..272, all claimed.  Fifteen hundred small Gaussians inside it: the list is longer than kBwdList, unit 0 leaves the
    length word cleared, the fifteen read the cleared word and build their own lists from 1 500-candidate rows.  (The boxes reach
    into the eight neighbouring supertiles, ~670 candidates each: their lists stay unpublished too, and five of them -- s = 127,
    129, 139, 140, 141 -- have claimed units as well.)  So at most 256 - 15 units take a list.  Returns (inputs, claimed units,
    ``may_take`` = those of them in supertiles whose list is short enough to be published: a CPU model of the kernel's dealing)."""
    H = W = 96
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=seed, P=3000, H=H, W=W, D=32)
    nsy, per_super, srow, scol = W // 8, 16, 10, 8
    s = srow * nsy + scol
    nsuper_xcd = (H // 8) * nsy // 8
    first = nsuper_xcd + (s // 8) * (per_super - 1)             # XCD-local index of the supertile's unit 1
    nunits = units((H, W, 32))
    claimed = nunits - RESIDENT_WAVES
    assert s % 8 == 0 and first >= RESIDENT_WAVES // 8 and first + per_super - 1 <= nunits // 8 and claimed == 256
    rng = np.random.default_rng(rng_seed)
    lo = np.asarray(si.pc_min, dtype=np.float64)
    si.means3D[:1500, 0] = (lo[0] + (8 * srow + 8 * rng.random(1500)) * si.grid_size).astype(np.float32)
    si.means3D[:1500, 1] = (lo[1] + (8 * scol + 8 * rng.random(1500)) * si.grid_size).astype(np.float32)
    # the claimed units whose supertile's list is short enough to be published (boxes as auxiliary.h:8-20 clips them)
    _, mi, radii, _ = prep(si)
    mi, r3 = np.asarray(mi, dtype=np.int64), np.asarray(radii, dtype=np.int64).reshape(len(mi), -1)
    blo, bhi = np.maximum(0, mi[:, :2] - r3[:, :1]), np.minimum([H, W], mi[:, :2] + r3[:, :1] + 1)
    may_take = 0
    for t in range((H // 8) * nsy):
        x0, y0 = 8 * (t // nsy), 8 * (t % nsy)
        ncand = int(((blo[:, 0] < x0 + 8) & (bhi[:, 0] > x0) & (blo[:, 1] < y0 + 8) & (bhi[:, 1] > y0)).sum())
        f = nsuper_xcd + (t // 8) * (per_super - 1)
        nclaimed = sum(1 for u in range(f, f + per_super - 1) if u >= RESIDENT_WAVES // 8)
        if t == s:
            assert ncand > K.kBwdList and nclaimed == per_super - 1
        may_take += nclaimed if ncand <= K.kBwdList else 0
    assert 0 < may_take <= claimed - (per_super - 1)
    return si, claimed, may_take


def wide_radius_scene(seed, P, H, W, D):
    """P Gaussians + the whole-grid one; a tenth of them isotropic with scales of 1 - 12 m: radii of 6 - 72 voxels, i.e. from one
    supertile to the whole of the tests' grids, next to the config's own radii of 1 - 4 voxels."""
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=seed, P=P, H=H, W=W, D=D)
    rng = np.random.default_rng(seed + 1000)
    wide = rng.choice(P, size=P // 10, replace=False)
    s = (1.0 + 11.0 * rng.random(len(wide))).astype(np.float32)
    si.scales[wide] = s[:, None]
    si.cov3D[wide] = (np.eye(3, dtype=np.float64)[None] / (s.astype(np.float64) ** 2)[:, None, None]).astype(np.float32)
    return si
