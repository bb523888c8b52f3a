"""The splat forward that a backward will follow (GF_PREPARE_BACKWARD, what _LocalAggregate.forward passes whenever a gradient is
wanted) at every bitmask-row regime of the matrix-core kernels.  With the flag the wave kernel does two jobs: it renders, and its
workgroups 0..63 finish the backward's row layout in their LDS block (finish_row_layout / finish_row_layout_long).  The flag must
leave the logits alone -- the same bits as the plain forward and as the tile kernel, with and without it -- and the backward it
prepares must give the bits of an unprepared one.

nwords = ceil(P / 64) bitmask words per row, P = means3D.shape[0] (nuscenes_gs144000 appends no whole-grid Gaussian):

    618   the last short row: <false, true>, the whole row in LDS
    619   the first long row: <false, true, true, true>, summary + gathered words
    3968  the last long row whose row-layout prefix (LDS dwords [0, nwords)) stays below the prefetched summary row (kLSumAt)
    3969  the first row whose prefix reaches it: summary dword 0 (row words 0..15, Gaussians 0..1023)
    4096  the longest row the wave kernel takes: summary dwords 0..127 (Gaussians 0..131 071)
    4097  past it: the tile kernel renders, nothing is prepared

For nwords >= 3968 the inputs are built so that the Gaussians a reached summary dword covers overlap the first unit of every
workgroup 0..63 (test_clobber_cases_reach_the_first_units checks that on the CPU, from the integer boxes)."""
import numpy as np
import pytest
import torch

import oracle
from gaussianformer_amd.synthetic import make_splat_inputs

from splat_cases import K, bwd, integer_boxes
from util import assert_grad_rows_close, assert_logits_close, hip_splat_forward, prep, whole_grid_rows

CONFIG = "nuscenes_gs144000"
H, W, D = 48, 40, 16   # 30 supertiles x 8 units: a wave grid of 240 workgroups, so workgroups 0..63 exist and the layout is taken

CASES = [
    # name, P, nwords
    ("last_short_row", 39552, 618),
    ("first_long_row", 39553, 619),
    ("last_clean_long_row", 253952, 3968),
    ("first_clobbered_row", 253953, 3969),
    ("longest_row", 262144, 4096),
    ("past_the_longest_row", 262145, 4097),
]


def _nwords(si):
    return (si.means3D.shape[0] + 63) // 64


def first_units(H, W, D):
    """The first unit of workgroups 0..63 of the wave kernel (supertiles dealt to the XCDs round-robin, the default): workgroup b
    starts at unit b >> 3 of the XCD b & 7, i.e. unit r of supertile 8 q + (b & 7) with (q, r) = divmod(b >> 3, units per supertile)
    -- the mapping of gf_splat_render_mfma_wave_kernel's first-unit prefetch.  Returns per workgroup ((x0, x1), (y0, y1), (z0, z1))
    voxel ranges, or None where the workgroup has no first unit (no prefetched summary)."""
    nsx, nsy = -(-H // K.kSuper), -(-W // K.kSuper)
    per_super = 4 * ((D + 7) >> 3)
    per_xcd = ((nsx * nsy + 7) >> 3) * per_super
    out = []
    for b in range(K.kRowLayoutBlocks):
        local, xcd = b >> 3, b & 7
        q, r = divmod(local, per_super)
        s = 8 * q + xcd
        if local >= per_xcd or s >= nsx * nsy:
            out.append(None)
            continue
        srow, scol = divmod(s, nsy)
        x0, y0, z0 = srow * K.kSuper + 4 * (r & 1), scol * K.kSuper + 4 * ((r >> 1) & 1), 8 * (r >> 2)
        out.append(((x0, min(x0 + 4, H)), (y0, min(y0 + 4, W)), (z0, min(z0 + 8, D))) if x0 < H and y0 < W else None)
    return out


def reached_dwords(nwords):
    """Summary dwords that finish_row_layout_long's prefix covers at this row length (at 3968 words: the one the next word would
    reach).  Dword i covers row words 16 i .. 16 i + 15, i.e. Gaussians 1024 i .. 1024 i + 1023."""
    return range(max(1, min(nwords, K.kLongWords) - K.kLSumAt))


_inputs_cache, _oracle_cache = {}, {}


def case_inputs(P):
    """Seeded inputs of P Gaussians, built once per module.  From 3968 words on, Gaussians are moved into the first units of workgroups
    0..63: all 1024 of summary dword 0 (Gaussian g to unit g % 64: every unit then has a candidate in each of the dword's sixteen
    words), and of every further reached dword i the Gaussians 1024 i + 16 m, m = 0..63 (one per unit).  Each is centred in a voxel
    of its unit, so it contributes there."""
    if P not in _inputs_cache:
        si = make_splat_inputs(CONFIG, seed=4, P=P, H=H, W=W, D=D)
        nwords = _nwords(si)
        if nwords >= K.kLSumAt:
            rng = np.random.default_rng(8)
            units = first_units(H, W, D)
            assert all(u is not None for u in units)
            lo, gs = np.asarray(si.pc_min, dtype=np.float64), si.grid_size
            for i in reached_dwords(nwords):
                gids = np.arange(1024) if i == 0 else 1024 * i + 16 * np.arange(64)
                for g in gids:
                    (x0, x1), (y0, y1), (z0, z1) = units[g % 64]
                    v = np.array([rng.integers(x0, x1), rng.integers(y0, y1), rng.integers(z0, z1)], dtype=np.float64)
                    si.means3D[g] = (lo + (v + 0.5 + rng.uniform(-0.25, 0.25, 3)) * gs).astype(np.float32)
        _inputs_cache[P] = (si,) + tuple(prep(si))
    return _inputs_cache[P]


def case_oracle(P):
    if P not in _oracle_cache:
        si, pi, mi, radii, cov6 = case_inputs(P)
        _oracle_cache[P] = oracle.splat_forward(si.variant, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6,
                                                   si.H, si.W, si.D)["logits"]
    return _oracle_cache[P]


@pytest.mark.parametrize("name,P,nwords", [c for c in CASES if c[2] >= K.kLSumAt], ids=lambda v: str(v))
def test_clobber_cases_reach_the_first_units(name, P, nwords):
    """CPU: the inputs of the long-row cases from 3968 words on are sensitive to a summary row that the row-layout prefix
    overwrites.  Every workgroup 0..63 has a first unit, and it has candidates (integer box meets the unit's voxels) in all sixteen
    row words of summary dword 0 and among the Gaussians of every further reached dword."""
    si, pi, mi, radii, cov6 = case_inputs(P)
    assert _nwords(si) == nwords
    lo, hi = integer_boxes(mi, radii, si.H, si.W, si.D)
    nsuper = -(-si.H // K.kSuper) * -(-si.W // K.kSuper)
    assert nsuper * 4 * ((si.D + 7) >> 3) >= K.kRowLayoutBlocks   # units: a wave grid of >= 64 workgroups (layout_ok)
    for b, u in enumerate(first_units(si.H, si.W, si.D)):
        assert u is not None, b
        meets = np.ones(lo.shape[0], bool)
        for a, (u0, u1) in enumerate(u):
            meets &= (lo[:, a] < u1) & (hi[:, a] > u0)
        cand = np.flatnonzero(meets)
        words0 = np.unique(cand[cand < 1024] // 64)
        assert np.array_equal(words0, np.arange(16)), (b, u, words0)
        for i in reached_dwords(nwords):
            assert ((cand >= 1024 * i) & (cand < 1024 * (i + 1))).any(), (b, u, i)


def _words(state):
    from gaussianformer_amd import _lib
    return _lib.SplatState.of(state)


@pytest.mark.gpu
@pytest.mark.parametrize("name,P,nwords", CASES, ids=lambda v: str(v))
def test_prepared_forward_and_backward_at_row_regime(gpu, name, P, nwords):
    """The prepared forward's logits equal, bit for bit, the plain forward's and the tile kernel's (with and without the flag), and
    are within 1e-4 scaled of the oracle; the state block reports the wave kernel and the preparation.  The backward on the
    prepared state (GF_MFMA_SPLAT | GF_RECORDS_VALID) equals the backward after an unprepared forward, bit for bit, and both are
    within 1e-3 of the exact kernels row by row.  A forward the tile kernel renders with GF_PREPARE_BACKWARD, followed by the
    backward the autograd op chooses, is within the same bound."""
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import _LocalAggregate
    si, pi, mi, radii, cov6 = case_inputs(P)
    assert _nwords(si) == nwords
    on_wave = nwords <= K.kLongWords
    g = np.random.default_rng(1).standard_normal((si.pts.shape[0], 18)).astype(np.float32)

    prepared, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PREPARE_BACKWARD)
    words = _words(state)
    assert not words.not_dense, words
    if on_wave:
        assert words.path == _lib.GF_PATH_MATRIX_CORE_WAVE and words.rows_ready and not words.rows_overflow, words
        # (right after its forward: the workspace still holds the records and the layout)
        got = bwd(gpu, si, t, state, g, flags=_lib.GF_MFMA_SPLAT | _lib.GF_RECORDS_VALID)
    else:
        assert words.path == _lib.GF_PATH_MATRIX_CORE and not words.rows_ready and not words.rows_overflow, words

    plain, t0, state0, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    words0 = _words(state0)
    assert not words0.not_dense and words0.path == (_lib.GF_PATH_MATRIX_CORE_WAVE if on_wave else _lib.GF_PATH_MATRIX_CORE), words0
    assert not words0.rows_ready and not words0.rows_overflow, words0
    if on_wave:
        unprepared = bwd(gpu, si, t0, state0, g, flags=_lib.GF_MFMA_SPLAT)
        exact = bwd(gpu, si, t0, state0, g, flags=_lib.GF_EXACT_FP32)

    with _lib.option("splat.mfma_tile_kernel", 1):
        tile_p, _, tstate_p, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PREPARE_BACKWARD)
        tile, _, tstate, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    for tw in (_words(tstate_p), _words(tstate)):
        assert not tw.not_dense and tw.path == _lib.GF_PATH_MATRIX_CORE, tw

    assert np.isfinite(prepared["logits"]).all()
    for other, what in ((plain, "plain forward"), (tile_p, "tile kernel, prepared"), (tile, "tile kernel")):
        diff = prepared["logits"] != other["logits"]
        assert not diff.any(), (f"{name}: prepared forward vs {what}: {int(diff.any(axis=1).sum())} voxels differ, "
                                f"max |diff| {np.abs(prepared['logits'] - other['logits']).max():.3e}")
    assert_logits_close(prepared["logits"], case_oracle(P), tol=1e-4)

    if not on_wave:
        return
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    names = ("means", "opacity", "semantics", "cov")
    for a, b, c, what in zip(got, unprepared, exact, names):
        assert np.isfinite(a).all() and np.array_equal(a, b), what
        assert_grad_rows_close(a, c.reshape(a.shape), whole, what=what)
        assert_grad_rows_close(b, c.reshape(b.shape), whole, what=what + " (unprepared)")
    if name == "first_long_row":   # (small enough for the CPU oracle's backward: the chain ends at an independent reference)
        ref = oracle.splat_backward("base", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, si.H, si.W, si.D, g)
        for a, c, what in zip(got, ref, names):
            assert_grad_rows_close(a, c.reshape(a.shape), whole, what=what + " (oracle)")

    # the tile kernel with GF_PREPARE_BACKWARD, then whichever backward the autograd op picks from the state words
    pts, pts_int, means, means_int, opa, sem, rad, cov = t
    leaves = [x.clone().requires_grad_(True) for x in (means, opa, sem, cov)]
    with _lib.option("splat.mfma_tile_kernel", 1):
        out = _LocalAggregate.apply(pts, pts_int, leaves[0], means_int, leaves[1], leaves[2], rad, leaves[3], si.H, si.W, si.D)
        torch.cuda.synchronize(gpu)   # (the op reads the state words on the host when they have landed)
        out.backward(torch.from_numpy(g).to(gpu))
    assert np.array_equal(out.detach().cpu().numpy(), tile_p["logits"])
    for x, c, what in zip(leaves, exact, names):
        a = x.grad.cpu().numpy()
        assert_grad_rows_close(a, c.reshape(a.shape), whole, what=what + " (tile kernel, prepared)")


@pytest.mark.gpu
def test_module_training_step_at_the_longest_rows(gpu):
    """LocalAggregator with tensors that require grad, on 262 000 Gaussians (4 094 words, inside the range where the row-layout
    prefix reaches the prefetched summary row; inputs built as for the clobber cases): the logits equal, bit for bit, those of the
    same module under torch.no_grad() (nothing prepared), and the gradients are within 1e-3 row by row of the exact-fp32 module's."""
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import LocalAggregator
    si, _, mi, radii, _ = case_inputs(262000)
    assert K.kLSumAt < _nwords(si) <= K.kLongWords
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)[None]
    mk = lambda mc: LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size, matrix_cores=mc).to(gpu)
    g = torch.from_numpy(np.random.default_rng(3).standard_normal((si.pts.shape[0], 18)).astype(np.float32)).to(gpu)

    m = mk(None)
    with torch.no_grad():
        ref = m(dev(si.pts), dev(si.means3D), dev(si.opacities), dev(si.semantics), dev(si.scales), dev(si.cov3D))
    words = _words(m.last_state)
    assert not words.rows_ready and not words.rows_overflow
    grads = []
    for mod in (m, mk(False)):
        leaves = [dev(a).requires_grad_(True) for a in (si.means3D, si.opacities, si.semantics, si.cov3D)]
        out = mod(dev(si.pts), leaves[0], leaves[1], leaves[2], dev(si.scales), leaves[3])
        torch.cuda.synchronize(gpu)
        if mod is m:
            words = _words(mod.last_state)
            assert not words.not_dense and words.path == _lib.GF_PATH_MATRIX_CORE_WAVE and words.rows_ready and not words.rows_overflow, words
            diff = (out != ref).any(dim=-1)
            assert not bool(diff.any()), (f"prepared forward vs torch.no_grad(): {int(diff.sum())} voxels differ, "
                                          f"max |diff| {float((out - ref).abs().max()):.3e}")
        out.backward(g.reshape(out.shape))
        grads.append([x.grad[0].cpu().numpy() for x in leaves])
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    for a, c, what in zip(*grads, ("means", "opacity", "semantics", "cov3D")):
        assert_grad_rows_close(a, c, whole, what=what)
