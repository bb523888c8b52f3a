"""The matrix-core render kernel (GF_MFMA_SPLAT: base variant, dense lattice, split-f16 MFMA with fp32 accumulation)
through the C ABI: same bound as the default kernel against the CPU oracle / the reference's own kernels (1e-4 scaled),
the device-side lattice check, and the fallbacks."""
import numpy as np
import pytest
import torch

import oracle
from gaussianformer_amd.synthetic import make_splat_inputs

from splat_cases import bwd, range_bounds, run_route, tensors, units, wave_equals_tile
from util import GRAD_RTOL, assert_grad_rows_close, assert_logits_close, hip_splat_forward, prep, print_grad_rows, whole_grid_rows

GRAD_NAMES = ("means3D_grad", "opacity_grad", "semantics_grad", "cov3D_grad")


def _rows_close(got, ref, whole, what):
    """Every Gaussian's gradient row against its own magnitude (tests/util.py), next to the tensor-wide bounds; printed."""
    print()
    for name, a, b in zip(GRAD_NAMES, got, ref):
        a, b = np.asarray(a), np.asarray(b)
        print_grad_rows(f"{name} [{what}]", assert_grad_rows_close(a, b.reshape(a.shape), whole, what=f"{name} [{what}]", rtol=GRAD_RTOL))

pytestmark = pytest.mark.gpu

SMALL = [
    # config, P, H, W, D
    ("nuscenes_gs25600_solid", 300, 24, 20, 16),
    ("nuscenes_gs25600_solid", 257, 23, 21, 16),   # H, W not multiples of the tile
    ("nuscenes_gs25600_solid", 200, 20, 20, 10),   # D not a multiple of 4: scalar row stores, upper brick partly outside
    ("nuscenes_gs25600_solid", 200, 20, 20, 40),   # several z groups per tile
    ("nuscenes_gs25600_solid", 90, 9, 7, 4),       # grid smaller than one double brick
    ("nuscenes_gs144000", 1000, 40, 44, 16),
    ("nuscenes_gs25600_solid", 0, 12, 12, 8),      # only the appended whole-grid Gaussian
]


def _oracle_logits(si, pi, mi, radii, cov6):
    return oracle.splat_forward(si.variant, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, si.H, si.W, si.D)["logits"]


def _reference_logits(si, pi, mi, radii, cov6):
    """The reference's own kernels when oracle/_ref is built, else the CPU oracle."""
    from oracle import ref as oref
    if oref.available():
        return oref.splat_forward("base", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, si.H, si.W, si.D)["logits"]
    return _oracle_logits(si, pi, mi, radii, cov6)


@pytest.mark.parametrize("config,P,H,W,D", SMALL)
def test_mfma_forward_small(gpu, config, P, H, W, D):
    from gaussianformer_amd import _lib
    si = make_splat_inputs(config, seed=3, P=P, H=H, W=W, D=D)
    pi, mi, radii, cov6 = prep(si)
    ref = _oracle_logits(si, pi, mi, radii, cov6)
    for flags in (_lib.GF_MFMA_SPLAT, _lib.GF_MFMA_SPLAT | _lib.GF_PTS_ASSUME_DENSE):
        got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=flags)
        assert_logits_close(got["logits"], ref, tol=1e-4)


def test_mfma_membership_is_exact(gpu):
    """Sigma^-1 = 0, opacity = semantics = 1: every covered voxel receives exactly 1 per covering Gaussian -- the box
    term of the exponent (0 inside, <= -32768 outside) and the split-f16 accumulation are exact on these values."""
    from gaussianformer_amd import _lib
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=6, P=2000, H=40, W=36, D=16)
    pi, mi, radii, cov6 = prep(si)
    si.opacities[:] = 1.0
    si.semantics[:] = 1.0
    cov6 = np.zeros_like(cov6)
    ref = _oracle_logits(si, pi, mi, radii, cov6)
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
    assert np.array_equal(got["logits"], ref)


def test_mfma_crowded_tile(gpu):
    """Thousands of Gaussians in one supertile: list refills, queue carried across them, many groups per wave."""
    from gaussianformer_amd import _lib
    si = make_splat_inputs("nuscenes_gs144000", seed=9, P=6000, H=20, W=20, D=16)
    pi, mi, radii, cov6 = prep(si)
    ref = _oracle_logits(si, pi, mi, radii, cov6)
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
    assert_logits_close(got["logits"], ref, tol=1e-4)


@pytest.mark.parametrize("config,kw", [
    ("nuscenes_gs25600_solid", {}),                                   # the headline shape: 401 bitmask words, ~165 candidates per supertile
    ("nuscenes_gs144000", dict(P=6000, H=20, W=20, D=16)),            # crowded: lists longer than the wave kernel's, refills
    ("nuscenes_gs25600_solid", dict(P=39000, H=44, W=36, D=24)),     # 610 words (nearly the longest row it takes), three z bricks
    ("nuscenes_gs25600_solid", dict(P=700, H=9, W=7, D=4)),          # one supertile column, one partial brick
    # round 6, long rows (kWRow < words <= 4096: the wave kernel's long-row instantiation -- summary, ranks, gathered words)
    ("nuscenes_gs144000", {}),                                        # BASELINE config [3]: 2 250 words, ~450 of them non-zero, one pass
    ("nuscenes_gs144000", dict(P=50000, H=24, W=24, D=16)),           # crowded: nine supertiles, every word non-zero: several passes
    ("nuscenes_gs25600_solid", dict(P=45000, H=9, W=7, D=4)),        # every bit set: the list fills inside a round (groups of eight words)
    ("nuscenes_gs144000", dict(P=40000, H=64, W=40, D=8)),            # just past kWRow (626 words), sparse rows
    ("nuscenes_gs144000", dict(P=262144, H=48, W=40, D=16)),          # the longest rows it takes (4 096 words)
])
def test_mfma_wave_and_tile_kernels_agree_bit_for_bit(gpu, config, kw):
    """The two matrix-core kernels -- one wave per double brick (rows of <= 618 words; longer rows, up to 4 096 words, in its
    long-row instantiation) and one workgroup per tile (the library option "splat.mfma_tile_kernel" forces it) -- take a double
    brick's hits in the same groups of 32 in ascending index and run the same
    arithmetic on them: equal bits, whatever path (fast fill, chunked refill, long-row passes) built the lists."""
    from gaussianformer_amd import _lib
    si = make_splat_inputs(config, seed=4, **kw)
    prepped = prep(si)
    t = tensors(gpu, si, prepped)
    wave = run_route(t, si, _lib.GF_MFMA_SPLAT)
    wave_equals_tile(wave, run_route(t, si, _lib.GF_MFMA_SPLAT, tile=True))
    assert_logits_close(wave[0], _oracle_logits(si, *prepped), tol=1e-4)


def test_mfma_inexact_lattice_falls_back(gpu):
    """pts one ulp off the lattice in a few voxels (still inside their voxels): the device-side check must notice -- the
    kernel evaluates its polynomial on the lattice, not on pts -- and the arbitrary-points body must produce the result
    for the positions actually given.  Anisotropic but exact steps are a lattice and stay on the matrix cores."""
    import torch
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import splat_forward
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=11, P=300, H=24, W=20, D=16)
    pi, mi, radii, cov6 = prep(si)
    rng = np.random.default_rng(1)
    pick = rng.choice(si.pts.shape[0], 50, replace=False)
    si.pts[pick, 0] = np.nextafter(si.pts[pick, 0], np.float32(1e9))
    ref = _oracle_logits(si, pi, mi, radii, cov6)          # the oracle reads pts: the perturbed positions
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6)]
    logits, _, _, _, state = splat_forward(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=_lib.GF_MFMA_SPLAT)
    # state block: the points ARE in their voxels (word 0 = 0, the backward keeps its dense path), the call was rendered
    # by the arbitrary-points body (word 1) because the lattice verdict (bit 1 of word 2) failed
    assert state.view(torch.int32)[:3].tolist() == [0, _lib.GF_PATH_ARBITRARY, _lib.GF_VERDICT_LATTICE]
    assert_logits_close(logits.cpu().numpy(), ref, tol=1e-4)
    # the thinnest Gaussians make one ulp visible: the result must be the one for the given positions, bit for bit the
    # arbitrary-points kernel's
    general, *_ = splat_forward(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=_lib.GF_PTS_GENERAL | _lib.GF_COMP_EXP)
    assert torch.equal(general, logits)


def test_mfma_coefficient_range_verdict(gpu):
    """A Gaussian whose exponent coefficients would leave the f16 range of the matrix-core kernel's operands (thin AND
    far-reaching: scale 0.004 m with a radius of 12 voxels) trips the prep launch's range verdict: the call is rendered
    by the arbitrary-points body (finite, within tolerance of the oracle) and the state block says so."""
    import torch
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import splat_forward
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=13, P=200, H=24, W=24, D=16)
    pi, mi, radii, cov6 = prep(si)
    cov6[5] = (np.float32(1.0 / 0.004 ** 2), np.float32(1.0), np.float32(1.0), 0, 0, 0)   # (xx, yy, zz, xy, yz, xz)
    radii[5] = 12
    ref = _oracle_logits(si, pi, mi, radii, cov6)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6)]
    logits, _, _, _, state = splat_forward(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D)
    assert state.view(torch.int32)[:3].tolist() == [0, _lib.GF_PATH_ARBITRARY, _lib.GF_VERDICT_THETA]
    assert bool(torch.isfinite(logits).all())
    assert_logits_close(logits.cpu().numpy(), ref, tol=1e-4)
    # with an ordinary covariance in its place the same call stays on the matrix cores
    cov6[5] = cov6[6]
    t[7] = torch.from_numpy(cov6).to(gpu)
    _, _, _, _, state = splat_forward(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D)
    assert state.view(torch.int32)[:3].tolist() == [0, _lib.GF_PATH_MATRIX_CORE_WAVE, 0]   # (a small P: the wave kernel)


@pytest.mark.parametrize("config", ["nuscenes_gs25600_solid", "nuscenes_gs144000"])
def test_mfma_forward_full_size(gpu, config):
    """BASELINE shapes: against the reference's own kernels when oracle/_ref is built, else the CPU oracle; linear in the
    semantics; deterministic."""
    from gaussianformer_amd import _lib
    si = make_splat_inputs(config, seed=0)
    pi, mi, radii, cov6 = prep(si)
    want = _reference_logits(si, pi, mi, radii, cov6)
    got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
    assert_logits_close(got["logits"], want, tol=1e-4)
    again, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
    assert np.array_equal(again["logits"], got["logits"])
    si.semantics *= np.float32(2.0)
    twice, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
    # (not bit-exact like the fp32 kernel: the low f16 halves of small operands are subnormal, where a factor 2 rounds anew)
    assert np.allclose(twice["logits"], np.float32(2.0) * got["logits"], rtol=2e-6, atol=1e-6)


def test_mfma_flag_is_ignored_where_it_does_not_apply(gpu):
    """prob variant and arbitrary points: the flag changes nothing."""
    from gaussianformer_amd import _lib
    si = make_splat_inputs("prob_gs6400", seed=3, P=120, H=24, W=20, D=16)
    pi, mi, radii, cov6 = prep(si)
    a, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    b, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=4, P=150, H=20, W=24, D=16, dense_pts=False, N=5000)
    pi, mi, radii, cov6 = prep(si)
    a, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    b, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
    assert np.array_equal(a["logits"], b["logits"])


def test_mfma_random_shapes_sweep(gpu):
    """Seeded sweep over grid shapes, Gaussian counts and scale ranges (thin and wide Gaussians, with and without the
    whole-grid one): the matrix-core kernel within the bound of the default one everywhere."""
    from gaussianformer_amd import _lib
    rng = np.random.default_rng(2024)
    worst = 0.0
    for it in range(10):
        H, W, D = int(rng.integers(5, 45)), int(rng.integers(5, 45)), int(rng.choice([4, 8, 12, 16, 24]))
        P = int(rng.integers(1, 1500))
        config = "nuscenes_gs144000" if it % 3 == 0 else "nuscenes_gs25600_solid"
        si = make_splat_inputs(config, seed=100 + it, P=P, H=H, W=W, D=D)
        pi, mi, radii, cov6 = prep(si)
        ref = _oracle_logits(si, pi, mi, radii, cov6)
        got, *_ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
        assert_logits_close(got["logits"], ref, what=f"sweep {it} ({config}, P={P}, {H}x{W}x{D})", tol=1e-4)
        worst = max(worst, float((np.abs(got["logits"].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max()))
    assert worst <= 1e-4


def test_mfma_module_keyword_and_autograd(gpu):
    """``LocalAggregator(..., matrix_cores=True)``: forward on the matrix cores, the same backward; gradients against the
    exact module on the same inputs."""
    import torch
    from gaussianformer_amd.local_aggregate import LocalAggregator
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=12, P=400, H=24, W=24, D=16)
    mods = [LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size, matrix_cores=mc).to(gpu)
            for mc in (False, True)]
    outs, grads = [], []
    for m in mods:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)[None]
        means, opa, sem, cov = (t(si.means3D).requires_grad_(True), t(si.opacities).requires_grad_(True),
                                t(si.semantics).requires_grad_(True), t(si.cov3D).requires_grad_(True))
        out = m(t(si.pts), means, opa, sem, t(si.scales), cov)
        g = torch.Generator(device="cpu").manual_seed(3)
        out.backward(torch.randn(out.shape, generator=g).to(gpu))
        outs.append(out.detach())
        grads.append([x.grad.clone() for x in (means, opa, sem, cov)])
    assert float(((outs[0] - outs[1]).abs() / outs[0].abs().clamp(min=1.0)).max()) <= 1e-4
    assert not torch.equal(outs[0], outs[1])                       # it really is the other kernel
    for a, b in zip(*grads):
        # the backward follows the forward: the exact Gaussian-major kernels after the exact forward, the voxel-major
        # matrix-core backward after the matrix-core forward (~1e-5 of the tensor's maximum apart; the bound against the
        # reference is 1e-3)
        assert float((a - b).abs().max()) <= 1e-4 * float(a.abs().max())
    _, mi, radii, _ = prep(si)
    _rows_close([x[0].cpu().numpy() for x in grads[1]], [x[0].cpu().numpy() for x in grads[0]],
                whole_grid_rows(mi, radii, si.H, si.W, si.D), "matrix-core module vs exact module")


# ---- round 4: the verdicts of the records pass (every call) and inputs at the edge of what stays on the matrix cores

def _run(gpu, si, pi, mi, radii, cov6, flags=0):
    """splat_cases.run_route on fresh tensors: (logits, [not-dense flag, GF_PATH_*, verdict bits])."""
    logits, state = run_route(tensors(gpu, si, (pi, mi, radii, cov6)), si, flags)
    return logits, list(state[:3])


@pytest.mark.parametrize("assume_dense", [False, True])
def test_mfma_large_semantics_fall_back(gpu, assume_dense):
    """a large opacity * semantics must not reach the split-f16 operands (cvt_pkrtz saturates at 65 504, and long
    before that the 2^-24 absolute resolution of the f16 weights, multiplied by S', leaves the tolerance: measured 1.7e-3 at
    S' = 2.9e4).  The records pass flags |S'| >= 64 (verdict bit 3) on EVERY call -- GF_PTS_ASSUME_DENSE skips the point scans, not
    the range verdicts -- and the arbitrary-points body renders the call: default flags, against the
    reference's own kernels."""
    from gaussianformer_amd import _lib
    si = make_splat_inputs("nuscenes_gs144000", seed=21, P=500, H=32, W=24, D=16)
    pi, mi, radii, cov6 = prep(si)
    si.semantics *= np.float32(1e5)
    want = _reference_logits(si, pi, mi, radii, cov6)
    flags = _lib.GF_PTS_ASSUME_DENSE if assume_dense else 0
    got, state = _run(gpu, si, pi, mi, radii, cov6, flags)
    assert state == [0, _lib.GF_PATH_ARBITRARY, _lib.GF_VERDICT_OPASEM]
    assert_logits_close(got, want, tol=1e-4)
    # one Gaussian is enough, and so is a NaN
    si.semantics /= np.float32(1e5)
    si.semantics[123, 4] = np.float32(7e4)
    got, state = _run(gpu, si, pi, mi, radii, cov6, flags)
    assert state[1:] == [_lib.GF_PATH_ARBITRARY, _lib.GF_VERDICT_OPASEM]
    assert_logits_close(got, _reference_logits(si, pi, mi, radii, cov6), tol=1e-4)
    # ... and just inside the bound (|opacity * semantics| < 64) the call stays on the matrix cores, still within the tolerance
    si.opacities[123] = np.float32(1.0)
    si.semantics[123, 4] = np.float32(63.0)
    got, state = _run(gpu, si, pi, mi, radii, cov6, flags)
    assert state == [0, _lib.GF_PATH_MATRIX_CORE_WAVE, 0]
    assert_logits_close(got, _reference_logits(si, pi, mi, radii, cov6), tol=1e-4)


def test_mfma_coefficient_range_verdict_under_assume_dense(gpu):
    """the theta range depends on each frame's covariances and radii, so GF_PTS_ASSUME_DENSE must not
    skip it: a thin, far-reaching Gaussian still sends the call to the arbitrary-points body (bit 2)."""
    from gaussianformer_amd import _lib
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=13, P=200, H=24, W=24, D=16)
    pi, mi, radii, cov6 = prep(si)
    cov6[5] = (np.float32(1.0 / 0.004 ** 2), np.float32(1.0), np.float32(1.0), 0, 0, 0)
    radii[5] = 12
    got, state = _run(gpu, si, pi, mi, radii, cov6, _lib.GF_PTS_ASSUME_DENSE)
    assert state == [0, _lib.GF_PATH_ARBITRARY, _lib.GF_VERDICT_THETA]
    assert_logits_close(got, _reference_logits(si, pi, mi, radii, cov6), tol=1e-4)


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_mfma_adversarial_inputs_just_inside_the_verdicts(gpu, seed):
    """the default kernel's margin was measured on one seed of one distribution.  Here a third of the Gaussians
    sit JUST INSIDE the records pass's accuracy verdict (0.72 (4.3 + sqrt Q)^2 in [900, 1190) -- thinner than anything the
    nuScenes configs produce: isotropic sigma down to 0.057 m, one thin axis down to 0.02 m), with rotated covariances and
    the largest radius the overflow bound admits, and the semantics span six orders of magnitude (x 1e-6 ... x 1, inside the
    |opacity * semantics| < 64 verdict).  The call must stay on the matrix cores and stay within 1e-4 (scaled) of the reference's own kernels."""
    from gaussianformer_amd import _lib
    rng = np.random.default_rng(seed)
    si = make_splat_inputs("nuscenes_gs144000" if seed % 2 else "nuscenes_gs25600_solid", seed=seed, P=900, H=40, W=32, D=16)
    pi, mi, radii, cov6 = prep(si)
    P = cov6.shape[0]
    pick = rng.choice(P - 1, P // 3, replace=False)          # (the last one may be the whole-grid Gaussian: left alone)
    for g in pick:
        s = rng.uniform(0.05, 1.0, 3)
        if rng.random() < 0.5:
            s[rng.integers(3)] = 0.02                          # one thin axis
        q = rng.standard_normal(4); q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        A = R @ np.diag(1.0 / s ** 2) @ R.T
        c = np.array([A[0, 0], A[1, 1], A[2, 2], A[0, 1], A[1, 2], A[0, 2]])
        _, near = range_bounds(c[None].astype(np.float32), np.array([1]), si.H, si.W, si.D)
        target = rng.uniform(900.0, 1190.0)
        # scale A so that the accuracy bound hits the target: sqrt(t Q) = sqrt(target / 0.7213) - 4.3
        sq_now = np.sqrt(near[0] / 0.7213475204444817) - 4.3
        t = ((np.sqrt(target / 0.7213475204444817) - 4.3) / sq_now) ** 2
        cov6[g] = (c * t).astype(np.float32)
        for r in (4, 3, 2, 1):
            b, n = range_bounds(cov6[g][None], np.array([r]), si.H, si.W, si.D)
            if b[0] < 2.9e4:
                break
        radii[g] = r
    b, n = range_bounds(cov6, radii, si.H, si.W, si.D)
    assert (b < 3e4).all() and (n < 1200).all() and (n[pick] > 880).all()
    scale = np.float32(10.0) ** rng.integers(-6, 1, size=(P, 1)).astype(np.float32)
    si.semantics = (si.semantics * scale).astype(np.float32)
    want = _reference_logits(si, pi, mi, radii, cov6)
    got, state = _run(gpu, si, pi, mi, radii, cov6)
    assert state == [0, _lib.GF_PATH_MATRIX_CORE_WAVE, 0], state
    assert_logits_close(got, want, tol=1e-4)
    # one step over the accuracy bound: the verdict notices and the call is still right
    g = int(pick[0])
    cov6[g] *= np.float32(2.0)
    assert range_bounds(cov6[g][None], radii[g:g + 1], si.H, si.W, si.D)[1][0] > 1200
    got, state = _run(gpu, si, pi, mi, radii, cov6)
    assert state == [0, _lib.GF_PATH_ARBITRARY, _lib.GF_VERDICT_THETA]
    assert_logits_close(got, _reference_logits(si, pi, mi, radii, cov6), tol=1e-4)


def test_mfma_very_thin_far_reaching_gaussians(gpu):
    """sigma = 0.01 m along one axis with radii of 12 and 20 voxels: far outside what the matrix-core operands carry -- the
    verdict sends the call to the exact body, which must agree with the reference (default flags)."""
    from gaussianformer_amd import _lib
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=41, P=300, H=48, W=40, D=16)
    pi, mi, radii, cov6 = prep(si)
    for g, r in ((3, 12), (77, 20), (150, 12)):
        cov6[g] = (np.float32(1e4), np.float32(4.0), np.float32(1.0), np.float32(3.0), 0, 0)
        radii[g] = r
    got, state = _run(gpu, si, pi, mi, radii, cov6)
    assert state == [0, _lib.GF_PATH_ARBITRARY, _lib.GF_VERDICT_THETA]
    assert_logits_close(got, _reference_logits(si, pi, mi, radii, cov6), tol=1e-4)


def test_registered_grid_skips_the_scan_and_keeps_the_verdicts(gpu):
    """``LocalAggregator.register_grid``: the verified tensor is rendered with GF_PTS_ASSUME_DENSE (same bits as the
    per-call verification), another tensor or a modified one is not, and the range verdicts still guard the call."""
    import torch
    from gaussianformer_amd.local_aggregate import LocalAggregator
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=12, P=400, H=24, W=24, D=16)
    agg = LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size).to(gpu)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)[None]
    pts = t(si.pts)
    args = (t(si.means3D), t(si.opacities), t(si.semantics), t(si.scales), t(si.cov3D))
    plain = agg(pts, *args)
    assert agg.register_grid(pts)
    assert agg._is_registered(pts.squeeze(0))
    fast = agg(pts, *args)
    assert torch.equal(plain, fast)
    other = pts.clone()
    assert not agg._is_registered(other.squeeze(0))
    pts[0, 5, 0] += 0.01                                         # modified in place: version counter moves on
    assert not agg._is_registered(pts.squeeze(0))
    shifted = t(si.pts + np.float32(0.01))                        # not the dense grid of this module's lattice verdict
    assert agg.register_grid(shifted) in (True, False)           # (either verdict is fine; the call must be right)
    again = agg(shifted, *args)
    assert torch.isfinite(again).all()


@pytest.mark.gpu
def test_backward_takes_the_forward_records_when_the_workspace_still_holds_them(gpu):
    """The forward's records pass lays out the matrix-core backward's rows; the backward repeats that pass only if the workspace
    has been used since (generation word, checked on the device).  Every combination gives the same bits: default flags after the
    forward (the pass stands down), after another call of a different shape has overwritten the workspace (the pass runs), twice
    in a row, and with GF_RECORDS_VALID (no pass launched)."""
    from gaussianformer_amd import _lib
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=21, P=1500, H=40, W=36, D=16)
    other = make_splat_inputs("nuscenes_gs25600_solid", seed=22, P=700, H=24, W=28, D=8)
    pi, mi, radii, cov6 = prep(si)
    g = np.random.default_rng(5).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    _, t, state0, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    assert not _lib.SplatState.of(state0).rows_ready                 # a forward that was not told of a backward prepares nothing
    plain = bwd(gpu, si, t, state0, g)
    _, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PREPARE_BACKWARD)
    words = _lib.SplatState.of(state)
    assert words.path == _lib.GF_PATH_MATRIX_CORE_WAVE and words.rows_ready
    base = bwd(gpu, si, t, state, g)                                    # records still there
    ref = oracle.splat_backward("base", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, si.H, si.W, si.D, g)
    for a, b in zip(base, ref):
        assert np.abs(a - b.reshape(a.shape)).max() <= 1e-4 * max(np.abs(b).max(), 1e-30)
    _rows_close(base, ref, whole_grid_rows(mi, radii, si.H, si.W, si.D), "records of the forward, P=1500 40x36x16")
    again = bwd(gpu, si, t, state, g)                                   # a second backward of the same forward
    asserted = bwd(gpu, si, t, state, g, flags=_lib.GF_MFMA_SPLAT | _lib.GF_RECORDS_VALID)
    for a, b, c, d in zip(base, again, asserted, plain):
        assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)
    # another shape through the same workspace: its sections lie over this forward's records
    hip_splat_forward(gpu, other, *prep(other))
    redo = bwd(gpu, si, t, state, g)
    for a, b in zip(base, redo):
        assert np.array_equal(a, b)
    # ... and a caller who vouches for records that are gone gets NaN, not numbers
    hip_splat_forward(gpu, other, *prep(other))
    wrong = bwd(gpu, si, t, state, g, flags=_lib.GF_MFMA_SPLAT | _lib.GF_RECORDS_VALID)
    assert all(np.isnan(a).all() for a in wrong)
    # the exact pipeline of another shape uses the workspace too
    _, t2, state2, _ = hip_splat_forward(gpu, other, *prep(other), flags=_lib.GF_EXACT_FP32)
    _, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PREPARE_BACKWARD)
    g2 = np.random.default_rng(6).standard_normal((other.pts.shape[0], 18)).astype(np.float32)
    bwd(gpu, other, t2, state2, g2, flags=_lib.GF_EXACT_FP32)
    after = bwd(gpu, si, t, state, g)
    for a, b in zip(base, after):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2000, 16, 16, 8), (3000, 8, 8, 16), (700, 24, 16, 8)])
def test_backward_after_a_prepared_forward_on_a_grid_of_few_workgroups(gpu, shape):
    """the forward finishes the backward's row layout in workgroups 0 .. 63 of its render launch; a grid with fewer
    workgroups than that (a few supertiles) and more than 64 waves of Gaussians used to leave Gaussians without their first row and
    still say "prepared".  Such a call now prepares nothing (word 4 of the state block = 0) and the backward lays its rows out
    itself: gradients as the oracle's, equal bit for bit to those behind an unprepared forward."""
    from gaussianformer_amd import _lib
    P, H, W, D = shape
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=31, P=P, H=H, W=W, D=D)
    pi, mi, radii, cov6 = prep(si)
    g = np.random.default_rng(9).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    ref = oracle.splat_backward("base", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, si.H, si.W, si.D, g)
    outs = []
    for fflags in (0, _lib.GF_PREPARE_BACKWARD):
        _, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=fflags)
        words = _lib.SplatState.of(state)
        nwg = 8 * -(-units((H, W, D)) // 8)
        if fflags and nwg < 64:
            assert not words.rows_ready, words
        got = bwd(gpu, si, t, state, g)
        outs.append(got)
        for a, b in zip(got, ref):
            assert np.isfinite(a).all()
            assert np.abs(a - b.reshape(a.shape)).max() <= 2e-4 * max(np.abs(b).max(), 1e-30)
        _rows_close(got, ref, whole_grid_rows(mi, radii, H, W, D), f"few workgroups {shape}, forward flags {fflags}")
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["several_whole_grid", "buffer_full"])
def test_backward_rows_of_whole_grid_gaussians_and_of_a_full_buffer(gpu, case):
    """The row layout without atomics at its edges: Gaussians with more rows than one workgroup sums (648 double bricks each,
    summed by the workgroups past the Gaussian range), and a buffer that has no room for most waves' rows (those Gaussians fall
    back to atomics) -- many large Gaussians on a small grid."""
    from gaussianformer_amd.synthetic import cov_inverse
    if case == "several_whole_grid":
        si = make_splat_inputs("nuscenes_gs25600_solid", seed=23, P=20, H=72, W=72, D=16)
        si.scales[3] = si.scales[11] = 60.0   # (with the appended one: three whole-grid Gaussians, 1 944 of the 2 656 rows provided)
    else:
        si = make_splat_inputs("nuscenes_gs25600_solid", seed=24, P=900, H=72, W=72, D=16)
        si.scales[:-1] = np.maximum(si.scales[:-1], 2.5)   # boxes of ~ 30 voxels a side: > 100 rows per Gaussian, 16 provided
    quats = np.tile(np.array([[1.0, 0.0, 0.0, 0.0]]), (si.scales.shape[0], 1))
    si.cov3D = cov_inverse(si.scales, quats).astype(np.float32)
    pi, mi, radii, cov6 = prep(si)
    g = np.random.default_rng(7).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    from gaussianformer_amd import _lib
    ref = oracle.splat_backward("base", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, si.H, si.W, si.D, g)
    for fflags in (0, _lib.GF_PREPARE_BACKWARD):
        _, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=fflags)
        if fflags:   # the forward reports whether every row fitted
            assert _lib.SplatState.of(state).rows_ready == (case == "several_whole_grid")
        got = bwd(gpu, si, t, state, g)
        for a, b in zip(got, ref):
            assert np.isfinite(a).all()
            assert np.abs(a - b.reshape(a.shape)).max() <= 2e-4 * max(np.abs(b).max(), 1e-30)
        _rows_close(got, ref, whole_grid_rows(mi, radii, si.H, si.W, si.D), f"{case}, forward flags {fflags}")


@pytest.mark.gpu
def test_backward_when_a_supertile_has_more_candidates_than_a_published_list_holds(gpu):
    """GF_PREPARE_BACKWARD publishes every supertile's candidate list for the backward -- up to 256 entries.  Two thousand small
    Gaussians inside one 8 x 8 column patch: that supertile's list does not fit, the forward raises the "not published" word (the
    rows still fit, so the state block says "prepared"), and the backward scans the bitmask rows itself -- same gradients as
    without any preparation, and as the oracle's."""
    from gaussianformer_amd import _lib
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=25, P=2000, H=40, W=40, D=16)
    rng = np.random.default_rng(26)
    lo = np.asarray(si.pc_min, dtype=np.float64)
    # (cells 16..23 x 16..23: one supertile; all heights)
    si.means3D[:-1, 0] = (lo[0] + (16 + 8 * rng.random(2000)) * si.grid_size).astype(np.float32)
    si.means3D[:-1, 1] = (lo[1] + (16 + 8 * rng.random(2000)) * si.grid_size).astype(np.float32)
    pi, mi, radii, cov6 = prep(si)
    g = np.random.default_rng(27).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    ref = oracle.splat_backward("base", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, si.H, si.W, si.D, g)
    _, t, state0, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    plain = bwd(gpu, si, t, state0, g)
    _, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PREPARE_BACKWARD)
    words = _lib.SplatState.of(state)
    assert words.path == _lib.GF_PATH_MATRIX_CORE_WAVE and words.rows_ready
    got = bwd(gpu, si, t, state, g, flags=_lib.GF_MFMA_SPLAT | _lib.GF_RECORDS_VALID)
    for a, b, c in zip(got, plain, ref):
        assert np.isfinite(a).all() and np.array_equal(a, b)
        assert np.abs(a - c.reshape(a.shape)).max() <= 2e-4 * max(np.abs(c).max(), 1e-30)
    _rows_close(got, ref, whole_grid_rows(mi, radii, si.H, si.W, si.D), "unpublished candidate list, P=2000 40x40x16")


@pytest.mark.gpu
@pytest.mark.parametrize("config, kw", [
    ("nuscenes_gs144000", dict(P=50000, H=24, W=24, D=16)),           # crowded supertiles: several passes in the forward, nothing published
    ("nuscenes_gs144000", dict(P=40000, H=64, W=40, D=8)),            # 626 words: just past the short rows; lists published, in pieces
    ("nuscenes_gs144000", dict(P=60000, H=96, W=88, D=16)),           # lists of one to four pieces
    ("nuscenes_gs25600_solid", dict(P=45000, H=72, W=64, D=16)),      # large Gaussians: the rows do not fit the buffer (state word 4, bit 1)
    ("nuscenes_gs25600_solid", dict(P=45000, H=16, W=16, D=8)),       # a grid of few workgroups: nothing prepared, the backward lays out itself
])
def test_backward_on_long_rows(gpu, config, kw):
    """Round 6: the matrix-core backward on bitmask rows of more than 618 words (39 552 < P <= 262 144, BASELINE config [3]).  The
    forward's long-row instantiation publishes every supertile's whole one-pass list (up to 896 entries), the backward's units take
    it in pieces of 256; a supertile that went in several passes publishes nothing and its units read the row's words from memory.
    Row by row within 1e-3 of the exact Gaussian-major kernels (whose gradients are the reference's, test_ref_parity); the same
    bits with and without the forward's preparation."""
    from gaussianformer_amd import _lib
    from util import assert_grad_rows_close, whole_grid_rows
    si = make_splat_inputs(config, seed=3, **kw)
    pi, mi, radii, cov6 = prep(si)
    g = np.random.default_rng(1).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    _, t, state0, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    plain = bwd(gpu, si, t, state0, g)                                  # the backward lays its rows out itself, scans the rows
    exact = bwd(gpu, si, t, state0, g, flags=_lib.GF_EXACT_FP32)
    _, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PREPARE_BACKWARD)
    words = _lib.SplatState.of(state)
    assert not words.not_dense and words.path == _lib.GF_PATH_MATRIX_CORE_WAVE, words
    prepared = words.rows_ready
    assert prepared == (config == "nuscenes_gs144000"), words
    # "the rows do not fit": the module takes the Gaussian-major backward then
    assert words.rows_overflow == (not prepared and si.H > 16), words
    got = bwd(gpu, si, t, state, g, flags=(_lib.GF_MFMA_SPLAT | _lib.GF_RECORDS_VALID) if prepared else 0)
    for a, b, c, name in zip(got, plain, exact, ("means", "opacity", "semantics", "cov")):
        if prepared:   # (rows that do not fit are added with atomics, in no fixed order)
            assert np.array_equal(a, b), name
        assert_grad_rows_close(a, c.reshape(a.shape), whole, what=name)
        assert_grad_rows_close(b, c.reshape(b.shape), whole, what=name + " (unprepared)")


@pytest.mark.gpu
def test_forward_and_backward_past_the_longest_rows(gpu):
    """P > 262 144 (rows of more than 4 096 words): the tile kernel renders (matrix cores), nothing is prepared for a backward; the
    backward's documented limit is 262 144 Gaussians per call -- more is refused loudly, and a backward per shard of the set gives
    the rows (gradients are per Gaussian)."""
    from gaussianformer_amd import _lib
    si = make_splat_inputs("nuscenes_gs144000", seed=5, P=270000, H=48, W=40, D=8)
    pi, mi, radii, cov6 = prep(si)
    g = np.random.default_rng(2).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    exact_out, t, state_e, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_EXACT_FP32)
    out, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PREPARE_BACKWARD)
    words = _lib.SplatState.of(state)
    assert not words.not_dense and words.path == _lib.GF_PATH_MATRIX_CORE and not words.rows_ready and not words.rows_overflow, words
    assert np.abs(out["logits"] - exact_out["logits"]).max() <= 1e-4
    whole = bwd(gpu, si, t, state, g)          # the Python op shards the set for the C entry point (262 144 per call)
    from gaussianformer_amd.local_aggregate import BACKWARD_MAX_GAUSSIANS
    assert BACKWARD_MAX_GAUSSIANS < 270000 and all(np.isfinite(a).all() and a.shape[0] == 270000 for a in whole)
    # two shards of 135 000: the matrix-core backward (long rows) of each against the exact one
    import copy
    for lo, hi in ((0, 135000), (135000, 270000)):
        sh = copy.copy(si)
        sh.means3D, sh.opacities, sh.semantics, sh.scales, sh.cov3D = (a[lo:hi] for a in (si.means3D, si.opacities, si.semantics, si.scales, si.cov3D))
        spi, smi, sradii, scov6 = pi, mi[lo:hi], radii[lo:hi], cov6[lo:hi]
        _, ts, sts, _ = hip_splat_forward(gpu, sh, spi, smi, sradii, scov6, flags=_lib.GF_PREPARE_BACKWARD)
        ws = _lib.SplatState.of(sts)
        assert ws[1] == _lib.GF_PATH_MATRIX_CORE_WAVE, ws
        got = bwd(gpu, sh, ts, sts, g, flags=(_lib.GF_MFMA_SPLAT | _lib.GF_RECORDS_VALID) if ws.rows_ready else 0)
        ex = bwd(gpu, sh, ts, sts, g, flags=_lib.GF_EXACT_FP32)
        from util import assert_grad_rows_close
        for a, b, w, name in zip(got, ex, whole, ("means", "opacity", "semantics", "cov")):
            assert_grad_rows_close(a, b.reshape(a.shape), None, what=name)
            # the sharded op's rows are these rows (the exact kernels cut the concatenated boxes into wave ranges by the shard's total:
            # a box split elsewhere rounds elsewhere, so to rounding, not bit for bit)
            assert_grad_rows_close(w[lo:hi].reshape(a.shape), b.reshape(a.shape), None, what=name + " (sharded op)", rtol=2e-5)


@pytest.mark.gpu
def test_module_training_steps_with_two_aggregators_sharing_the_stream(gpu):
    """A few "training steps" through the autograd module, with a second aggregator call of another shape between a forward and its
    backward (it is handed the same workspace): the module's bookkeeping (workspace stamps, state words on the host) must pass
    GF_RECORDS_VALID only when nobody else used the workspace -- checked through the results, which have to match the exact
    module in every step either way."""
    from gaussianformer_amd.local_aggregate import LocalAggregator
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)[None]
    cfg = dict(P=500, H=32, W=24, D=16)
    other = make_splat_inputs("nuscenes_gs25600_solid", seed=40, P=300, H=16, W=16, D=8)
    m_other = LocalAggregator(other.scale_multiplier, other.H, other.W, other.D, list(other.pc_min), other.grid_size).to(gpu)
    for step in range(4):
        si = make_splat_inputs("nuscenes_gs25600_solid", seed=41 + step, **cfg)
        mods = [LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size, matrix_cores=mc).to(gpu)
                for mc in (False, True)]
        grads = []
        for k, m in enumerate(mods):
            leaves = [t(a).requires_grad_(True) for a in (si.means3D, si.opacities, si.semantics, si.cov3D)]
            out = m(t(si.pts), leaves[0], leaves[1], leaves[2], t(si.scales), leaves[3])
            if k == 1 and step % 2 == 1:   # someone else takes the stream's workspace between this forward and its backward
                with torch.no_grad():
                    m_other(t(other.pts), t(other.means3D), t(other.opacities), t(other.semantics), t(other.scales), t(other.cov3D))
            g = torch.Generator(device="cpu").manual_seed(50 + step)
            out.backward(torch.randn(out.shape, generator=g).to(gpu))
            grads.append([x.grad.clone() for x in leaves])
        for a, b in zip(*grads):
            assert torch.isfinite(b).all()
            assert float((a - b).abs().max()) <= 1e-4 * float(a.abs().max())


@pytest.mark.gpu
def test_forward_and_backward_are_reproducible_bit_for_bit_at_the_full_shape(gpu):
    """Ten forward + backward pairs of the nuScenes frame (matrix-core kernels, rows laid out by prefix sums, every sum in a fixed
    order): logits and the gradients of every Gaussian but the whole-grid one -- whose 64-row work items are combined with float
    atomics -- are equal bit for bit across runs."""
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import splat_backward, splat_forward
    from util import to_dev
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=0)
    pi, mi, radii, cov6 = prep(si)
    t = to_dev(gpu, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6)
    g = torch.randn(si.pts.shape[0], 18, generator=torch.Generator().manual_seed(1)).to(gpu)
    ref = None
    for _ in range(10):
        logits, _, _, _, state = splat_forward(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=_lib.GF_PREPARE_BACKWARD)
        out = splat_backward(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, g, state=state, flags=_lib.GF_MFMA_SPLAT | _lib.GF_RECORDS_VALID)
        cur = [logits.clone()] + [x[:-1].clone() for x in out]
        assert all(bool(torch.isfinite(x).all()) for x in cur)
        if ref is None:
            ref = cur
        else:
            assert all(torch.equal(a, b) for a, b in zip(cur, ref))


def test_product_library_is_not_a_development_build_and_reads_no_environment(gpu, monkeypatch):
    """Round 6: the library selects its kernels by arguments, flags and gf_set_option -- an environment variable
    of an earlier round changes nothing, a development option (the development build was removed after a5ba306) is refused."""
    from gaussianformer_amd import _lib
    assert not _lib.is_development_build()
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=3, P=800, H=24, W=24, D=16)
    pi, mi, radii, cov6 = prep(si)
    want, _, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    for k in ("GF_MFMA_TILE", "GF_MFMA_PAIR", "GF_MFMA_SOLO", "GF_FUSED", "GF_UNITS_BANDS", "GF_PREP_WAVES"):
        monkeypatch.setenv(k, "1")
    got, _, state2, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    assert _lib.SplatState.of(state2).path == _lib.GF_PATH_MATRIX_CORE_WAVE
    assert np.array_equal(got["logits"], want["logits"])
    with pytest.raises(RuntimeError):
        _lib.set_option("dev.splat_solo", 1)
    with pytest.raises(RuntimeError):
        _lib.set_option("no.such.option", 1)


def test_module_notices_a_dense_grid_that_is_not_its_lattice(gpu):
    """the module picks the matrix-core kernel from (pc_min, grid_size); a caller's dense ``pts`` built differently
    (here: a few centres one ulp off) fails the device verdict in every frame.  The module reads the state word back without
    waiting, warns once and switches itself to the exact-fp32 kernel."""
    import time
    import warnings
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import LocalAggregator
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=13, P=300, H=24, W=24, D=16)
    m = LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size).to(gpu)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)[None]
    pts = si.pts.copy()
    pts[::97, 1] = np.nextafter(pts[::97, 1], np.float32(1e9))
    args = (t(pts), t(si.means3D), t(si.opacities), t(si.semantics), t(si.scales), t(si.cov3D))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        first = m(*args)
        assert _lib.SplatState.of(m.last_state).path == _lib.GF_PATH_ARBITRARY
        torch.cuda.synchronize()
        time.sleep(0.05)
        for _ in range(3):
            out = m(*args)
        torch.cuda.synchronize()
    assert m._grid_exact is False and any("exact-fp32" in str(w.message) for w in caught)
    assert _lib.SplatState.of(m.last_state).path == _lib.GF_PATH_EXACT_TILE
    assert float(((out - first).abs() / first.abs().clamp(min=1.0)).max()) <= 1e-4
    # the module's own lattice is left alone
    m2 = LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size).to(gpu)
    for _ in range(4):
        m2(t(si.pts), *args[1:])
        torch.cuda.synchronize()
    assert m2._grid_exact is True


def test_module_keeps_the_voxel_indices_of_the_last_grid_tensor(gpu):
    """``points_int`` is recomputed only when the ``pts`` tensor changes (storage, shape or version counter): the second frame
    on the same grid tensor reuses it, an in-place edit or a new tensor does not."""
    from gaussianformer_amd.local_aggregate import LocalAggregator
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=14, P=300, H=24, W=24, D=16)
    m = LocalAggregator(si.scale_multiplier, si.H, si.W, si.D, list(si.pc_min), si.grid_size).to(gpu)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)[None]
    pts = t(si.pts)
    rest = (t(si.means3D), t(si.opacities), t(si.semantics), t(si.scales), t(si.cov3D))
    first = m(pts, *rest)
    kept = m._points_int_cache[2]
    again = m(pts, *rest)
    assert m._points_int_cache[2] is kept and torch.equal(first, again)
    pts2 = pts.clone()
    other = m(pts2, *rest)
    assert m._points_int_cache[2] is not kept and torch.equal(other, first)
    kept2 = m._points_int_cache[2]
    pts2[0, 0, 0] += 0.0   # an in-place write bumps the version counter: the indices are recomputed
    m(pts2, *rest)
    assert m._points_int_cache[2] is not kept2
    ref = ((pts2.squeeze(0) - m.pc_min) / m.grid_size).to(torch.int)
    assert torch.equal(m._points_int_cache[2], ref)


@pytest.mark.parametrize("assume_dense", [False, True])
def test_one_verdict_word_follows_the_inputs_call_after_call(gpu, assume_dense):
    """Round 6: on a workspace that was handed over zeroed (GF_WORKSPACE_ZEROED; SplatForwardPlan) the wave kernel reads ONE verdict
    word -- a double-buffered block [A, B, V0, V1] kept on the device -- instead of every prep wave's word.  The verdict has to follow
    the inputs call after call on the SAME workspace: violation (range bit 3) -> benign -> violation (theta, bit 2) -> benign ->
    a pts tensor that is not the lattice (bit 1, with the scans on) -> benign; twice in a row each, so that both parities of the
    block see both outcomes; every result against the exact-fp32 kernel on a workspace of its own."""
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import SplatForwardPlan
    from util import to_dev
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=77, P=600, H=32, W=24, D=16)
    pi, mi, radii, cov6 = prep(si)
    t = to_dev(gpu, si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6)
    base = _lib.GF_PTS_ASSUME_DENSE if assume_dense else 0
    plan = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=base)
    exact = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=base | _lib.GF_EXACT_FP32)
    pts, sem, cov, rad = t[0], t[5], t[7], t[6]
    sem0, cov0, rad0, pts0 = sem.clone(), cov.clone(), rad.clone(), pts.clone()

    def step(path, bits):
        got = plan.run().clone()
        torch.cuda.synchronize()
        assert plan.state_words()[1:3] == [path, bits], (plan.state_words()[:3], path, bits)
        want = exact.run()
        assert_logits_close(got.cpu().numpy(), want.cpu().numpy(), tol=1e-4)

    wave, arb = _lib.GF_PATH_MATRIX_CORE_WAVE, _lib.GF_PATH_ARBITRARY
    lattice, theta, opasem = _lib.GF_VERDICT_LATTICE, _lib.GF_VERDICT_THETA, _lib.GF_VERDICT_OPASEM
    for _ in range(2):
        step(wave, 0)
    sem[17, 3] = 7e4                                        # |opacity * semantics| >= 64
    for _ in range(2):
        step(arb, opasem)
    sem.copy_(sem0)
    for _ in range(3):
        step(wave, 0)
    cov[5] = torch.tensor([1.0 / 0.004 ** 2, 1.0, 1.0, 0, 0, 0], device=gpu)   # theta out of range
    rad[5] = 12
    step(arb, theta)
    sem[40, 0] = 9e4                                        # both at once
    step(arb, theta | opasem)
    cov.copy_(cov0); rad.copy_(rad0); sem.copy_(sem0)
    step(wave, 0)
    if not assume_dense:
        pts[1000, 2] += 1e-3                                # not the exact lattice any more (the point is still in its voxel)
        for _ in range(2):
            step(arb, lattice)
        pts.copy_(pts0)
        for _ in range(2):
            step(wave, 0)
    # the same under HIP-graph replay: the block's state lives on the device
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.run(); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.run(stream=s.cuda_stream)
    for poison in (False, True, True, False, False):
        sem.copy_(sem0)
        if poison:
            sem[17, 3] = 7e4
        g.replay()
        torch.cuda.synchronize()
        assert plan.state_words()[1:3] == ([arb, opasem] if poison else [wave, 0]), (poison, plan.state_words()[:3])
        assert_logits_close(plan.logits.cpu().numpy(), exact.run().cpu().numpy(), tol=1e-4)


def _list_builder_scene(side=16):
    """Grid side x side x 8 (16: four supertiles, one z brick; 32: the same Gaussians in the same places, twelve more supertiles
    that hold the whole-grid Gaussian alone), 16 000 Gaussians (250 bitmask words: 15 999 + the whole-grid one, which is
    bit 63 of word 249 in every row), all of radius 1 (scales 0.08 .. 0.16 m, boxes of three voxels a side, kept inside their
    supertile).  Supertile (0, 0): Gaussians 64 k, k < 230 -- 231 non-zero words of one bit each: more than 192 and at most 256, the
    fast path's loop branch in both kernels.  Supertile (0, 1): Gaussians 64 k + 1, k < 40 -- 41 non-zero words, the three-round
    branch.  Supertile (1, 1): all the others, ~15 700 -- every word dense, every 64-word chunk holds ~4 000 candidates: the chunked
    fill goes in by lane groups and `sg` carries over between passes.  Supertile (1, 0): the whole-grid Gaussian alone.
    Semantics are softplus (positive: sums of thousands of terms without cancellation) and opacities uniform, as the config draws
    them; nothing had to be thinned for the oracle bounds."""
    from gaussianformer_amd.synthetic import cov_inverse
    P = 15999
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=41, P=P, H=side, W=side, D=8)
    rng = np.random.default_rng(42)
    lo = np.asarray(si.pc_min, dtype=np.float64)
    idx = np.arange(P)
    sparse = (idx % 64 == 0) & (idx < 64 * 230)
    few = (idx % 64 == 1) & (idx < 64 * 40)
    x0 = np.where(sparse | few, 0.0, 8.0)
    y0 = np.where(sparse, 0.0, 8.0)
    # centre cells 2 .. 5 of the supertile: the box of radius 1 stays inside it
    si.means3D[:-1, 0] = (lo[0] + (x0 + 2.0 + 4.0 * rng.random(P)) * si.grid_size).astype(np.float32)
    si.means3D[:-1, 1] = (lo[1] + (y0 + 2.0 + 4.0 * rng.random(P)) * si.grid_size).astype(np.float32)
    si.scales[:-1] = (0.08 + 0.08 * rng.random((P, 3))).astype(np.float32)
    quats = np.tile(np.array([[1.0, 0.0, 0.0, 0.0]]), (si.scales.shape[0], 1))
    si.cov3D = cov_inverse(si.scales, quats).astype(np.float32)
    return si


@pytest.mark.parametrize("side", [16, 32])
def test_list_builder_regimes_agree_across_kernels_and_with_the_oracle(gpu, side):
    """One small scene (_list_builder_scene) takes the candidate-list code of the wave kernel and of the matrix-core backward --
    the same text in both, kept in each kernel -- through all its regimes: three rounds side by side (<= 192 non-zero words), the
    loop branch (231 words), and the chunked fill by lane groups with `sg` carried between passes.  Wave and tile kernel give equal
    bits; the backward behind a plain forward, behind a GF_PREPARE_BACKWARD forward and with GF_RECORDS_VALID gives equal bits;
    both meet the oracle at the bounds of test_mfma_crowded_tile (1e-4 scaled) and of
    test_backward_when_a_supertile_has_more_candidates_than_a_published_list_holds (2e-4 of the largest gradient).
    GF_RECORDS_VALID may only be asserted behind a forward that says "prepared" (word 4 of the state block; the library answers
    NaN otherwise, test_backward_takes_the_forward_records_when_the_workspace_still_holds_them).  At 16 x 16 x 8 the render launch
    has 16 workgroups, fewer than the 64 that finish the row layout of 250 waves of Gaussians, so that forward prepares nothing
    (test_backward_after_a_prepared_forward_on_a_grid_of_few_workgroups) and the third backward cannot be asked for; side = 32
    puts the same Gaussians on a grid of 64 units, where it is prepared and all three are compared.
    Measured on an MI355X at side 16: forward 9.5e-6 scaled, gradients 9.3e-6 of the largest."""
    from gaussianformer_amd import _lib
    si = _list_builder_scene(side)
    pi, mi, radii, cov6 = prep(si)
    assert si.means3D.shape[0] == 16000 and (radii[:-1] == 1).all()
    wave, t, state0, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
    assert _lib.SplatState.of(state0).path == _lib.GF_PATH_MATRIX_CORE_WAVE   # (otherwise the scene fell back and proved nothing)
    with _lib.option("splat.mfma_tile_kernel", 1):
        tile, _, tstate, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
    assert _lib.SplatState.of(tstate).path == _lib.GF_PATH_MATRIX_CORE
    assert np.array_equal(wave["logits"], tile["logits"])
    ref = _oracle_logits(si, pi, mi, radii, cov6)
    err = np.abs(wave["logits"].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    print("forward: max scaled error", err.max(), "max |logit|", np.abs(ref).max())
    assert_logits_close(wave["logits"], ref, tol=1e-4)

    g = np.random.default_rng(43).standard_normal((si.pts.shape[0], 18)).astype(np.float32)
    gref = oracle.splat_backward("base", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, si.H, si.W, si.D, g)
    _, t, state0, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6)
    assert _lib.SplatState.of(state0).path == _lib.GF_PATH_MATRIX_CORE_WAVE
    plain = bwd(gpu, si, t, state0, g)
    _, t, state, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_PREPARE_BACKWARD)
    words = _lib.SplatState.of(state)
    print("prepared forward: state words", words)
    assert words.path == _lib.GF_PATH_MATRIX_CORE_WAVE
    assert words.rows_ready == (side == 32)
    prepared = bwd(gpu, si, t, state, g)
    asserted = bwd(gpu, si, t, state, g, flags=_lib.GF_MFMA_SPLAT | _lib.GF_RECORDS_VALID) if words.rows_ready else prepared
    for a, b, c, r in zip(plain, prepared, asserted, gref):
        print("backward: max error / max |ref|", np.abs(a - r.reshape(a.shape)).max() / max(np.abs(r).max(), 1e-30))
        assert np.isfinite(a).all()
        assert np.array_equal(a, b) and np.array_equal(a, c)
        assert np.abs(a - r.reshape(a.shape)).max() <= 2e-4 * max(np.abs(r).max(), 1e-30)
