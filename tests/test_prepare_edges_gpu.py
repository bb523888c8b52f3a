"""The splat's integer path and Sigma^-1 at cell, ceil and scale edges, on the device.

Every splat call starts from the integer cell ``means3D_int``, the integer radius ``radii`` and the packed Sigma^-1 of each
Gaussian.  The project computes them on three routes that must be one function: the checker
(``oracle.prepare_splat_inputs``, pinned to the reference's expression by tests/test_prepare_edges.py), the fused kernel
(``gf_gaussian_prepare``) and the torch expressions of the ``LocalAggregator*`` modules, which run on the device.  The
inputs (tests/prepare_edges.py) sit on the cell faces and the ceil steps, where a division that is not correctly rounded
moves a Gaussian's whole box, and at the ends of the conditioning range of the prob configs.

Each test prints the figures it judges (``pytest -s``); profiles/prepare_edges.txt records them.
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import prepare_edges as pe
from test_prepare_edges import (CELL_IDS, VALUE_BOUND, cotangent, grad_ratios, truth_fp64, value_ratio)

pytestmark = pytest.mark.gpu

H, W, D = pe.GRID
# (radii_mode name, radii_min of the kernel, per_axis / radii_min of the checker)
RADII_MODES = [("GF_RADII_SCALAR", 1, False, None), ("GF_RADII_SCALAR_CLAMPED", 1, False, 1),
               ("GF_RADII_SCALAR_CLAMPED", 4, False, 4), ("GF_RADII_PER_AXIS", 1, True, 1), ("GF_RADII_PER_AXIS", 4, True, 4)]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _identity_rot(P, dev):
    q = torch.zeros(P, 4, device=dev)
    q[:, 0] = 1.0
    return q


def _oracle(pts, means, scales, lo, g, m, per_axis, radii_min):
    cov = np.zeros((len(means), 3, 3), np.float32)
    pi, mi, radii, _ = oracle.prepare_splat_inputs(pts, means, scales, cov, list(lo), g, m, per_axis=per_axis, radii_min=radii_min)
    return pi, mi, radii


def _same(t, a):
    return t.dtype == torch.int32 and tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy(), a)


# ------------------------------------------------------------------ 3a: gf_gaussian_prepare
@pytest.mark.parametrize("g,lo", pe.CELLS, ids=CELL_IDS)
def test_gaussian_prepare_integers_on_faces_and_ceil_steps(gpu, g, lo):
    from gaussianformer_amd import _lib
    from gaussianformer_amd.gaussian_prepare import gaussian_prepare
    means = pe.boundary_means(lo, g, H, W, D)
    P = len(means)
    rot = _identity_rot(P, gpu)
    for m in pe.MULTIPLIERS:
        scales = pe.tile(pe.ceil_scales(g, m), P)
        for mode, rmin, per_axis, omin in RADII_MODES:
            mi, radii, _ = gaussian_prepare(_t(means, gpu), _t(scales, gpu), rot, list(lo), g, m, H, W, D,
                                            radii_mode=getattr(_lib, mode), radii_min=rmin)
            _, mi_ref, radii_ref = _oracle(means, means, scales, lo, g, m, per_axis, omin)
            assert _same(mi, mi_ref), f"means3D_int: {(mi.cpu().numpy() != mi_ref).sum()} components differ (m={m})"
            assert _same(radii, radii_ref), f"radii ({mode}, min {rmin}): {(radii.cpu().numpy() != radii_ref).sum()} differ (m={m})"


INT_GUARD, FLOAT_GUARD, GUARD_ROWS = -123456789, -7.0e33, 300


@pytest.mark.parametrize("g,lo", pe.CELLS, ids=CELL_IDS)
def test_gaussian_prepare_rows_do_not_depend_on_the_launch(gpu, g, lo):
    """The first P rows of a shorter call (one thread; one short of, exactly, one past a block) are the full call's rows, and
    nothing is written past row P of guard-padded outputs."""
    from gaussianformer_amd import _lib
    means = pe.boundary_means(lo, g, H, W, D)
    full = len(means)
    m = 3
    scales = pe.tile(pe.ceil_scales(g, m), full)
    means_t, scales_t, rot = _t(means, gpu), _t(scales, gpu), _identity_rot(full, gpu)
    pc = (ctypes.c_float * 3)(*lo)

    def run(P, mode, rmin):
        per_axis = mode == "GF_RADII_PER_AXIS"
        rows = P + GUARD_ROWS
        mi = torch.full((rows, 3), INT_GUARD, dtype=torch.int32, device=gpu)
        radii = torch.full((rows, 3) if per_axis else (rows,), INT_GUARD, dtype=torch.int32, device=gpu)
        cov = torch.full((rows, 6), FLOAT_GUARD, dtype=torch.float32, device=gpu)
        _lib.call("gf_gaussian_prepare", gpu, P, H, W, D, ctypes.cast(pc, ctypes.c_void_p), float(g), float(m),
                  getattr(_lib, mode), rmin, means_t, scales_t, rot, mi, radii, cov, None, None)
        for out, guard in ((mi, INT_GUARD), (radii, INT_GUARD), (cov, FLOAT_GUARD)):
            assert (out[P:] == guard).all(), f"P={P}: written past row P"
            assert (out[:P] != guard).all()
        return mi[:P], radii[:P], cov[:P]

    for mode, rmin, per_axis, omin in RADII_MODES:
        whole = run(full, mode, rmin)
        _, mi_ref, radii_ref = _oracle(means, means, scales, lo, g, m, per_axis, omin)
        assert _same(whole[0], mi_ref) and _same(whole[1], radii_ref)
        for P in (1, 255, 256, 257):
            for part, ref in zip(run(P, mode, rmin), whole):
                assert torch.equal(part, ref[:P]), f"P={P} ({mode})"


# ------------------------------------------------------------------ 3b: the modules' torch expressions
def _modules(lo, g, m, dims=pe.GRID, **kw):
    from gaussianformer_amd.local_aggregate import LocalAggregator, LocalAggregatorProb, LocalAggregatorProbFast
    return [("LocalAggregator", LocalAggregator(m, *dims, list(lo), g, **kw), False, None),
            ("LocalAggregatorProb/1", LocalAggregatorProb(m, *dims, list(lo), g, radii_min=1, **kw), False, 1),
            ("LocalAggregatorProb/4", LocalAggregatorProb(m, *dims, list(lo), g, radii_min=4, **kw), False, 4),
            ("LocalAggregatorProbFast/1", LocalAggregatorProbFast(m, *dims, list(lo), g, radii_min=1, **kw), True, 1),
            ("LocalAggregatorProbFast/4", LocalAggregatorProbFast(m, *dims, list(lo), g, radii_min=4, **kw), True, 4)]


def _host_scalar_cells(agg, x):
    """The expression the modules used before ``_cell_of``: a true division by the Python float on the device."""
    return ((x - agg.pc_min) / agg.grid_size).to(torch.int)


def _host_scalar_radii(agg, extent):
    return torch.ceil(extent * agg.scale_multiplier / agg.grid_size).to(torch.int)


@pytest.mark.parametrize("g,lo", pe.CELLS, ids=CELL_IDS)
def test_module_route_integers_on_faces_and_ceil_steps(gpu, g, lo):
    """``_prepare`` (means3D_int), ``_points_int`` (on a ``pts`` of the same face values) and ``_radii`` of the three modules
    equal the checker bit for bit on the device.  Also counts -- a figure, except on the 0.5 m cell where it must be zero --
    where a true division by the host scalar ``grid_size`` parts from the checker there (what the modules once evaluated)."""
    means = pe.boundary_means(lo, g, H, W, D)
    P = len(means)
    x = _t(means, gpu)
    sem, opa, cov = torch.zeros(1, P, 18, device=gpu), torch.zeros(1, P, device=gpu), torch.zeros(1, P, 3, 3, device=gpu)
    for m in pe.MULTIPLIERS:
        scales = pe.tile(pe.ceil_scales(g, m), P)
        s = _t(scales, gpu)
        for name, agg, per_axis, omin in _modules(lo, g, m, check_inputs=False):
            agg = agg.to(gpu)
            pi_ref, mi_ref, radii_ref = _oracle(means, means, scales, lo, g, m, per_axis, omin)
            if name == "LocalAggregator":
                old_cells = (_host_scalar_cells(agg, x).cpu().numpy() != mi_ref).sum()
                old_radii = (_host_scalar_radii(agg, s.max(dim=-1)[0]).cpu().numpy() != radii_ref).sum()
                old_axis = (_host_scalar_radii(agg, s).cpu().numpy()
                            != _oracle(means, means, scales, lo, g, m, True, None)[2]).sum()
                print(f"cell {g} m={m}: division by the host scalar on the device differs from the checker in {old_cells} of "
                      f"{3 * P} centre components, {old_radii} of {P} scalar radii, {old_axis} of {3 * P} per-axis radii")
                if g == 0.5:    # a power of two: x * 2 == x / 0.5 exactly
                    assert old_cells == 0 and old_radii == 0 and old_axis == 0
            out = agg._prepare(x[None], x[None], opa, sem, s[None], cov)
            assert _same(out[3], mi_ref), f"{name}: means3D_int differs in {(out[3].cpu().numpy() != mi_ref).sum()} components"
            assert _same(out[1], pi_ref) and _same(agg._points_int(x.clone()), pi_ref), name
            radii = agg._radii(s)
            assert _same(radii, radii_ref), f"{name}: {(radii.cpu().numpy() != radii_ref).sum()} radii differ (m={m})"


@pytest.mark.parametrize("g,lo", pe.CELLS, ids=CELL_IDS)
def test_cell_and_radius_helpers(gpu, g, lo):
    """``_cell_of`` -- also the cell expression of ``register_grid`` -- and ``_radius_of`` equal the checker on the device,
    wherever the module itself lies; the divisor is a 0-dim buffer that follows ``.to()`` and stays out of the ``state_dict``
    (the reference's).  On the 0.5 m cell they give the integers of the expression they replace: the product's bits are
    unchanged."""
    from gaussianformer_amd.local_aggregate import LocalAggregator
    m = 3
    means = pe.boundary_means(lo, g, H, W, D)
    scales = pe.tile(pe.ceil_scales(g, m), len(means))
    x, s = _t(means, gpu), _t(scales, gpu)
    agg = LocalAggregator(m, H, W, D, list(lo), g)
    assert list(agg.state_dict()) == ["pc_min"] and agg._cell.dim() == 0 and agg._cell.dtype == torch.float32
    assert agg._cell.item() == float(np.float32(g))
    _, mi_ref, radii_ref = _oracle(means, means, scales, lo, g, m, True, None)
    assert _same(agg._cell_of(x), mi_ref) and _same(agg._radius_of(s), radii_ref)      # the module still on the CPU
    agg = agg.to(gpu)
    assert agg._cell.device == x.device and list(agg.state_dict()) == ["pc_min"]
    assert _same(agg._cell_of(x), mi_ref) and _same(agg._radius_of(s), radii_ref)
    if g == 0.5:
        assert torch.equal(agg._cell_of(x), _host_scalar_cells(agg, x))
        assert torch.equal(agg._radius_of(s), _host_scalar_radii(agg, s))


def test_register_grid_keys_the_dense_grid(gpu):
    """``register_grid`` accepts the dense lattice of a 0.5 m cell and refuses it shifted by one voxel (its cell expression
    is ``_cell_of``); the grid of a 0.4 m cell is no exact lattice and is refused before that."""
    from gaussianformer_amd.local_aggregate import LocalAggregator
    dims, m = pe.SMALL_GRID, pe.SMALL_MULTIPLIER
    pts, _, _ = pe.end_to_end_case(pe.SMALL_PC_MIN, 0.5, *dims, m)
    agg = LocalAggregator(m, *dims, list(pe.SMALL_PC_MIN), 0.5).to(gpu)
    assert agg.register_grid(_t(pts, gpu)[None]) is True
    assert agg.register_grid(_t(pts + np.float32(0.5), gpu)[None]) is False
    pts4, _, _ = pe.end_to_end_case(pe.SMALL_PC_MIN, 0.4, *dims, m)
    assert LocalAggregator(m, *dims, list(pe.SMALL_PC_MIN), 0.4).to(gpu).register_grid(_t(pts4, gpu)[None]) is False


# ------------------------------------------------------------------ 3c: status bits and asserts agree
def _route2_bits(gpu, means, scales, lo, g, m, mode, rmin):
    from gaussianformer_amd import _lib
    from gaussianformer_amd.gaussian_prepare import gaussian_prepare
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    gaussian_prepare(_t(means, gpu), _t(scales, gpu), _identity_rot(len(means), gpu), list(lo), g, m, H, W, D,
                     radii_mode=getattr(_lib, mode), radii_min=rmin, status=status)
    return int(status.item())


def _route3_bits(gpu, agg, means, scales, pts):
    """The GF_PREPARE_* bits whose assert of the module fires (``check_inputs``): each condition is looked at on its own, as
    the reference's asserts stop at the first."""
    from gaussianformer_amd import _lib
    P = len(means)
    args = (_t(pts, gpu)[None], _t(means, gpu)[None], torch.zeros(1, P, device=gpu), torch.zeros(1, P, 18, device=gpu),
            _t(scales, gpu)[None], torch.zeros(1, P, 3, 3, device=gpu))
    out = agg._prepare(*args)
    violations, radii = out[-1], agg._radii(out[6])
    bits = 0
    assert not bool(violations[0]), "the query point is inside the grid"
    bits |= _lib.GF_PREPARE_MEAN_OUT_OF_GRID if bool(violations[1]) else 0
    bits |= _lib.GF_PREPARE_RADIUS_BELOW_ONE if bool((radii < 1).any()) else 0
    try:
        agg._splat_inputs(*args)
        fired = False
    except AssertionError:
        fired = True
    assert fired == (bits != 0)
    return bits


@pytest.mark.parametrize("g,lo", pe.CELLS, ids=CELL_IDS)
def test_status_bits_fire_exactly_when_the_module_asserts(gpu, g, lo):
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import LocalAggregator, LocalAggregatorProb
    m = 3
    OUT, BELOW = _lib.GF_PREPARE_MEAN_OUT_OF_GRID, _lib.GF_PREPARE_RADIUS_BELOW_ONE
    base = LocalAggregator(m, H, W, D, list(lo), g, check_inputs=True).to(gpu)
    prob = LocalAggregatorProb(m, H, W, D, list(lo), g, radii_min=1, check_inputs=True).to(gpu)
    pts = np.array([pe.mid_cell(lo, g, (H, W, D))], np.float32)      # one query point, mid-cell
    ordinary = lambda n: np.full((n, 3), 0.3, np.float32)
    below, above = pe.below_lower_face(lo, g, H, W, D), pe.upper_face(lo, g, H, W, D)
    on_face = pe.boundary_means(lo, g, H, W, D)
    on_face = on_face[(_oracle(on_face, on_face, ordinary(len(on_face)), lo, g, m, False, None)[1] >= np.array([H, W, D])).any(-1)]
    assert len(on_face) >= 3      # the upper face itself (and neighbours) of every axis: cell ``dim``
    cases = [("(lo - g, lo)", below, ordinary(len(below)), 0, 0),
             ("beyond the upper face", above, ordinary(len(above)), OUT, OUT),
             ("on the upper face", on_face, ordinary(len(on_face)), OUT, OUT),
             ("zero scale", pts, np.zeros((1, 3), np.float32), BELOW, 0)]
    for name, means, scales, want_scalar, want_clamped in cases:
        for agg, mode, want in ((base, "GF_RADII_SCALAR", want_scalar), (prob, "GF_RADII_SCALAR_CLAMPED", want_clamped)):
            r2 = _route2_bits(gpu, means, scales, lo, g, m, mode, 1)
            r3 = _route3_bits(gpu, agg, means, scales, pts)
            assert r2 == r3 == want, f"{name} ({mode}): kernel status {r2}, module asserts {r3}, expected {want}"


# ------------------------------------------------------------------ 3d: end to end, small
@pytest.mark.parametrize("g", [0.4, 0.5])
def test_forward_and_forward_from_rotations_agree_on_faces(gpu, g):
    """A third of the centres on cell faces, a third of the scales on ceil steps: ``forward`` (integers from the module's
    torch expressions, Sigma^-1 from GaussianArgs) and ``forward_from_rotations`` (everything from ``gf_gaussian_prepare``)
    render the same boxes -- ``torch.equal`` logits, gradients within the bound of
    tests/test_prepare.py::test_gaussian_args_module_and_fused_aggregator."""
    from gaussianformer_amd.gaussian_prepare import GaussianArgs
    from gaussianformer_amd.local_aggregate import LocalAggregator
    dims, lo, m = pe.SMALL_GRID, pe.SMALL_PC_MIN, pe.SMALL_MULTIPLIER
    pts_np, means_np, scales_np = pe.end_to_end_case(lo, g, *dims, m)
    P = len(means_np)
    rng = np.random.default_rng(4)
    pts, means, scales = _t(pts_np, gpu)[None], _t(means_np, gpu)[None], _t(scales_np, gpu)[None]
    rot = _t(rng.standard_normal((1, P, 4)).astype(np.float32), gpu)
    sem = _t(np.abs(rng.standard_normal((1, P, 18))).astype(np.float32), gpu)
    opa = _t(rng.random((1, P, 1)).astype(np.float32), gpu)
    args = GaussianArgs(num_classes=18).to(gpu)
    agg = LocalAggregator(m, *dims, list(lo), g, check_inputs=True, matrix_cores=False).to(gpu)

    def run(fused):
        leaves = [t.clone().requires_grad_(True) for t in (means, scales, rot, sem, opa)]
        mm, s, q, se, o = leaves
        m2, o2, se2, s2, cov = args(mm, s, q, se, o)
        if fused:
            out = agg.forward_from_rotations(pts, m2, o2.reshape(1, -1), se2, s2, q)
        else:
            out = agg(pts, m2, o2.reshape(1, -1), se2, s2, cov)
        out.backward(torch.ones_like(out) * 0.01)
        return out.detach(), [t.grad for t in leaves]

    out_a, grads_a = run(False)
    out_b, grads_b = run(True)
    assert out_a.shape == (dims[0] * dims[1] * dims[2], 18) and out_a.abs().max() > 0
    differ = (out_a != out_b).any(-1).sum().item()
    print(f"cell {g}: {differ} of {out_a.shape[0]} voxels differ between forward and forward_from_rotations")
    assert torch.equal(out_a, out_b), f"{differ} voxels differ"
    for ga, gb in zip(grads_a, grads_b):
        assert torch.isfinite(ga).all()
        assert torch.allclose(ga, gb, rtol=1e-4, atol=1e-5 * ga.abs().max().item())


# ------------------------------------------------------------------ 4: Sigma^-1 at the conditioning edges
P_EXT = 4099


@pytest.fixture(scope="module")
def ext():
    """The conditioning set and its float64 truth (CPU, computed once): ``A`` and the gradients under the seeded cotangent for
    the packed and the full form, on the rows that have a rotation."""
    scales, rot = pe.extreme_gaussians(P_EXT, 1)
    reg = pe.regular_rows(P_EXT)
    d = dict(scales=scales, rot=rot, reg=torch.from_numpy(reg), g={}, sg={}, qg={})
    for packed in (True, False):
        g = cotangent(P_EXT, packed)
        A, sg, qg = truth_fp64(scales[reg], rot[reg], g[d["reg"]], packed)
        d["A"] = A
        d["g"][packed], d["sg"][packed], d["qg"][packed] = g, sg, qg
    return d


def _prepare_cov(gpu, scales, rot, full):
    from gaussianformer_amd.gaussian_prepare import gaussian_prepare
    P = scales.shape[0]
    return gaussian_prepare(torch.zeros(P, 3, device=gpu), scales, rot, [0.0, 0.0, 0.0], 1.0, 1.0, 1, 1, 1, full_cov=full)[2]


def test_sigma_inverse_values_at_the_conditioning_edges(gpu, ext):
    """Scales over [0.01, 3.2] per axis (anisotropy up to 320, Sigma^-1 entries up to 1e4) and quaternion norms over
    [1e-3, 1e3]: per row within 4e-6 of the row's largest entry of float64 truth, the packed and the full form equal element
    for element, ``gaussian_prepare`` and ``covariance_inverse`` the same bits."""
    from gaussianformer_amd.gaussian_prepare import covariance_inverse
    from oracle import prepare_ref
    s, q, reg = _t(ext["scales"], gpu), _t(ext["rot"], gpu), ext["reg"]
    got = {("prepare", False): _prepare_cov(gpu, s, q, False), ("prepare", True): _prepare_cov(gpu, s, q, True),
           ("covariance_inverse", False): covariance_inverse(s, q, packed=True),
           ("covariance_inverse", True): covariance_inverse(s, q, packed=False)}
    for (name, full), cov in got.items():
        cov = cov.cpu()
        assert cov.shape == ((P_EXT, 3, 3) if full else (P_EXT, 6)) and torch.isfinite(cov).all()
        r = value_ratio(cov[reg], ext["A"])
        print(f"{name} ({'full' if full else 'packed'}): values at {r:.3f} of the bound ({VALUE_BOUND:g} of the row's largest entry)")
        assert r <= 1.0
    for name in ("prepare", "covariance_inverse"):
        assert torch.equal(prepare_ref.pack6(got[(name, True)]), got[(name, False)])
        assert torch.equal(got[(name, True)], got[(name, True)].transpose(-1, -2))
    assert torch.equal(got[("prepare", False)], got[("covariance_inverse", False)])


@pytest.mark.parametrize("packed", [True, False])
def test_sigma_inverse_gradients_at_the_conditioning_edges(gpu, ext, packed):
    from gaussianformer_amd.gaussian_prepare import covariance_inverse
    reg = ext["reg"]
    s = _t(ext["scales"], gpu).requires_grad_(True)
    q = _t(ext["rot"], gpu).requires_grad_(True)
    g = ext["g"][packed]
    covariance_inverse(s, q, packed=packed).backward(g.to(gpu))
    sg, qg = s.grad.cpu(), q.grad.cpu()
    assert torch.isfinite(sg).all() and torch.isfinite(qg).all()
    rs, rq = grad_ratios(sg[reg], qg[reg], ext["sg"][packed], ext["qg"][packed], ext["scales"][reg.numpy()],
                         ext["rot"][reg.numpy()], g[reg])
    print(f"covariance_inverse(packed={packed}): scale gradients at {rs:.3f}, rotation gradients at {rq:.3f} of the bound")
    assert rs <= 1.0 and rq <= 1.0
    # equal scales: Sigma^-1 = I / s^2 whatever the rotation -- the rotation gradient is zero in exact arithmetic
    row = P_EXT + pe.ROW_EQUAL_SCALES
    smin = float(ext["scales"][row].min())
    qn = float(np.linalg.norm(ext["rot"][row].astype(np.float64)))
    tol = 2e-5 * ext["qg"][packed][-1].abs().max().item() + 2e-6 * g[reg].abs().max().item() / smin ** 2 / qn
    print(f"equal scales: |rotation gradient| {qg[row].abs().max().item():.3e}, bound {tol:.3e}")
    assert ext["qg"][packed][-1].abs().max().item() <= 1e-9 * tol and qg[row].abs().max().item() <= tol


def _constructed(gpu, ext):
    from gaussianformer_amd.gaussian_prepare import covariance_inverse
    s = _t(ext["scales"], gpu).requires_grad_(True)
    q = _t(ext["rot"], gpu).requires_grad_(True)
    cov = covariance_inverse(s, q, packed=False)
    cov.backward(ext["g"][False].to(gpu))
    return cov.detach().cpu(), s.grad.cpu(), q.grad.cpu()


@pytest.mark.parametrize("row,name", [(pe.ROW_ZERO_QUAT, "zero"), (pe.ROW_TINY_QUAT, "norm 1e-20")])
def test_quaternion_without_a_direction_gives_zero(gpu, ext, row, name):
    """The zero quaternion, and a norm of 1e-20 -- below the 1e-12 clamp that ``F.normalize`` and ``unit_quat`` share, where
    ``q / 1e-12`` is no unit quaternion and ``R^T S^-2 R`` the inverse of nothing (left to itself the closed form gives
    1e-32 / s^2 there, the reference the inverse of 1e-32 s^2): no rotation, Sigma^-1 exactly 0, a rotation gradient of exactly
    0, everything finite."""
    cov, sg, qg = _constructed(gpu, ext)
    row = P_EXT + row
    print(f"{name}: |Sigma^-1| {cov[row].abs().max().item():.3e}, |rotation gradient| {qg[row].abs().max().item():.3e}, "
          f"|scale gradient| {sg[row].abs().max().item():.3e}")
    assert torch.isfinite(cov[row]).all() and torch.isfinite(sg[row]).all() and torch.isfinite(qg[row]).all()
    assert (cov[row] == 0).all() and (qg[row] == 0).all()
    for full in (False, True):
        assert (_prepare_cov(gpu, _t(ext["scales"], gpu), _t(ext["rot"], gpu), full)[row] == 0).all()


def test_identity_quaternion_gives_the_diagonal(gpu, ext):
    """(1, 0, 0, 0): Sigma^-1 = diag(1 / s^2), the off-diagonal exactly 0 and the diagonal within one fp32 epsilon (the square
    and the reciprocal round by half an ulp each)."""
    cov, _, _ = _constructed(gpu, ext)
    row = P_EXT + pe.ROW_IDENTITY
    want = 1.0 / torch.from_numpy(ext["scales"][row]).double() ** 2
    rel = ((torch.diagonal(cov[row]).double() - want).abs() / want).max().item()
    print(f"identity quaternion: diagonal off by {rel / 2.0 ** -23:.3f} fp32 epsilon")
    assert rel <= 2.0 ** -23 * (1 + 2.0 ** -20)
    assert (cov[row] - torch.diag(torch.diagonal(cov[row])) == 0).all()


def test_rotations_view_off_a_16_byte_boundary(gpu, ext):
    """A contiguous ``rotations`` view that starts 4 bytes into its storage (a slice of an anchor tensor): the library loads a
    quaternion with one 16-byte load and refuses the pointer; the Python layer copies the view.  Same bits as the aligned
    copy from ``gaussian_prepare``, ``covariance_inverse`` (values and gradients) and ``forward_from_rotations``."""
    from gaussianformer_amd import _lib
    from gaussianformer_amd.gaussian_prepare import covariance_inverse
    from gaussianformer_amd.local_aggregate import LocalAggregator
    P = 300
    scales, rot = _t(ext["scales"][:P], gpu), _t(ext["rot"][:P], gpu)
    flat = torch.zeros(4 * P + 4, device=gpu)
    flat[1:4 * P + 1] = rot.reshape(-1)
    view = flat[1:4 * P + 1].view(P, 4)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and rot.data_ptr() % 16 == 0 and torch.equal(view, rot)
    with pytest.raises(RuntimeError, match="16-byte aligned"):       # the C entry point keeps its check
        _lib.call("gf_gaussian_prepare", gpu, P, 1, 1, 1, ctypes.cast((ctypes.c_float * 3)(), ctypes.c_void_p), 1.0, 1.0,
                  _lib.GF_RADII_SCALAR, 1, None, scales, view, None, None, torch.empty(P, 6, device=gpu), None, None)
    assert torch.equal(_prepare_cov(gpu, scales, view, False), _prepare_cov(gpu, scales, rot, False))
    res = []
    for r in (rot, view):
        s, q = scales.clone().requires_grad_(True), r.detach().requires_grad_(True)
        cov = covariance_inverse(s, q, packed=True)
        cov.backward(ext["g"][True][:P].to(gpu))
        res.append((cov.detach(), s.grad, q.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # end to end: the fused aggregator entry, forward and backward
    dims, lo, m, g = pe.SMALL_GRID, pe.SMALL_PC_MIN, pe.SMALL_MULTIPLIER, 0.5
    pts_np, means_np, scales_np = pe.end_to_end_case(lo, g, *dims, m, P=P + 60)
    pts, means, sc = _t(pts_np, gpu)[None], _t(means_np[:P], gpu)[None], _t(scales_np[:P], gpu)[None]
    rng = np.random.default_rng(6)
    sem = _t(np.abs(rng.standard_normal((1, P, 18))).astype(np.float32), gpu)
    opa = _t(rng.random((1, P)).astype(np.float32), gpu)
    agg = LocalAggregator(m, *dims, list(lo), g, matrix_cores=False).to(gpu)
    res = []
    for r in (rot, view):
        s, q = sc.clone().requires_grad_(True), r.detach()[None].requires_grad_(True)
        out = agg.forward_from_rotations(pts, means, opa, sem, s, q)
        out.backward(torch.ones_like(out) * 0.01)
        res.append((out.detach(), q.grad))
    assert torch.equal(res[0][0], res[1][0]) and res[0][0].abs().max() > 0
    assert torch.allclose(res[0][1], res[1][1], rtol=1e-4, atol=1e-5 * res[0][1].abs().max().item())   # (fp32 atomics)
