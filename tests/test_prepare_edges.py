"""The splat's integer path and Sigma^-1 at cell, ceil and scale edges -- the part that needs no GPU: the built input sets
(tests/prepare_edges.py) can tell a correctly rounded fp32 division from a multiplication by the fp32 reciprocal, the
checker (oracle.prepare_splat_inputs) is the reference's expression bit for bit, and the bounds the GPU tests
(tests/test_prepare_edges_gpu.py) hold Sigma^-1 to leave a plain fp32 closed form a margin of 3x."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle import prepare_ref
import prepare_edges as pe

CELL_IDS = [f"cell{g}" for g, _ in pe.CELLS]


# ------------------------------------------------------------------ the sets can see the difference
def _differing(g, lo):
    means = pe.boundary_means(lo, g, *pe.GRID)
    cells = sum(int((pe.cells_divide(means[:, a], lo[a], g) != pe.cells_reciprocal(means[:, a], lo[a], g)).sum())
                for a in range(3))
    radii = 0
    for m in pe.MULTIPLIERS:
        s = pe.ceil_scales(g, m)
        radii += int((pe.radii_divide(s.max(-1), m, g) != pe.radii_reciprocal(s.max(-1), m, g)).sum())   # scalar modes
        radii += int((pe.radii_divide(s, m, g) != pe.radii_reciprocal(s, m, g)).sum())                    # per axis
    return cells, radii


@pytest.mark.parametrize("g,lo", pe.CELLS, ids=CELL_IDS)
def test_sets_tell_division_from_reciprocal(g, lo):
    """On a cell that is no power of two, ``trunc(d / g)`` and ``trunc(d * fl32(1 / g))`` (likewise the ceil of the radii)
    must part on the built sets often enough for a device that takes the shortcut to be caught; on 0.5 they cannot part --
    the recorded reason the product's workload is unaffected."""
    cells, radii = _differing(g, lo)
    print(f"cell {g}: {cells} centre components and {radii} radii differ")
    if g == 0.5:
        assert cells == 0 and radii == 0
    else:
        assert cells >= 10 and radii >= 1
        if g == 0.32:
            assert radii >= 10


@pytest.mark.parametrize("g,lo", pe.CELLS, ids=CELL_IDS)
def test_sets_cover_what_they_claim(g, lo):
    H, W, D = pe.GRID
    means = pe.boundary_means(lo, g, H, W, D)
    assert 8 * 256 < len(means) <= 9 * 256 and means.dtype == np.float32          # nine blocks, the last one partial
    cells = np.stack([pe.cells_divide(means[:, a], lo[a], g) for a in range(3)], -1)
    for a, n in enumerate((H, W, D)):
        seen = set(cells[:, a].tolist())
        assert {0, n - 1, n} <= seen and len(seen & set(range(n + 1))) >= 0.95 * (n + 1)   # the grid, and the cell past it
    below = pe.below_lower_face(lo, g, H, W, D)
    assert (below < np.asarray(lo, np.float32)).any(-1).all()
    assert (np.stack([pe.cells_divide(below[:, a], lo[a], g) for a in range(3)], -1) >= 0).all()    # truncation: cell 0
    above = pe.upper_face(lo, g, H, W, D)
    ca = np.stack([pe.cells_divide(above[:, a], lo[a], g) for a in range(3)], -1)
    assert (ca >= np.array([H, W, D])).any(-1).all()
    for m in pe.MULTIPLIERS:
        s = pe.ceil_scales(g, m)
        r = pe.radii_divide(s, m, g)
        assert (s > 0).all() and set(pe.RADII_R) <= set(r.max(-1).tolist())         # every r is some row's largest
        assert all(set(pe.RADII_R) <= set(r[:, a].tolist()) for a in range(3))
        three = np.sort(r[:len(r) // 2], -1)
        assert (three[:, 0] < three[:, 1]).all() and (three[:, 1] < three[:, 2]).all()    # first half: three different r
    assert np.array_equal(pe.boundary_means(lo, g, H, W, D), means)                 # deterministic


@pytest.mark.parametrize("g", [g for g, _ in pe.CELLS])
def test_end_to_end_case_is_sensitive_and_in_grid(g):
    lo, dims, m = pe.SMALL_PC_MIN, pe.SMALL_GRID, pe.SMALL_MULTIPLIER
    pts, means, scales = pe.end_to_end_case(lo, g, *dims, m)
    assert pts.shape == (dims[0] * dims[1] * dims[2], 3) and 300 <= len(means) <= 400
    pi, mi, radii, _ = oracle.prepare_splat_inputs(pts, means, scales, np.zeros((len(means), 3, 3), np.float32), list(lo), g, m)
    key = (pi[:, 0] * dims[1] + pi[:, 1]) * dims[2] + pi[:, 2]
    assert np.array_equal(key, np.arange(len(pts)))                                  # the dense grid, point n in voxel n
    assert (mi >= 0).all() and (mi < np.array(dims)).all() and (radii >= 1).all()    # the range asserts pass
    cells = sum(int((pe.cells_divide(means[:, a], lo[a], g) != pe.cells_reciprocal(means[:, a], lo[a], g)).sum())
                for a in range(3))
    print(f"end-to-end case, cell {g}: {cells} centre components differ")
    assert cells == 0 if g == 0.5 else cells >= 1


def test_extreme_gaussians_cover_the_range():
    P = 4099
    s, q = pe.extreme_gaussians(P, 1)
    s2, q2 = pe.extreme_gaussians(P, 1)
    assert np.array_equal(s, s2) and np.array_equal(q, q2)
    assert s.min() >= 0.01 and s.max() <= 3.2 and s.min() < 0.0105 and s.max() > 3.0
    n = np.linalg.norm(q.astype(np.float64), axis=-1)
    reg = pe.regular_rows(P)
    assert n[reg].min() >= 0.99e-3 and n[reg].max() <= 1.01e3 and n[reg].min() < 2e-3 and n[reg].max() > 5e2
    assert (q[pe.ROW_ZERO_QUAT] == 0).all() and 0 < n[pe.ROW_TINY_QUAT] < 1e-12
    assert q[pe.ROW_IDENTITY].tolist() == [1, 0, 0, 0] and len(set(s[pe.ROW_EQUAL_SCALES].tolist())) == 1


# ------------------------------------------------------------------ the definition is pinned
def _torch_cpu_reference(pts, means, scales, lo, g, m, per_axis, radii_min):
    """The reference's expressions (local_aggregate/__init__.py:137-141, _prob :150-152, _prob_fast :151) evaluated by
    torch on the CPU, where the true division by a Python float is correctly rounded."""
    pc_min = torch.tensor(lo, dtype=torch.float).unsqueeze(0)
    points_int = ((torch.from_numpy(pts) - pc_min) / g).to(torch.int)
    means_int = ((torch.from_numpy(means) - pc_min) / g).to(torch.int)
    sc = torch.from_numpy(scales)
    radii = torch.ceil((sc if per_axis else sc.max(dim=-1)[0]) * m / g).to(torch.int)
    if radii_min is not None:
        radii = radii.clamp(min=radii_min)
    return points_int.numpy(), means_int.numpy(), radii.numpy()


@pytest.mark.parametrize("g,lo", pe.CELLS, ids=CELL_IDS)
def test_oracle_is_the_reference_expression(g, lo):
    means = pe.boundary_means(lo, g, *pe.GRID)
    P = len(means)
    cov = np.zeros((P, 3, 3), np.float32)
    for m in pe.MULTIPLIERS:
        scales = pe.tile(pe.ceil_scales(g, m), P)
        for per_axis, radii_min in ((False, None), (False, 1), (False, 4), (True, 1), (True, 4)):
            pi, mi, radii, _ = oracle.prepare_splat_inputs(means, means, scales, cov, list(lo), g, m,
                                                           per_axis=per_axis, radii_min=radii_min)
            ref = _torch_cpu_reference(means, means, scales, lo, g, m, per_axis, radii_min)
            for got, want in zip((pi, mi, radii), ref):
                assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)


# ------------------------------------------------------------------ the yardstick of the Sigma^-1 bounds
VALUE_BOUND = 4e-6      # of the row's largest |entry| (tests/test_prepare.py::test_prepare_forward)


def truth_fp64(scales, rotations, g, packed):
    """float64 ``prepare_ref.covariance_inverse`` and its autograd under the cotangent ``g`` on the rows that have a
    rotation (``pe.regular_rows``): ``(A [P,3,3], scales_grad, rotations_grad)``."""
    s = torch.from_numpy(scales).double().requires_grad_(True)
    q = torch.from_numpy(rotations).double().requires_grad_(True)
    A = prepare_ref.covariance_inverse(s, q)
    (prepare_ref.pack6(A) if packed else A).backward(torch.as_tensor(g).double())
    return A.detach(), s.grad, q.grad


def value_ratio(got, truth):
    """Worst ``|got - truth| / (VALUE_BOUND x the row's largest |entry|)``; ``got`` is ``[P,3,3]`` or packed ``[P,6]``."""
    truth = truth.double()
    ref = truth if got.dim() == 3 else prepare_ref.pack6(truth)
    scale = truth.abs().amax(dim=(-1, -2)).reshape(-1, *([1] * (ref.dim() - 1)))
    return ((got.double() - ref).abs() / (VALUE_BOUND * scale)).max().item()


def grad_ratios(sg, qg, sg_ref, qg_ref, scales, rotations, g):
    """Worst ``|got - truth| / bound`` for the scale and the rotation gradient, row by row, with the bound of
    tests/test_prepare.py::test_prepare_backward_matches_autograd: ``2e-5 max|truth row| + 2e-6 (max|g| / s_min^2) extra``,
    ``extra = 1 / s_min`` for the scales and ``1 / ||q||`` for the rotations (the gradient passes through
    ``(I - q^ q^T) / ||q||``)."""
    s = torch.as_tensor(scales).double()
    smin = s.amin(dim=-1, keepdim=True)
    qn = torch.as_tensor(rotations).double().norm(dim=-1, keepdim=True)
    bound = torch.as_tensor(g).abs().max().item() / smin ** 2
    out = []
    for got, ref, extra in ((sg, sg_ref, 1.0 / smin), (qg, qg_ref, 1.0 / qn)):
        tol = 2e-5 * ref.abs().amax(dim=-1, keepdim=True) + 2e-6 * bound * extra
        out.append(((got.double() - ref).abs() / tol).max().item())
    return out


def cotangent(P, packed):
    return torch.randn((P, 6) if packed else (P, 3, 3), generator=torch.Generator().manual_seed(5))


def closed_form_fp32(scales, rotations):
    """``R^T S^-2 R`` in float32 torch, the quaternion normalised by F.normalize -- what the kernel evaluates per thread."""
    w, x, y, z = F.normalize(rotations, dim=-1).unbind(-1)
    R = torch.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1).reshape(-1, 3, 3)
    return torch.einsum("pki,pk,pkj->pij", R, 1.0 / (scales * scales), R)


@pytest.mark.parametrize("packed", [True, False])
def test_bounds_leave_a_plain_fp32_closed_form_a_margin_of_three(packed):
    """The yardstick of the GPU tests' Sigma^-1 bounds: a straightforward fp32 evaluation of the closed form stays inside
    them by 3x on the conditioning set, in values and autograd gradients.  (``prepare_ref`` in fp32 inverts Cov and is
    ~4e-3 off on these inputs: not a usable yardstick, and no second bound term.)"""
    scales, rot = pe.extreme_gaussians(4099, 1)
    reg = pe.regular_rows(len(scales))
    scales, rot = scales[reg], rot[reg]
    g = cotangent(len(scales), packed)
    A, sg_ref, qg_ref = truth_fp64(scales, rot, g, packed)
    s = torch.from_numpy(scales).requires_grad_(True)
    q = torch.from_numpy(rot).requires_grad_(True)
    got = closed_form_fp32(s, q)
    (prepare_ref.pack6(got) if packed else got).backward(g)
    rv = value_ratio(got.detach(), A)
    rs, rq = grad_ratios(s.grad, q.grad, sg_ref, qg_ref, scales, rot, g)
    print(f"closed form fp32, packed={packed}: values {rv:.3f}, scale grads {rs:.3f}, rotation grads {rq:.3f} of the bound")
    assert rv <= 1 / 3 and rs <= 1 / 3 and rq <= 1 / 3
