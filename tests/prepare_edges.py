"""Input builders for the splat's per-Gaussian pre-processing at its edges (tests/test_prepare_edges*.py): centres on and
around the cell faces, scales on and around the steps of the radius' ceil, and Gaussians at the ends of the conditioning
range.  numpy only, deterministic; a plain helper module like tests/dcn_ref.py.

The integer path is ``trunc((x - lo) / g)`` and ``ceil(s * m / g)`` in fp32 with a correctly rounded division
(oracle.prepare_splat_inputs).  A device may be tempted to multiply by ``fl32(1 / g)`` instead; ``cells_*`` / ``radii_*`` below
state both so that a test can count where they part.
"""
import numpy as np

f32 = np.float32

# (cell, pc_min) of the product (0.5), of the module's own tests (0.4) and of two further cells that are no power of two
CELLS = [(0.5, (-50.0, -50.0, -5.0)), (0.4, (-40.0, -40.0, -1.0)), (0.2, (-51.2, -51.2, -5.0)), (0.32, (-40.0, -40.0, -1.0))]
GRID = (200, 200, 16)          # the product's grid: only P grows with it
MULTIPLIERS = (2, 3, 4, 5)     # the configs use 3, 4 and 5
RADII_R = range(1, 64)
# the small end-to-end splat: the origin is near zero so that the ulp of a centre resolves the faces k = 13, 17, 21, where
# a 0.4 m cell's division and reciprocal part (from k = 21 on only with the origins of CELLS)
SMALL_GRID, SMALL_PC_MIN, SMALL_MULTIPLIER = (24, 20, 8), (-1.0, -1.0, -1.0), 3


def _ulps(v, k):
    """``v`` moved by ``k`` float32 ulps (k may be negative)."""
    v = f32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, f32(np.inf if k > 0 else -np.inf), dtype=f32)
    return v


def mid_cell(lo, g, dims):
    """A mid-cell value per axis (cell dim // 2)."""
    return [f32(f32((n // 2 + 0.5) * g) + f32(l)) for n, l in zip(dims, lo)]


def _on_axis(values, axis, mid):
    out = np.empty((len(values), 3), f32)
    out[:] = mid
    out[:, axis] = values
    return out


def face_values(lo, g, n):
    """One axis: ``fl32(fl32(k * g) + lo)`` for k = 0..n (the upper face included) and its +-1 and +-2 ulp neighbours."""
    vals = []
    for k in range(n + 1):
        face = f32(f32(k * f32(g)) + f32(lo))
        vals += [_ulps(face, d) for d in (-2, -1, 0, 1, 2)]
    return np.array(vals, f32)


def below_lower_face(pc_min, g, H, W, D):
    """Centres in ``(lo - g, lo)`` on one axis each: truncation toward zero puts them in cell 0, the range asserts pass."""
    mid = mid_cell(pc_min, g, (H, W, D))
    rows = [_on_axis(np.array([f32(f32(lo) - f32(t * g)) for t in (0.05, 0.5, 0.95)], f32), ax, mid)
            for ax, lo in enumerate(pc_min)]
    return np.concatenate(rows)


def upper_face(pc_min, g, H, W, D):
    """Centres beyond the upper face on one axis each (the face itself is part of ``face_values``): cell ``dim`` or
    ``dim + 1``, out of grid."""
    mid = mid_cell(pc_min, g, (H, W, D))
    rows = [_on_axis(np.array([f32(f32(f32(n * f32(g)) + f32(lo)) + f32(t * g)) for t in (0.25, 1.5)], f32), ax, mid)
            for ax, (lo, n) in enumerate(zip(pc_min, (H, W, D)))]
    return np.concatenate(rows)


def boundary_means(pc_min, g, H, W, D):
    """Centres ``[P, 3]`` fp32: every cell face of every axis and its neighbours (the other two axes mid-cell), then the
    centres just below the lower face and those beyond the upper one.  P is about 2 100 at the product's grid."""
    mid = mid_cell(pc_min, g, (H, W, D))
    rows = [_on_axis(face_values(lo, g, n), ax, mid) for ax, (lo, n) in enumerate(zip(pc_min, (H, W, D)))]
    return np.concatenate(rows + [below_lower_face(pc_min, g, H, W, D), upper_face(pc_min, g, H, W, D)])


def _step(r, g, m, d):
    return _ulps(f32(f32(r * f32(g)) / f32(m)), d)


def ceil_scales(g, m):
    """Scales ``[378, 3]`` fp32 on the steps of ``ceil(s * m / g)``: ``fl32(fl32(r * g) / m)`` and its +-1 ulp neighbours,
    r = 1..63, a different r on each axis.  First half: three steps (r, r + 21, r + 42 modulo 63) per row, rotated through
    the axes -- the per-axis mode meets every r on every axis.  Second half: r on one axis, r / 2 and r / 4 on the others, so
    that every r is also the largest of its row -- what the scalar modes take."""
    a, b = [], []
    for r in RADII_R:
        for d in (-1, 0, 1):
            tri = [_step(r, g, m, d), _step(1 + (r + 20) % 63, g, m, d), _step(1 + (r + 41) % 63, g, m, d)]
            a.append(np.roll(tri, r % 3))
            s = _step(r, g, m, d)
            b.append(np.roll([s, f32(s * f32(0.5)), f32(s * f32(0.25))], r % 3))
    return np.array(a + b, f32)


# the hand-made rows of extreme_gaussians, counted from the end
ROW_ZERO_QUAT, ROW_TINY_QUAT, ROW_IDENTITY, ROW_EQUAL_SCALES = -4, -3, -2, -1


def extreme_gaussians(P, seed):
    """``(scales [P, 3], rotations [P, 4])`` fp32 at the ends of the conditioning range: scales log-uniform in [0.01, 3.2]
    per axis (the prob configs' range), quaternions of uniform direction and a norm log-uniform in [1e-3, 1e3].  The last
    four rows are made by hand: an exactly zero quaternion, a norm of 1e-20 (below the 1e-12 clamp of F.normalize), the
    identity (1, 0, 0, 0), and three equal scales."""
    rng = np.random.default_rng(seed)
    scales = np.exp(rng.uniform(np.log(0.01), np.log(3.2), (P, 3)))
    q = rng.standard_normal((P, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    q *= np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (P, 1)))
    scales, q = scales.astype(f32), q.astype(f32)
    q[ROW_ZERO_QUAT] = 0.0
    q[ROW_TINY_QUAT] = q[ROW_TINY_QUAT].astype(np.float64) / np.linalg.norm(q[ROW_TINY_QUAT].astype(np.float64)) * 1e-20
    q[ROW_IDENTITY] = (1.0, 0.0, 0.0, 0.0)
    scales[ROW_EQUAL_SCALES] = scales[ROW_EQUAL_SCALES, 0]
    return scales, q


def regular_rows(P):
    """Mask of the rows whose Sigma^-1 is defined (a rotation exists): all but the zero and the below-clamp quaternion."""
    m = np.ones(P, bool)
    m[[ROW_ZERO_QUAT, ROW_TINY_QUAT]] = False
    return m


def tile(a, P):
    """``a`` repeated along axis 0 to ``P`` rows (pairs the shorter set with the longer one)."""
    return np.ascontiguousarray(np.resize(a, (P,) + a.shape[1:])) if len(a) != P else a


def end_to_end_case(pc_min, g, H, W, D, m, P=360, seed=11):
    """``(pts [H W D, 3], means [P, 3], scales [P, 3])`` fp32 for a small splat: the dense voxel-centre grid (the arithmetic
    of the reference's get_meshgrid, x-major), and Gaussians all inside the grid of which the first third sits on cell faces
    with all three axes (faces 0..dim-1 and their neighbours), the second third has scales on the ceil steps r = 1..12 (every
    r the largest of its row), and the rest is ordinary."""
    rng = np.random.default_rng(seed)
    dims = (H, W, D)
    axes = [np.arange(n, dtype=f32) * f32(g) + f32(0.5) * f32(g) + f32(lo) for n, lo in zip(dims, pc_min)]
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    t = P // 3
    assert t >= 5 * max(dims)
    inside = np.stack([rng.uniform(lo + 0.1 * g, lo + (n - 0.1) * g, P) for n, lo in zip(dims, pc_min)], -1).astype(f32)
    means = inside.copy()
    for ax, (lo, n) in enumerate(zip(pc_min, dims)):
        faces = face_values(lo, g, n)[:5 * n]
        means[:t, ax] = tile(rng.permutation(faces), t)      # (t >= 5 n on every axis: every face value is used)
    scales = rng.uniform(0.08, 0.6, (P, 3)).astype(f32)
    steps = ceil_scales(g, m)
    steps = steps[len(steps) // 2:][:3 * 12]
    scales[t:2 * t] = tile(steps, t)
    return pts, means, scales


# ---- the two candidate definitions, in numpy fp32 --------------------------------------------------------------------------
def cells_divide(x, lo, g):
    return ((x.astype(f32) - f32(lo)) / f32(g)).astype(np.int32)


def cells_reciprocal(x, lo, g):
    return ((x.astype(f32) - f32(lo)) * (f32(1) / f32(g))).astype(np.int32)


def radii_divide(s, m, g):
    return np.ceil(s.astype(f32) * f32(m) / f32(g)).astype(np.int32)


def radii_reciprocal(s, m, g):
    return np.ceil(s.astype(f32) * f32(m) * (f32(1) / f32(g))).astype(np.int32)
