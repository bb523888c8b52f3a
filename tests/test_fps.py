"""Farthest point sampling without a GPU: the numpy oracle (tests/fps_ref.py) on hand-worked orders and tie cases,
argument validation through the C ABI (before any HIP call), and the drop-in ``pointops`` refusing CPU tensors."""
import ctypes

import numpy as np
import pytest

from tests import fps_ref


def test_points_on_a_line():
    # 0 first, then the far end 10, then 5 (d = 25); then 2, 7 and 8 all have d = 4 and go in index order
    x = np.array([0, 10, 5, 2, 7, 8], np.float32)
    p = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    assert fps_ref.fps_segment(p, 6).tolist() == [0, 1, 2, 3, 4, 5]
    # reordered: the same geometry, other indices
    order = [3, 1, 0, 5, 2, 4]
    q = p[order]
    got = fps_ref.fps_segment(q, 4)
    assert q[got[0], 0] == 2.0 and q[got[1], 0] == 10.0


def test_square_corners_then_centre():
    p = np.array([[0, 0, 0], [1, 1, 0], [0.5, 0.5, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    # from corner 0: the opposite corner (d = 2); then corners 3 and 4 tie at d = 1 -> 3 first; then 4; then the centre
    assert fps_ref.fps_segment(p, 5).tolist() == [0, 1, 3, 4, 2]


def test_lattice_ties_go_to_the_lowest_index():
    from gaussianformer_amd.synthetic import make_fps_tie_points
    p = make_fps_tie_points("lattice", 512, seed=1)
    got = fps_ref.fps_segment(p, 200)
    d = np.full(p.shape[0], 1e10, np.float32)
    ties = 0
    for i in range(len(got) - 1):
        c = p[got[i]]
        diff = p - c
        d = np.minimum(d, diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2])
        best = np.flatnonzero(d == d.max())
        assert got[i + 1] == best[0]
        ties += len(best) > 1
    assert ties > 150   # the lattice really decides most picks by exact ties


def test_duplicates_and_more_picks_than_points():
    p = np.array([[1, 2, 3], [1, 2, 3], [4, 5, 6], [4, 5, 6]], np.float32)
    # 0, then 2 (first of the far pair), then every d is 0: the lowest index, 0, again and again
    assert fps_ref.fps_segment(p, 7).tolist() == [0, 2, 0, 0, 0, 0, 0]
    one = np.array([[3, 3, 3]], np.float32)
    assert fps_ref.fps_segment(one, 3).tolist() == [0, 0, 0]


def test_zero_picks_and_segments():
    xyz = np.arange(30, dtype=np.float32).reshape(10, 3)
    assert fps_ref.fps(xyz, [10], [0]).size == 0
    got = fps_ref.fps(xyz, [4, 4, 10], [2, 2, 5])
    assert got.dtype == np.int32 and got.tolist() == [0, 3, 4, 9, 6]


def test_the_1e10_cap():
    # at +-1e6 every squared distance exceeds 1e10, so d stays 1e10 everywhere but at the picks: the order is by index
    p = np.array([[1e6, 1e6, 1e6], [-1e6, -1e6, -1e6], [1e6, -1e6, 1e6], [-1e6, 1e6, -1e6]], np.float32)
    assert fps_ref.fps_segment(p, 4).tolist() == [0, 1, 2, 3]


def _call(n, off, new, ws_bytes=1 << 20, xyz=1):
    from gaussianformer_amd import _lib
    lib = _lib.load()
    b = len(off)
    oh = (ctypes.c_int * b)(*off)
    nh = (ctypes.c_int * b)(*new)
    fake = ctypes.c_void_p(16) if xyz else None   # never dereferenced: validation fails before any HIP call
    rc = lib.gf_farthest_point_sampling(n, b, ctypes.cast(oh, ctypes.c_void_p), ctypes.cast(nh, ctypes.c_void_p), fake, fake, fake,
                                        fake, fake, ws_bytes, None)
    return rc, lib.gf_last_error().decode()


def test_abi_validates_offsets():
    rc, msg = _call(10, [6, 4], [2, 4])
    assert rc == -1 and "non-decreasing" in msg
    rc, msg = _call(10, [4, 10], [3, 2])
    assert rc == -1 and "non-decreasing" in msg
    rc, msg = _call(10, [4, 9], [1, 2])
    assert rc == -1 and "offset[b-1]" in msg
    rc, msg = _call(-1, [4], [1])
    assert rc == -1


def test_abi_refuses_an_empty_segment_with_picks():
    rc, msg = _call(10, [4, 4, 10], [1, 2, 3])
    assert rc == -1 and "segment 1 is empty" in msg
    # an empty segment without picks is fine up to the workspace check (all-zero picks return before it)
    rc, msg = _call(10, [4, 4, 10], [0, 0, 0], ws_bytes=0)
    assert rc == 0


def test_abi_refuses_a_segment_over_the_limit():
    from gaussianformer_amd import sampling
    n = sampling.MAX_SEGMENT_POINTS + 1
    rc, msg = _call(n, [n], [10])
    assert rc == -1 and "262144" in msg
    rc, msg = _call(n + 5, [5, n + 5], [1, 1])   # the limit is per segment
    assert rc == -1 and "segment 1" in msg
    m = sampling.MAX_SEGMENT_POINTS
    rc, msg = _call(2 * m, [m, 2 * m], [1, 2], ws_bytes=0)   # two segments at the limit: only the workspace is short
    assert rc == -2 and "workspace" in msg


def test_workspace_size_and_option():
    from gaussianformer_amd import _lib
    lib = _lib.load()
    assert lib.gf_fps_workspace_bytes(0) == 0
    assert lib.gf_fps_workspace_bytes(-1) == 0
    assert lib.gf_fps_workspace_bytes(129600) >= 129600 * 20
    assert _lib.get_option("fps.exhaustive") == 0
    with _lib.option("fps.exhaustive", 1):
        assert _lib.get_option("fps.exhaustive") == 1
    assert _lib.get_option("fps.exhaustive") == 0


def test_pointops_drop_in_has_no_cpu_fallback():
    import torch
    from pointops import farthest_point_sampling
    xyz = torch.rand(100, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        farthest_point_sampling(xyz, torch.tensor([100], dtype=torch.int), torch.tensor([10], dtype=torch.int))
