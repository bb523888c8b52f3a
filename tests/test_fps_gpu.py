"""gf_farthest_point_sampling on the MI355X: every case bit-identical to the numpy oracle (tests/fps_ref.py) and, at full
size, to the exhaustive mode (gf_set_option("fps.exhaustive", 1): no pruning).  FPS is prefix-stable, so the first picks of
a long run are checked against the oracle and the whole run against the exhaustive mode."""
import os

import numpy as np
import pytest

from tests import fps_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _run(gpu, xyz, offset, new_offset, exhaustive=False):
    import torch
    from gaussianformer_amd import _lib
    from pointops import farthest_point_sampling
    x = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).to(gpu)
    off = torch.tensor(offset, dtype=torch.int32, device=gpu)
    new = torch.tensor(new_offset, dtype=torch.int32, device=gpu)
    with _lib.option("fps.exhaustive", int(exhaustive)):
        idx = farthest_point_sampling(x, off, new)
    assert idx.dtype == torch.int32 and idx.device == x.device and idx.shape == (int(new_offset[-1]),)
    return idx.cpu().numpy()


def _check(gpu, xyz, offset, new_offset):
    want = fps_ref.fps(xyz, offset, new_offset)
    got = _run(gpu, xyz, offset, new_offset)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_run(gpu, xyz, offset, new_offset, exhaustive=True), want)


@pytest.mark.parametrize("n,m", [(1, 1), (63, 20), (64, 64), (65, 65), (5000, 1000), (20000, 3000)])
def test_uniform(gpu, n, m):
    xyz = np.random.default_rng(n).uniform(-40.0, 40.0, (n, 3)).astype(np.float32)
    _check(gpu, xyz, [n], [m])


@pytest.mark.parametrize("kind", ["lattice", "duplicates", "identical"])
def test_ties(gpu, kind):
    from gaussianformer_amd.synthetic import make_fps_tie_points
    xyz = make_fps_tie_points(kind, 4096, seed=5)
    _check(gpu, xyz, [4096], [1500])


def test_more_picks_than_points_and_the_cap(gpu):
    rng = np.random.default_rng(9)
    big = np.where(rng.random((300, 3)) < 0.5, -1e6, 1e6).astype(np.float32) + rng.uniform(-5, 5, (300, 3)).astype(np.float32)
    _check(gpu, big, [300], [400])
    _check(gpu, rng.uniform(0, 1, (10, 3)).astype(np.float32), [10], [37])


def test_uneven_segments(gpu):
    rng = np.random.default_rng(11)
    sizes = [1, 700, 0, 64, 3001, 2, 129]
    picks = [1, 300, 0, 80, 1000, 0, 5]
    xyz = rng.normal(0.0, 10.0, (sum(sizes), 3)).astype(np.float32)
    _check(gpu, xyz, np.cumsum(sizes).tolist(), np.cumsum(picks).tolist())


def test_lifter_three_segment_call(gpu):
    """The lifter's benchmarking=True call, unchanged (model/lifter/gaussian_lifter_v2.py:241-246)."""
    import torch
    from pointops import farthest_point_sampling
    from gaussianformer_amd.synthetic import make_lifter_points
    scan = torch.from_numpy(make_lifter_points(seed=2, h=27, w=50)).to(gpu)
    scan = scan[torch.from_numpy(np.random.default_rng(0).permutation(scan.shape[0])).to(gpu)]
    num_anchor, num_subsets = 1500, 3
    sublens = torch.linspace(0, scan.shape[0], num_subsets + 1, dtype=torch.int, device=scan.device)[1:]
    new_sublens = torch.linspace(0, num_anchor, num_subsets + 1, dtype=torch.int, device=scan.device)[1:]
    scanidx = farthest_point_sampling(scan, sublens, new_sublens)
    want = fps_ref.fps(scan.cpu().numpy(), sublens.cpu().numpy(), new_sublens.cpu().numpy())
    np.testing.assert_array_equal(scanidx.cpu().numpy(), want)
    assert scan[scanidx, :].shape == (num_anchor, 3)


def test_recorded_reference_lifter_calls(gpu):
    """The calls the reference's own GaussianLifterV2 made (tools/make_golden_lifter_fps.py), with the oracle's answers."""
    g = np.load(os.path.join(GOLDEN, "lifter_fps.npz"))
    calls = sorted({k.split("_")[0] for k in g.files})
    assert len(calls) >= 2
    for c in calls:
        scan, off, new, want = g[c + "_scan"], g[c + "_offset"], g[c + "_new_offset"], g[c + "_idx"]
        assert off.dtype == np.int32 and new.dtype == np.int32
        np.testing.assert_array_equal(fps_ref.fps(scan, off, new), want)
        np.testing.assert_array_equal(_run(gpu, scan, off.tolist(), new.tolist()), want)


def _long_run(gpu, xyz, m, prefix):
    n = xyz.shape[0]
    got = _run(gpu, xyz, [n], [m])
    np.testing.assert_array_equal(got, _run(gpu, xyz, [n], [m], exhaustive=True))
    np.testing.assert_array_equal(got[:prefix], fps_ref.fps(xyz, [n], [prefix]))
    assert len(np.unique(got)) == m   # m < n distinct points: no repeats


def test_lifter_shaped_full_size(gpu):
    from gaussianformer_amd.synthetic import make_lifter_points
    xyz = make_lifter_points(seed=0)
    assert xyz.shape == (129600, 3)
    _long_run(gpu, xyz, 19200, 4000)


def test_segment_at_the_limit(gpu):
    from gaussianformer_amd import sampling
    n = sampling.MAX_SEGMENT_POINTS
    xyz = np.random.default_rng(4).uniform(-50.0, 50.0, (n, 3)).astype(np.float32)
    _long_run(gpu, xyz, 6400, 1500)


def test_repeatable_and_on_a_side_stream(gpu):
    import torch
    from pointops import farthest_point_sampling
    from gaussianformer_amd.synthetic import make_lifter_points
    xyz = torch.from_numpy(make_lifter_points(seed=3, h=54, w=100)).to(gpu)
    off = torch.tensor([xyz.shape[0]], dtype=torch.int32, device=gpu)
    new = torch.tensor([4000], dtype=torch.int32, device=gpu)
    a = farthest_point_sampling(xyz, off, new)
    b = farthest_point_sampling(xyz, off, new)
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        c = farthest_point_sampling(xyz, off, new)
    torch.cuda.current_stream(gpu).wait_stream(s)
    torch.cuda.synchronize(gpu)
    assert torch.equal(a, b) and torch.equal(a, c)
    np.testing.assert_array_equal(a.cpu().numpy()[:1000], fps_ref.fps(xyz.cpu().numpy(), [xyz.shape[0]], [1000]))
