"""The submanifold sparse convolution's three products -- output, input gradient, weight gradient -- against the float64 dense
definition ELEMENT BY ELEMENT (tests/subm_judge.py: ``2^-20 sum|a||b|`` per element, plus the f16 format's range term
``2 * 2^-39 rng`` for the default format's output and input gradient), at the shapes where the kernels of csrc/subm_conv.hip
take another path: all nine channel pairs on the tile walk (segments shorter than a tile, fewer MFMA blocks than waves in the
weight gradient), the run walk with 19 - 36 weight-gradient chunks per segment forward and backward, a single segment of
exactly 1 .. 1025 pairs (the 32-pair staging step, the 128-pair tile, the 512-pair chunk, each at n - 1, n, n + 1), K = 7
(343 offsets: more than a workgroup's threads), empty segments, batch faces, crowded cells, and operands whose large elements do
not dominate sum|a||b| (where the f16 format's contract is the composite bound and not the plain one).

Measured on an MI355X, worst error in units of 2^-24 sum|a||b| (the bound is 16; every test prints its own figures):

    ordinary operands        f16 x 2 (default)   bf16 x 3   f32 MFMA
    out                      3.3                 1.3        1.7         (the walks; f16 x 2 also the edge cases: its 3.3 is one segment of 1025 pairs)
    grad_feat                2.7                 1.6        2.0
    grad_weight (f32 MFMA)   3.6 on segments of at most a chunk or two, 0.2 - 0.3 on segments of 19 - 36 chunks

    outlier operands         f16 x 2 (default)                                   bf16 x 3       f32 MFMA
    out (forward case)       790 / 1 596 = 0.81 / 0.78 of the composite bound    11.6 / 12.5    11.6 / 12.5       (32 -> 64 / 128 -> 128)
    grad_feat (input case)   890 / 2 486 = 0.64 / 0.72 of the composite bound    14.4 / 10.8    14.4 / 10.8
    grad_weight              6.7 / 13.2 / 13.4 / 13.2 (forward 32 -> 64, input 32 -> 64, forward 128 -> 128, input 128 -> 128); with one
                             chain per 512-pair chunk, before the blocked summation: 21 - 23 / 30 - 32 / 35 - 36 / 43, and 6.3
                             on ordinary operands (float atomics between chunks: a figure moves by a unit from run to run)
"""
import numpy as np
import pytest
import torch

import subm_judge as J
from test_subm_conv import _points

pytestmark = pytest.mark.gpu

GRID = (10, 10, 6)
_truth = {}


def _operands(N, K, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, cin, generator=g), torch.randn(K ** 3, cin, cout, generator=g) * 0.1, torch.randn(N, cout, generator=g)


def _case(N, cin, cout):
    """Points, operands and float64 truth at GRID, K = 3 (points: ``_points`` with ``default_rng(21)``), computed once, only read."""
    key = (N, cin, cout)
    if key not in _truth:
        idx = _points(np.random.default_rng(21), N, 1, GRID)
        feat, weight, gout = _operands(N, 3, cin, cout, seed=100 + cin + cout // 32)
        _truth[key] = (idx, feat, weight, gout, J.Truth(feat, idx, weight, gout, 1, GRID, 3))
    return _truth[key]


def _products(gpu, idx, feat, weight, gout, batch, shape, K, rulebook=None):
    """(out, grad_feat, grad_weight, rulebook) of the device op through autograd."""
    from gaussianformer_amd.sparse_conv import Rulebook, subm_conv3d
    rb = rulebook if rulebook is not None else Rulebook(idx.to(gpu), batch, shape, K)
    fd, wd = feat.to(gpu).requires_grad_(True), weight.to(gpu).requires_grad_(True)
    out = subm_conv3d(fd, idx.to(gpu), wd, batch, shape, K, rulebook=rb)
    out.backward(gout.to(gpu))
    return out.detach().cpu(), fd.grad.cpu(), wd.grad.cpu(), rb


def _judge(what, t, out, gfeat, gweight=None, f16=True):
    """The products of one run; ``f16``: the default format (its output and input gradient get the range term)."""
    J.check(f"{what} out", out, t.out, t.mag_out, t.rng_out if f16 else None)
    J.check(f"{what} grad_feat", gfeat, t.grad_feat, t.mag_grad_feat, t.rng_grad_feat if f16 else None)
    if gweight is not None:
        J.check(f"{what} grad_weight", gweight, t.grad_weight, t.mag_grad_weight)


def _judge_other_formats(gpu, what, t, idx, feat, weight, gout, batch, shape, K, rb, out):
    """The same rulebook through the two formats with fp32's range (library options): output and input gradient to the plain
    bound (the weight gradient does not depend on the format)."""
    from gaussianformer_amd import _lib
    for option, name in (("subm.bf16x3", "bf16 x 3"), ("subm.f32_mfma", "f32 mfma")):
        with _lib.option(option, 1):
            out2, gfeat2, _, _ = _products(gpu, idx, feat, weight, gout, batch, shape, K, rulebook=rb)
        assert not torch.equal(out2, out)       # another kernel did run
        _judge(f"{what} {name}", t, out2, gfeat2, f16=False)


def _run(gpu, what, idx, feat, weight, gout, batch, shape, K):
    t = J.Truth(feat, idx, weight, gout, batch, shape, K)
    out, gfeat, gweight, rb = _products(gpu, idx, feat, weight, gout, batch, shape, K)
    _judge(what, t, out, gfeat, gweight)
    return t, gweight, rb


@pytest.mark.parametrize("cin,cout", [(ci, co) for ci in (32, 64, 128) for co in (32, 64, 128)])
def test_every_channel_pair_at_the_tile_walk(gpu, cin, cout):
    """The digest test's shape: 3 326 pairs in segments of 86 .. 478, some shorter than one tile; at 32 -> 32 and 32 -> 64 the
    weight gradient has fewer MFMA blocks than waves."""
    idx, feat, weight, gout, t = _case(300, cin, cout)
    out, gfeat, gweight, rb = _products(gpu, idx, feat, weight, gout, 1, GRID, 3)
    assert rb.total == 3326
    print()
    _judge(f"tile walk {cin}->{cout}", t, out, gfeat, gweight)
    _judge_other_formats(gpu, f"tile walk {cin}->{cout}", t, idx, feat, weight, gout, 1, GRID, 3, rb, out)


@pytest.mark.parametrize("cin,cout", [(128, 128), (64, 32), (32, 128), (32, 32)])
def test_run_walk_and_many_chunk_segments(gpu, cin, cout):
    """311 574 pairs in segments of 9 671 .. 18 328: the run walk forward AND backward (the input gradient at the swapped
    pair), 19 - 36 weight-gradient chunks per segment on the atomic path, ragged last tiles, runs and chunks."""
    idx, feat, weight, gout, t = _case(3000, cin, cout)
    out, gfeat, gweight, rb = _products(gpu, idx, feat, weight, gout, 1, GRID, 3)
    assert rb.total == 311574 and rb.total // 128 >= 27 * 32, rb.total
    print()
    _judge(f"run walk {cin}->{cout}", t, out, gfeat, gweight)
    _judge_other_formats(gpu, f"run walk {cin}->{cout}", t, idx, feat, weight, gout, 1, GRID, 3, rb, out)
    if (cin, cout) == (128, 128):
        # sized by a capacity: the gated double launch (run form and tile form, the device's count lets one of them write)
        from gaussianformer_amd.sparse_conv import Rulebook
        roomy = Rulebook(idx.to(gpu), 1, GRID, 3, pair_capacity=128 * 3000)
        out, gfeat, gweight, _ = _products(gpu, idx, feat, weight, gout, 1, GRID, 3, rulebook=roomy)
        assert roomy.check() == rb.total
        _judge("run walk 128->128, capacity rulebook", t, out, gfeat, gweight)


def test_segment_lengths_at_the_kernels_edges(gpu):
    """K = 1, points in distinct cells: the single segment has exactly N pairs -- around the weight gradient's 32-pair staging
    step and two-step prefetch (31 .. 65), the gather-GEMM's 128-pair tile, the 512-pair chunk (one chunk: plain stores; two:
    atomics), and a second tile / third chunk of one pair."""
    shape, cin, cout = (12, 12, 8), 64, 64
    rng = np.random.default_rng(5)
    print()
    for N in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1024, 1025):
        cells = rng.permutation(shape[0] * shape[1] * shape[2])[:N]
        idx = torch.from_numpy(np.stack([np.zeros(N, dtype=np.int64), cells // (shape[1] * shape[2]), (cells // shape[2]) % shape[1],
                                         cells % shape[2]], 1).astype(np.int32))
        feat, weight, gout = _operands(N, 1, cin, cout, seed=N)
        _, _, rb = _run(gpu, f"one segment of {N} pairs", idx, feat, weight, gout, 1, shape, 1)
        assert rb.total == N


@pytest.mark.parametrize("cin,cout", [(32, 32), (128, 64)])
def test_kernel_size_seven(gpu, cin, cout):
    """343 offsets (kSubmMaxK3): more segment starts than a workgroup has threads."""
    N, shape, K = 500, (7, 7, 7), 7
    idx = _points(np.random.default_rng(23), N, 1, shape)
    feat, weight, gout = _operands(N, K, cin, cout, seed=7)
    print()
    _run(gpu, f"K=7 {cin}->{cout}", idx, feat, weight, gout, 1, shape, K)


def test_empty_segments(gpu):
    """A grid one cell deep: the 18 offsets with dz != 0 have no pair; their weight-gradient slices are exactly zero."""
    N, shape, K = 200, (9, 9, 1), 3
    idx = _points(np.random.default_rng(24), N, 1, shape)
    feat, weight, gout = _operands(N, K, 32, 64, seed=8)
    print()
    t, gweight, rb = _run(gpu, "grid (9,9,1)", idx, feat, weight, gout, 1, shape, K)
    empty = [k for k in range(27) if k % 3 != 1]
    assert float(t.mag_grad_weight[empty].abs().max()) == 0.0 and float(t.mag_grad_weight[13].min()) > 0.0
    assert float(gweight[empty].abs().max()) == 0.0


def test_batch_faces_do_not_touch(gpu):
    """The last x plane of batch 0 and the first of batch 1 are neighbours in the linear cell index, not in the grid."""
    N, batch, shape, K = 300, 2, (6, 5, 4), 3
    rng = np.random.default_rng(25)
    idx = _points(rng, N, batch, shape)
    idx[10:35, 0], idx[10:35, 1] = 0, shape[0] - 1
    idx[35:60, 0], idx[35:60, 1] = 1, 0
    idx[10:60, 2:] = torch.from_numpy(np.stack([rng.integers(0, shape[1], 50), rng.integers(0, shape[2], 50)], 1).astype(np.int32))
    assert int(((idx[:, 0] == 0) & (idx[:, 1] == shape[0] - 1)).sum()) >= 20 and int(((idx[:, 0] == 1) & (idx[:, 1] == 0)).sum()) >= 20
    feat, weight, gout = _operands(N, K, 64, 64, seed=9)
    print()
    _run(gpu, "batch faces", idx, feat, weight, gout, batch, shape, K)


def test_cells_of_one_two_and_forty_points(gpu):
    shape, K = (6, 6, 4), 3
    cells = [(2, 2, 1)] * 40 + [(3, 2, 1)] * 2 + [(2, 3, 2)] * 2 + [(1, 1, 1), (4, 4, 3), (3, 3, 2), (5, 0, 0), (0, 5, 3), (2, 1, 0)]
    rng = np.random.default_rng(26)
    order = rng.permutation(len(cells))
    idx = torch.tensor([(0,) + cells[i] for i in order], dtype=torch.int32)
    N = idx.shape[0]
    feat, weight, gout = _operands(N, K, 32, 128, seed=10)
    print()
    _, _, rb = _run(gpu, "cells of 1, 2 and 40 points", idx, feat, weight, gout, 1, shape, K)
    assert rb.total >= 40 * 40 + 2 * 40 * 2


def _outlier_case(cin, cout, which):
    """One channel per row and one input channel per weight column raised by 2^16 .. 2^26, half of the columns thinned
    (``subm_judge.outlier_operands``).  ``forward``: the outliers sit in ``feat`` and the columns of ``W``; ``input_gradient``:
    in ``grad_out`` and the input-channel rows of ``W`` -- the columns of the call the backward makes."""
    key = ("outlier", cin, cout, which)
    if key not in _truth:
        o = J.OUTLIER_GEOMETRY
        N, batch, shape, K = o["N"], o["batch"], o["shape"], o["K"]
        idx = J.outlier_points()
        if which == "forward":
            feat, weight = J.outlier_operands(N, cin, K ** 3, cout, seed=41)
            gout = _operands(N, K, cin, cout, seed=11)[2]
        else:
            gout, wt = J.outlier_operands(N, cout, K ** 3, cin, seed=43)
            weight = wt.flip(0).transpose(1, 2).contiguous()                 # so that W.flip(0).transpose(1, 2) is ``wt``
            feat = _operands(N, K, cin, cout, seed=11)[0]
        _truth[key] = (idx, feat, weight, gout, J.Truth(feat, idx, weight, gout, batch, shape, K), (batch, shape, K))
    return _truth[key]


@pytest.mark.parametrize("which", ["forward", "input_gradient"])
@pytest.mark.parametrize("cin,cout", [(32, 64), (128, 128)])
def test_f16_contract_where_it_bites(gpu, cin, cout, which):
    """The small elements of a row (column) with one raised channel lose their lo terms to f16's subnormal spacing, and the
    default format's contract is the COMPOSITE bound: 19 - 42 % of the elements lie beyond ``2^-20 mag`` (worst 790 - 2 486
    units) and all are within 0.64 - 0.81 of the composite bound -- the matrix cores do honour f16 subnormal inputs (a kernel
    that flushed them would miss it several hundredfold: tests/test_subm_judge.py).  The formats with fp32's range keep the
    plain bound (measured 10.8 - 14.4 units on the side that carries the outliers)."""
    idx, feat, weight, gout, t, geo = _outlier_case(cin, cout, which)
    print()
    out, gfeat, _, rb = _products(gpu, idx, feat, weight, gout, *geo)
    got, ref, mag = (out, t.out, t.mag_out) if which == "forward" else (gfeat, t.grad_feat, t.mag_grad_feat)
    beyond = J.fraction_beyond_plain(got, ref, mag)
    print(f"f16 x 2, {which}: {100 * beyond:.1f} % of the elements beyond 2^-20 mag alone")
    _judge(f"outliers ({which}) {cin}->{cout} f16 x 2", t, out, gfeat)
    assert beyond > 0.10                       # the case is in the regime it claims
    _judge_other_formats(gpu, f"outliers ({which}) {cin}->{cout}", t, idx, feat, weight, gout, *geo, rb, out)


@pytest.mark.parametrize("which", ["forward", "input_gradient"])
@pytest.mark.parametrize("cin,cout", [(32, 64), (128, 128)])
def test_weight_gradient_of_outlier_operands(gpu, cin, cout, which):
    """The weight gradient of the cases above, to ``2^-20 mag`` like every other weight gradient of this file: 6.7 - 13.4 units.

    This test found a defect.  ``gf_subm_wgrad_kernel`` summed a chunk's 512 pairs in ONE chain of f32 MFMAs
    (bitwise an fmaf chain); where a few products dominate ``sum |a||b|`` of an element every later pair rounds at the size of
    the whole sum -- about 0.4 units rms per pair, 0.4 sqrt(n) per chain, the worst of 10^5 elements at 4.5 sigma: 1.9 sqrt(512)
    = 43 -- and it measured 21 - 23, 30 - 32, 35 - 36 and 43 units on these four cases (the same chains in numpy fp32: 24.7 and
    52.8).  Now a step's 32 pairs are summed from zero and the steps' sums added (32 + 16 roundings and the segment's one to
    four chunks here; the numpy restatement of that: 11.9 and 13.5)."""
    idx, feat, weight, gout, t, geo = _outlier_case(cin, cout, which)
    print()
    _, _, gweight, _ = _products(gpu, idx, feat, weight, gout, *geo)
    J.check(f"outliers ({which}) {cin}->{cout} grad_weight", gweight, t.grad_weight, t.mag_grad_weight)


def test_one_wrong_pair_on_the_device_fails_the_weight_gradient(gpu):
    """The judgement sees ONE pair of 18 328: ``pair_in`` overwritten at one slot in the middle of the longest segment with
    another point of the same set (inside [0, N)), nothing else changed."""
    from gaussianformer_amd.sparse_conv import Rulebook
    N = 3000
    idx, feat, weight, gout, t = _case(N, 64, 32)
    rb = Rulebook(idx.to(gpu), 1, GRID, 3)
    fd, gd = feat.to(gpu), gout.to(gpu)
    r, at = J.worst(rb.weight_grad(fd, gd), t.grad_weight, t.mag_grad_weight)
    assert r <= 1.0, (r, at)
    pin, po = rb.pair_in[:rb.total].cpu().long(), rb.pair_out[:rb.total].cpu().long()
    d = idx.long()[pin, 1:] - idx.long()[po, 1:]                        # offset of a pair: cell(in) - cell(out)
    k_of = ((d[:, 0] + 1) * 3 + d[:, 1] + 1) * 3 + d[:, 2] + 1
    assert bool((k_of[1:] >= k_of[:-1]).all())                          # the pairs are grouped by offset, ascending
    counts = torch.bincount(k_of, minlength=27)
    k = int(counts.argmax())
    assert int(counts[k]) == 18328 and k == 13
    slot = int((k_of < k).sum()) + int(counts[k]) // 2
    old = int(pin[slot])
    new = (old + N // 2) % N
    rb.pair_in[slot] = new
    r, at = J.worst(rb.weight_grad(fd, gd), t.grad_weight, t.mag_grad_weight)
    print(f"\npair_in[{slot}]: {old} -> {new}: err/bound {r:.1f} at {at}")
    assert r > 1.0 and at[0] == k, (r, at)
    others = [j for j in range(27) if j != k]
    assert J.worst(rb.weight_grad(fd, gd)[others], t.grad_weight[others], t.mag_grad_weight[others])[0] <= 1.0
