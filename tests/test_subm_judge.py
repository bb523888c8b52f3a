"""The sparse convolution's element-by-element judgement (tests/subm_judge.py) itself, on the CPU: it accepts what a correct
kernel computes and rejects what the tensor-wide bounds of tests/test_subm_conv.py let through.

(1) The two-term f16 format restated in numpy (hi, lo as numpy float16 under the row / column scales, ``hi.hi + hi.lo + lo.hi``
in float64) on operands whose large elements do not dominate sum |a||b|: with IEEE subnormals it meets the composite bound
``2^-20 mag + 2 * 2^-39 rng`` (measured: 0.37 - 0.39 of the bound; the second constant would have to be 0.64 - 0.75), with f16
subnormals flushed to zero it misses it several hundredfold (371 - 738 x the bound) -- and 19 - 42 % of its elements lie beyond
``2^-20 mag`` alone (worst 790 - 1 595 units of 2^-24 mag), so the case is in the regime it claims.
(2) One product ``feat[j] . W[k]`` missing from one output row, and one pair's outer product missing from a weight-gradient
segment of more than 10 000 pairs, fail the plain bound, and the judgement names the row (the offset) they were taken from."""
import numpy as np
import pytest
import torch

import subm_judge as J
from test_subm_conv import _points

_cache = {}


def _outlier(cin, cout):
    """(operands, float64 truth, yardsticks, emulations) of the outlier case, computed once and only read."""
    key = ("outlier", cin, cout)
    if key not in _cache:
        o = J.OUTLIER_GEOMETRY
        geo = (o["batch"], o["shape"], o["K"])
        idx = J.outlier_points().long()
        a, w = J.outlier_operands(o["N"], cin, o["K"] ** 3, cout, seed=41)
        a64, w64 = a.double(), w.double()
        ref = J.D(a64, idx, w64, *geo)
        mag = J.D(a64.abs(), idx, w64.abs(), *geo)
        rng = J._rng(a64, idx, w64, *geo)
        ieee = J.f16_emulated(a, idx, w, *geo)
        flushed = J.f16_emulated(a, idx, w, *geo, flush=True)
        _cache[key] = (ref, mag, rng, ieee, flushed)
    return _cache[key]


@pytest.mark.parametrize("cin,cout", [(32, 64), (128, 128)])
def test_composite_bound_separates_ieee_subnormals_from_flushed_ones(cin, cout):
    ref, mag, rng, ieee, flushed = _outlier(cin, cout)
    beyond = J.fraction_beyond_plain(ieee, ref, mag)
    r_ieee, at = J.worst(ieee, ref, mag, rng)
    r_flushed, at_f = J.worst(flushed, ref, mag, rng)
    print(f"\n{cin}->{cout}: {100 * beyond:.1f} % beyond 2^-20 mag (worst {J.units(ieee, ref, mag):.0f} units); err/bound "
          f"IEEE {r_ieee:.3f} at {at}, flushed {r_flushed:.1f} at {at_f}")
    assert beyond > 0.10                      # the case is in the regime it claims: the plain bound does not hold here ...
    assert J.worst(ieee, ref, mag)[0] > 1.0
    assert r_ieee <= 1.0                      # ... the documented contract does ...
    assert r_flushed > 100.0                  # ... and lost subnormal lo terms are two orders of magnitude outside it
    # the formats with fp32's range are judged by the plain bound: the truth itself passes it, trivially
    assert J.worst(ref, ref, mag)[0] == 0.0


def _ordinary():
    """The many-chunk shape of the GPU tests (N = 3000 on a (10, 10, 6) grid, K = 3, 64 -> 32) with its pairs listed on the CPU."""
    if "ordinary" not in _cache:
        N, batch, shape, K, cin, cout = 3000, 1, (10, 10, 6), 3, 64, 32
        idx = _points(np.random.default_rng(21), N, batch, shape)
        g = torch.Generator().manual_seed(3)
        feat = torch.randn(N, cin, generator=g)
        weight = torch.randn(K ** 3, cin, cout, generator=g) * 0.1
        gout = torch.randn(N, cout, generator=g)
        _cache["ordinary"] = (J.Truth(feat, idx, weight, gout, batch, shape, K), idx.long())
    return _cache["ordinary"]


def _pairs_of_offset(idx, shape, d):
    """(out i, in j) with cell(j) = cell(i) + d, both inside the grid."""
    X, Y, Z = shape
    cells = {}
    for n, c in enumerate(idx.tolist()):
        if 0 <= c[1] < X and 0 <= c[2] < Y and 0 <= c[3] < Z:
            cells.setdefault(tuple(c), []).append(n)
    return [(i, j) for c, members in cells.items() for i in members
            for j in cells.get((c[0], c[1] + d[0], c[2] + d[1], c[3] + d[2]), ())]


def test_one_missing_product_fails_the_plain_bound():
    t, idx = _ordinary()
    batch, shape, K = t.geo
    assert J.worst(t.out, t.out, t.mag_out)[0] == 0.0
    k = 5                                                    # offset (-1, 0, +1)
    d = (k // 9 - 1, (k // 3) % 3 - 1, k % 3 - 1)
    i, j = _pairs_of_offset(idx, shape, d)[7]
    mut = t.out.clone()
    mut[i] -= t.feat[j] @ t.weight[k]
    r, at = J.worst(mut, t.out, t.mag_out)
    assert r > 1.0 and at[0] == i, (r, at)
    # the input gradient likewise: the same pair carries grad_out[i] . W[k]^T to row j
    mut = t.grad_feat.clone()
    mut[j] -= t.weight[k] @ t.grad_out[i]
    r, at = J.worst(mut, t.grad_feat, t.mag_grad_feat)
    assert r > 1.0 and at[0] == j, (r, at)


def test_one_missing_pair_of_a_long_segment_fails_the_weight_gradient():
    t, idx = _ordinary()
    batch, shape, K = t.geo
    k = 13                                                   # the centre offset: every point with every point of its cell
    pairs = _pairs_of_offset(idx, shape, (0, 0, 0))
    assert len(pairs) >= 10000, len(pairs)
    assert J.worst(t.grad_weight, t.grad_weight, t.mag_grad_weight)[0] == 0.0
    i, j = pairs[len(pairs) // 2]
    mut = t.grad_weight.clone()
    mut[k] -= torch.outer(t.feat[j], t.grad_out[i])
    r, at = J.worst(mut, t.grad_weight, t.mag_grad_weight)
    print(f"\none of {len(pairs)} pairs missing: err/bound {r:.1f} at {at}; "
          f"tensor-wide {float((mut - t.grad_weight).abs().max() / t.grad_weight.abs().max()):.2e} of max|gw|")
    assert r > 1.0 and at[0] == k, (r, at)
    # and not by its largest element only: most elements of the pair's outer product are outside their bounds
    outside = (torch.outer(t.feat[j], t.grad_out[i]).abs() > J.bound(t.mag_grad_weight[k])).double().mean()
    assert float(outside) > 0.9, float(outside)


def test_f16_split_restatement():
    """The numpy split itself: hi + lo is x to 2^-22 |x| + 2^-39 max per row, scales are exact, a zero row stays zero."""
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(64, 32, generator=g) * torch.exp2(torch.randint(-30, 30, (64, 32), generator=g).float())).numpy()
    x[5] = 0.0
    hi, lo = J.f16_split(x, 1)
    m = np.abs(x).max(axis=1, keepdims=True).astype(np.float64)
    assert (np.abs(hi + lo - x) <= 2.0 ** -22 * np.abs(x) + 2.0 ** -39 * m).all()
    assert (hi[5] == 0).all() and (lo[5] == 0).all()
    hf, lf = J.f16_split(x, 1, flush=True)
    assert (np.abs(hf + lf - x) > 2.0 ** -22 * np.abs(x) + 2.0 ** -39 * m).any()
