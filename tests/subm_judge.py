"""The element-by-element judgement of the submanifold sparse convolution's three products (plain module, CPU, fp64).

Yardsticks come from ``oracle.subm_ref.subm_conv3d_dense`` (``D`` below) in float64:

* ``mag`` = sum |a||b| per element of a product: ``D(|feat|, |W|)`` for the output, and for the two gradients the float64 autograd
  gradients of ``D(|feat|, |W|)`` under ``|grad_out|``.
* ``rng`` (the default two-term f16 format only; output and input gradient) = ``D(A, |W|) + D(|feat|, B)`` with ``A[j, :] =
  max_c |feat[j, c]|`` and ``B[k, :, o] = max_c |W[k, c, o]|``; for the input gradient the same expression on ``(grad_out,
  W.flip(0).transpose(1, 2))``, which is the call the backward makes.

The bound of an element is ``2^-20 mag + 2 * 2^-39 rng + tiny``:

* ``2^-20`` is 16 units of fp32 roundoff of sum |a||b| -- the bound ``test_subm_conv_bf16_split_against_f32_mfma`` uses (DESIGN
  §3.7 records the three formats at 3.1 - 5.5 units; a float32 CPU evaluation of ``step_ref.subm_conv_sparse`` errs up to 3.04).
* the second term is the f16 format's RANGE (include/gf_hip.h): a row of the features and a column of a weight slice
  are scaled so that their largest magnitude lies in [2^14, 2^15), so the split of an operand errs by at most ``2^-22 |x| + 2^-39
  max`` (f16's subnormal spacing 2^-24, half of it, over 2^14).  With a' = a + da, b' = b + db the product sum errs by
  ``sum |da||b| + |a||db|`` (+ second order): the three ``2^-22`` terms -- da, db and the dropped lo.lo -- are inside ``2^-20 mag``,
  the two range terms are ``2^-39 (A |b| + |a| B)`` once each -- together ``2^-39 rng``.  The constant 2 gives that first-order
  count one binade: for the second-order terms, and for the fp32 accumulation of sums that ``mag`` no longer measures where the
  range term is the larger one.  It is derived, not fitted: on the outlier operands the numpy emulation below (exact
  accumulation) needs 0.64 - 0.75 in its place, the same emulation with f16 subnormals flushed to zero 750 - 1 480, and the
  kernels on an MI355X come to 0.64 - 0.81 of the whole bound.
  ``subm.bf16x3``, ``subm.f32_mfma`` and the weight gradient (f32 MFMA) have fp32's range: ``2^-20 mag`` alone.
* ``tiny`` = 1e-30 (2^-120 where products underflow fp32), as in tests/test_subm_conv.py.

``worst`` returns the largest ``err / bound`` and where it is, so a failure names the element.  The module also holds the numpy
emulation of the f16 split (hi, lo as numpy float16; ``hi.hi + hi.lo + lo.hi`` evaluated in float64 through ``D``) and the
outlier operands on which the range term bites -- shared by tests/test_subm_judge.py (CPU) and tests/test_subm_truth_gpu.py."""
import numpy as np
import torch

from oracle.subm_ref import subm_conv3d_dense as D

UNIT = 2.0 ** -24          # one unit of fp32 roundoff
PLAIN = 2.0 ** -20         # 16 units: the bound on sum |a||b|
RANGE = 2.0 * 2.0 ** -39   # the f16 format's range term, on rng
TINY = 1e-30


class Truth:
    """float64 truth and yardsticks of one case, computed once: ``out``, ``grad_feat``, ``grad_weight``, their ``mag_*``, and
    ``rng_out`` / ``rng_grad_feat``."""

    def __init__(self, feat, idx, weight, grad_out, batch, shape, K):
        idx = idx.long()
        geo = (batch, shape, K)
        f, w, g = feat.double(), weight.double(), grad_out.double()
        f1, w1 = f.clone().requires_grad_(True), w.clone().requires_grad_(True)
        out = D(f1, idx, w1, *geo)
        self.grad_feat, self.grad_weight = torch.autograd.grad(out, (f1, w1), g)
        self.out = out.detach()
        fa, wa = f.abs().requires_grad_(True), w.abs().requires_grad_(True)
        mag = D(fa, idx, wa, *geo)
        self.mag_grad_feat, self.mag_grad_weight = torch.autograd.grad(mag, (fa, wa), g.abs())
        self.mag_out = mag.detach()
        self.rng_out = _rng(f, idx, w, *geo)
        self.rng_grad_feat = _rng(g, idx, w.flip(0).transpose(1, 2), *geo)
        self.feat, self.weight, self.grad_out, self.idx, self.geo = f, w, g, idx, geo


def _rng(a, idx, w, batch, shape, K):
    A = a.abs().amax(dim=1, keepdim=True).expand_as(a)
    B = w.abs().amax(dim=1, keepdim=True).expand_as(w)
    return D(A, idx, w.abs(), batch, shape, K) + D(a.abs(), idx, B, batch, shape, K)


def bound(mag, rng=None, tiny=TINY):
    b = PLAIN * mag + tiny
    return b if rng is None else b + RANGE * rng


def worst(got, ref, mag, rng=None, tiny=TINY):
    """(largest err / bound, its index) over the elements; a non-finite element counts as infinitely wrong."""
    got = torch.as_tensor(got).detach().cpu().double()
    err = (got - ref).abs()
    ratio = torch.where(torch.isfinite(err), err / bound(mag, rng, tiny), torch.full_like(err, float("inf")))
    flat = int(ratio.argmax())
    return float(ratio.flatten()[flat]), tuple(int(v) for v in np.unravel_index(flat, tuple(ratio.shape)))


def units(got, ref, mag):
    """Largest error in units of 2^-24 sum |a||b| (over the elements with a non-zero yardstick)."""
    got = torch.as_tensor(got).detach().cpu().double()
    live = mag > 0
    if not bool(live.any()):
        return 0.0
    return float(((got - ref).abs()[live] / (UNIT * mag[live])).max())


def fraction_beyond_plain(got, ref, mag, tiny=TINY):
    """Share of the elements whose error is NOT within 2^-20 sum |a||b| alone."""
    got = torch.as_tensor(got).detach().cpu().double()
    return float(((got - ref).abs() > bound(mag, None, tiny)).double().mean())


def check(what, got, ref, mag, rng=None, tiny=TINY):
    """Prints the worst error in units of 2^-24 sum |a||b| and asserts the bound element by element; returns the units."""
    u = units(got, ref, mag)
    r, at = worst(got, ref, mag, rng, tiny)
    print(f"{what}: worst {u:.2f} units of 2^-24 sum|a||b|, err/bound {r:.3f} at {at}")
    assert r <= 1.0, f"{what}: element {at} errs {r:.3g} x its bound ({u:.3g} units)"
    return u


# ---- the f16 two-term split, restated in numpy -----------------------------------------------------------------------------

def f16_split(x, axis, flush=False):
    """``x`` (float32 array) as hi + lo in numpy float16 under an exact power-of-two scale per slice along ``axis`` (the
    slice's largest |x| brought to [2^14, 2^15)), returned unscaled in float64.  ``flush``: f16 subnormals read as zero."""
    x = np.asarray(x, dtype=np.float32)
    m = np.abs(x).max(axis=axis, keepdims=True)
    E = np.clip(np.frexp(m)[1].astype(np.int32) - 1, -126, 127)
    e = 14 - E
    xs = np.ldexp(x, e).astype(np.float32)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    if flush:
        smallest_normal = np.float16(2.0 ** -14)
        hi = np.where(np.abs(hi) < smallest_normal, np.float16(0), hi)
        lo = np.where(np.abs(lo) < smallest_normal, np.float16(0), lo)
    return np.ldexp(hi.astype(np.float64), -e), np.ldexp(lo.astype(np.float64), -e)


def f16_emulated(a, idx, w, batch, shape, K, flush=False):
    """What the f16 format computes with exact accumulation: rows of ``a`` and columns of every ``w[k]`` split, then
    ``hi.hi + hi.lo + lo.hi`` in float64."""
    ah, al = (torch.from_numpy(v) for v in f16_split(a.float().numpy(), 1, flush))
    wh, wl = (torch.from_numpy(v) for v in f16_split(w.float().numpy(), 1, flush))
    geo = (batch, shape, K)
    return D(ah, idx, wh, *geo) + D(ah, idx, wl, *geo) + D(al, idx, wh, *geo)


# ---- operands on which the range term bites --------------------------------------------------------------------------------

OUTLIER_GEOMETRY = dict(N=400, batch=2, shape=(5, 4, 3), K=3)


def outlier_operands(N, cin, K3, cout, seed):
    """``a [N, cin]`` with one channel per row and ``w [K3, cin, cout]`` with one input channel per (k, column) raised by
    2^16 .. 2^26, and every second weight column thinned to about 50 % zeros: large elements that do NOT dominate
    sum |a||b| of every output element, so the small ones' lost lo terms show."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(N, cin, generator=g)
    ch = torch.randint(0, cin, (N,), generator=g)
    a[torch.arange(N), ch] *= torch.exp2(torch.randint(16, 27, (N,), generator=g).float())
    w = torch.randn(K3, cin, cout, generator=g) * 0.1
    keep = (torch.rand(K3, cin, cout, generator=g) < 0.5).float()
    keep[:, :, ::2] = 1.0
    w = w * keep
    cw = torch.randint(0, cin, (K3, 1, cout), generator=g)
    up = torch.exp2(torch.randint(16, 27, (K3, 1, cout), generator=g).float())
    w.scatter_(1, cw, w.gather(1, cw) * up)
    return a, w


def outlier_points(seed=31):
    """Points of OUTLIER_GEOMETRY: uniform cells (3.3 points per cell), two of them outside the grid."""
    o = OUTLIER_GEOMETRY
    rng = np.random.default_rng(seed)
    X, Y, Z = o["shape"]
    N = o["N"]
    idx = np.stack([rng.integers(0, o["batch"], N), rng.integers(0, X, N), rng.integers(0, Y, N), rng.integers(0, Z, N)], 1)
    idx[:2, 1] = X + 3
    return torch.from_numpy(idx.astype(np.int32))
