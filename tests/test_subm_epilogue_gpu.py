"""The sparse convolution's epilogue on the GPU: ``gf_subm_conv_apply_epilogue`` (the raw entry point) and ``Rulebook.apply``
with ``bias`` / ``residual`` / ``norm`` / ``relu``.

Without an epilogue the bytes are the plain call's, digest for digest.  The parts that are single correctly rounded adds are
held with ``==``.  The LayerNorm parts are held to the float64 restatement applied to the NATIVE convolution output ``c`` (so only
the epilogue is judged) by DESIGN.md §3.13b's rule, ``max|native - truth| <= 2 Y + 4 eps32 max|truth|`` with Y the error of
torch's float32 composition on the same ``c``; the sample is all 3001 x Cout values of a case."""
import functools
import hashlib
import json

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from gaussianformer_amd import _lib
from gaussianformer_amd.sparse_conv import Rulebook
from row_judge import Guarded, bound, held, max_error, spy  # noqa: F401  (spy is a fixture)
from test_subm_conv import _points
from test_subm_gemm_digests import GOLDEN, K, SHAPE, case_name

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHANNELS = [(128, 128), (64, 32)]
N_ODD = 3001          # not a multiple of the 8 (Cout = 128) or 32 (Cout = 32) rows of a reduce workgroup


def raw_call(rb, feat, weight, out, bias=None, residual=None, ln_weight=None, ln_bias=None, relu=0):
    """The C entry point on a caller-made ``out``."""
    cin, cout = weight.shape[1], weight.shape[2]
    partial = torch.empty(max(rb.total, 1), cout, device=DEV)
    nscratch = int(_lib.load().gf_subm_apply_scratch_bytes(rb.N, cin))
    scratch = torch.empty(max(nscratch, 16), dtype=torch.uint8, device=DEV)
    _lib.call("gf_subm_conv_apply_epilogue", DEV, *rb.dims, cin, cout, rb.total, feat, weight, rb.tables, rb.pair_in, partial, out,
              scratch, nscratch, bias, residual, ln_weight, ln_bias, relu)
    return out


def digest_draws(N, cin, cout):
    """``test_subm_gemm_digests.compute``'s inputs (the same generator, the same order of draws)."""
    rng = np.random.default_rng(21)
    idx = _points(rng, N, 1, SHAPE).to(DEV)
    feat = rng.integers(-2 ** 23, 2 ** 23, (N, cin)) * 2.0 ** rng.integers(-30, -17, (N, cin))
    weight = rng.integers(-2 ** 23, 2 ** 23, (K ** 3, cin, cout)) * 2.0 ** rng.integers(-34, -23, (K ** 3, cin, cout))
    return idx, torch.from_numpy(feat.astype(np.float32)).to(DEV), torch.from_numpy(weight.astype(np.float32)).to(DEV)


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("N", [3000, 300])
def test_without_an_epilogue_the_bytes_are_the_plain_calls(N, cin, cout):
    idx, feat, weight = digest_draws(N, cin, cout)
    rb = Rulebook(idx, 1, SHAPE, K)
    plain = rb.apply(feat, weight)
    out = raw_call(rb, feat, weight, torch.full((N, cout), 7.0, device=DEV))
    assert torch.equal(out.view(torch.int32), plain.view(torch.int32))
    with open(GOLDEN) as f:
        want = json.load(f)[case_name(N, cin, cout)]["f16x2"]
    assert hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest() == want
    assert hashlib.sha256(plain.cpu().numpy().tobytes()).hexdigest() == want


class Case:
    """N = 3001 points on the digest test's grid, their plain output ``c`` and the epilogue's operands; the first two points lie
    outside the grid, and every point with x <= 3 has zero features, so the points with x <= 2 see nothing but zeros."""

    def __init__(self, cin, cout):
        rng = np.random.default_rng(5)
        idx = _points(rng, N_ODD, 1, SHAPE)
        g = torch.Generator().manual_seed(cin + cout)
        feat = torch.randn(N_ODD, cin, generator=g)
        feat[idx[:, 1] <= 3] = 0
        self.outside = (idx[:, 1] >= SHAPE[0]).to(DEV)
        self.dark = (idx[:, 1] <= 2).to(DEV)
        assert int(self.outside.sum()) == 2 and int(self.dark.sum()) > 100
        self.idx, self.feat = idx.to(DEV), feat.to(DEV)
        self.weight = (torch.randn(K ** 3, cin, cout, generator=g) * 0.1).to(DEV)
        self.bias = torch.randn(cout, generator=g).to(DEV)
        self.residual = torch.randn(N_ODD, cout, generator=g).to(DEV)
        self.gamma = (1 + 0.5 * torch.randn(cout, generator=g)).to(DEV)
        self.beta = torch.randn(cout, generator=g).to(DEV)
        self.rb = Rulebook(self.idx, 1, SHAPE, K)
        self.c = self.rb.apply(self.feat, self.weight)
        self.cout = cout

    def compose(self, parts, dtype):
        """``relu?(LN?((c + bias) + residual))`` in ``dtype`` on the native ``c``."""
        t = lambda v: v.to(dtype)
        x = t(self.c)
        if "bias" in parts:
            x = x + t(self.bias)
        if "residual" in parts:
            x = x + t(self.residual)
        if "norm" in parts:
            x = F.layer_norm(x, (self.cout,), t(self.gamma), t(self.beta), 1e-5)
        return torch.relu(x) if "relu" in parts else x

    def native(self, parts, rb=None):
        return (rb or self.rb).apply(self.feat, self.weight, bias=self.bias if "bias" in parts else None,
                                     residual=self.residual if "residual" in parts else None,
                                     norm=(self.gamma, self.beta) if "norm" in parts else None, relu="relu" in parts)


@functools.lru_cache(maxsize=None)
def case(cin, cout):
    return Case(cin, cout)


EXACT = [("bias",), ("residual",), ("relu",), ("bias", "residual", "relu")]
NORMED = [("norm",), ("bias", "norm", "relu"), ("residual", "norm"), ("bias", "residual", "norm", "relu")]


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("parts", EXACT, ids="+".join)
def test_exact_parts(parts, cin, cout, spy):
    c = case(cin, cout)
    del spy[:]
    got = c.native(parts)
    assert spy == ["gf_subm_conv_apply_epilogue"]
    want = c.compose(parts, torch.float32)
    assert got.shape == want.shape and bool((got == want).all())
    assert c.c.abs().max() > 0 and bool((want != c.c).any())


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("parts", NORMED, ids="+".join)
def test_layernorm_parts(parts, cin, cout):
    c = case(cin, cout)
    got = c.native(parts)
    truth, torch32 = c.compose(parts, torch.float64), c.compose(parts, torch.float32)
    held(f"epilogue {'+'.join(parts)} {cin}x{cout}", got, truth, bound(max_error(torch32, truth), truth))
    # an nn.LayerNorm is the same call
    ln = nn.LayerNorm(cout).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(c.gamma)
        ln.bias.copy_(c.beta)
        again = c.rb.apply(c.feat, c.weight, bias=c.bias if "bias" in parts else None,
                           residual=c.residual if "residual" in parts else None, norm=ln, relu="relu" in parts)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_a_rows_bits_do_not_depend_on_its_place(cin, cout):
    """The same point set in reverse order: every row's bits move with the row (another workgroup, another lane group)."""
    c = case(cin, cout)
    parts = ("bias", "residual", "norm", "relu")
    rb = Rulebook(c.idx.flip(0).contiguous(), 1, SHAPE, K)
    plain = rb.apply(c.feat.flip(0).contiguous(), c.weight)
    full = rb.apply(c.feat.flip(0).contiguous(), c.weight, bias=c.bias, residual=c.residual.flip(0).contiguous(),
                    norm=(c.gamma, c.beta), relu=True)
    same = (plain.flip(0).view(torch.int32) == c.c.view(torch.int32)).all(1)     # rows whose convolution bits did not move
    assert int(same.sum()) > 100
    assert torch.equal(full.flip(0)[same].view(torch.int32), c.native(parts)[same].view(torch.int32))


@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_nothing_is_written_beyond_out_and_the_inputs_stay(cin, cout):
    c = case(cin, cout)
    keep = [t.clone() for t in (c.residual, c.bias, c.gamma, c.beta, c.feat, c.weight)]
    g = Guarded(N_ODD * cout * 4, DEV, 1 << 16, sentinel=-77.0)
    out = raw_call(c.rb, c.feat, c.weight, g.floats(N_ODD, cout), c.bias, c.residual, c.gamma, c.beta, 1)
    torch.cuda.synchronize()
    assert g.intact()
    assert torch.equal(out.view(torch.int32), c.native(("bias", "residual", "norm", "relu")).view(torch.int32))
    for t, k in zip((c.residual, c.bias, c.gamma, c.beta, c.feat, c.weight), keep):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))


@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_rows_without_any_input(cin, cout):
    """Points outside the grid and points whose own and neighbours' features are all zero: ``c`` is exactly 0 there."""
    c = case(cin, cout)
    rows = c.outside | c.dark
    assert not c.c[rows].any()
    got = c.native(("norm",))[rows]
    assert torch.equal(got.view(torch.int32), c.beta.expand_as(got).contiguous().view(torch.int32))      # LN(0) = ln_bias, bit for bit
    got = c.native(("bias", "norm"))[rows]
    assert bool((got.view(torch.int32) == got[0].view(torch.int32)).all())                                # one row, whatever its place
    truth = F.layer_norm(c.bias.double(), (cout,), c.gamma.double(), c.beta.double(), 1e-5)
    torch32 = F.layer_norm(c.bias, (cout,), c.gamma, c.beta, 1e-5)
    held(f"LN(bias) {cin}x{cout}", got[0], truth, bound(max_error(torch32, truth), truth))


@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_an_over_capacity_rulebook_gives_nan_everywhere(cin, cout):
    c = case(cin, cout)
    rb = Rulebook(c.idx, 1, SHAPE, K, pair_capacity=1)
    out = c.native(("bias", "norm", "relu"), rb)
    assert out.shape == (N_ODD, cout) and bool(torch.isnan(out).all())
    assert bool(torch.isnan(c.native(("relu",), rb)).all()) and bool(torch.isnan(c.native(("bias", "residual"), rb)).all())
    with pytest.raises(RuntimeError, match="pair_capacity"):
        rb.check()


def test_refusals_of_the_python_call():
    c = case(64, 32)
    for bad in (nn.LayerNorm(32, eps=1e-6).to(DEV), nn.LayerNorm(32, elementwise_affine=False).to(DEV), nn.BatchNorm1d(32).to(DEV),
                (c.gamma,), (c.gamma, None)):
        with pytest.raises(ValueError, match="norm"):
            c.rb.apply(c.feat, c.weight, norm=bad)
    with pytest.raises(ValueError, match="bias"):
        c.rb.apply(c.feat, c.weight, bias=c.bias[:16])
    with pytest.raises(ValueError, match="residual"):
        c.rb.apply(c.feat, c.weight, residual=c.residual[:-1])
    # the library's own refusal on device pointers: out is left alone
    out = torch.full((N_ODD, 32), 3.0, device=DEV)
    with pytest.raises(RuntimeError, match="aliases residual"):
        raw_call(c.rb, c.feat, c.weight, out, residual=out)
    with pytest.raises(RuntimeError, match="relu = 2"):
        raw_call(c.rb, c.feat, c.weight, out, relu=2)
    with pytest.raises(RuntimeError, match="bias = .* is not 16-byte aligned"):
        raw_call(c.rb, c.feat, c.weight, out, bias=torch.zeros(36, device=DEV)[1:33])
    with pytest.raises(RuntimeError, match="ln_weight"):
        raw_call(c.rb, c.feat, c.weight, out, ln_weight=c.gamma)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


def test_graph_replay_equals_eager():
    c = case(128, 128)
    rb = Rulebook(c.idx, 1, SHAPE, K, pair_capacity=128 * N_ODD)      # (sized by a capacity: both gather-GEMM walks are launched)
    feat = c.feat.clone()

    def call():
        return rb.apply(feat, c.weight, bias=c.bias, residual=c.residual, norm=(c.gamma, c.beta), relu=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for scale in (1.0, -0.5):
        feat.copy_(c.feat * scale)
        graph.replay()
        got = out.clone()
        assert torch.equal(got.view(torch.int32), call().view(torch.int32))
        assert bool(torch.isfinite(got).all()) and got.abs().max() > 0
