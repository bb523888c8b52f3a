"""The sparse convolution stage's native training step on the GPU: the saving forward
(``gf_subm_conv_apply_epilogue_train``), the stage backward in its standalone form (``gf_subm_stage_backward``) and inside the
data-gradient convolution (``gf_subm_conv_apply_stage_backward``), ``subm_stage`` / ``subm_stages`` above them and
``SparseConv3D.native_training`` above those.

What is bitwise: the saving forward's ``out`` against the epilogue entry's, ``pre`` against torch's fp32 adds on the native
convolution, the two forms of the backward against each other, a graph replay against eager, the module against the functional
chain.  What is held to float64 (``tests/subm_stage_ref.py``, DESIGN.md §3.13b's rule through ``row_judge.judge_leaves``): the
standalone backward on kink-free rows, and the block's gradients against the truth that takes the ReLUs' sides as the native
route took them."""
import functools
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import row_ref
import subm_stage_ref as ref
from gaussianformer_amd import _lib
from gaussianformer_amd.sparse_conv import Rulebook, SubMConv3d, subm_stage, subm_stages
from row_judge import Guarded, judge_leaves, max_error, spy  # noqa: F401  (spy is a fixture)
from test_sparse_block_tail_gpu import BS, BUILD, E, G, block
from test_sparse_block_tail_gpu import K as BLOCK_K
from test_subm_conv import _points
from test_subm_gemm_digests import K, SHAPE

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHANNELS = [(128, 128), (64, 32)]
N_ODD = 3001          # not a multiple of the 8 (Cout = 128) or 32 (Cout = 32) rows of a workgroup
GUARD = 1 << 16
MASK_MARGIN = 1e-4    # test 7's margin: >= 10 x the largest measured stage error


def sizes(n, cout):
    return _lib.train_sizes("gf_subm_stage_train_sizes", n, cout)


def bits(t):
    return t.contiguous().view(torch.int32)


class Case:
    """N points on the digest test's grid (the first two outside it, a tenth sharing cells) and a stage's operands."""

    def __init__(self, N, cin, cout):
        rng = np.random.default_rng(5 + N)
        self.idx = _points(rng, N, 1, SHAPE).to(DEV)
        g = torch.Generator().manual_seed(N + cin + cout)
        r = lambda *shape: torch.randn(*shape, generator=g)
        self.feat, self.weight = r(N, cin).to(DEV), (r(K ** 3, cin, cout) * 0.1).to(DEV)
        self.bias, self.residual = r(cout).to(DEV), r(N, cout).to(DEV)
        self.gamma, self.beta = (1 + 0.3 * r(cout)).to(DEV), (0.3 * r(cout)).to(DEV)
        self.pre, self.grad_next = (1.5 * r(N, cout) + 0.1).to(DEV), r(N, cin).to(DEV)      # the backward's: a stage's rows, the next one's g_pre
        self.rb = Rulebook(self.idx, 1, SHAPE, K)
        self.N, self.cin, self.cout = N, cin, cout


@functools.lru_cache(maxsize=None)
def case(N, cin, cout):
    return Case(N, cin, cout)


class Outputs:
    """The caller regions of one backward call, each with a guard behind it; prefilled so that an unwritten value shows."""

    def __init__(self, N, cout, with_bias=True):
        self.N, self.cout = N, cout
        self.nwork = sizes(N, cout)[1]
        self.g = {"g_pre": Guarded(N * cout * 4, DEV, GUARD, sentinel=-77.0, body=-55.0), "work": Guarded(self.nwork, DEV, GUARD)}
        for k in ("ln_weight", "ln_bias") + (("bias",) if with_bias else ()):
            self.g[k] = Guarded(cout * 4, DEV, GUARD, sentinel=-77.0, body=-55.0)

    def args(self):
        f = lambda k: self.g[k].floats(self.cout) if k in self.g else None
        return (self.g["g_pre"].floats(self.N, self.cout), f("ln_weight"), f("ln_bias"), f("bias"), self.g["work"].buf, self.nwork)

    def results(self):
        torch.cuda.synchronize()
        assert all(g.intact() for g in self.g.values())
        out = {k: (g.floats(self.N, self.cout) if k == "g_pre" else g.floats(self.cout)).clone() for k, g in self.g.items() if k != "work"}
        assert not any(bool((t == -55.0).any()) for t in out.values())          # every value was written
        return out


def standalone(o, pre, grad_out, gamma, beta, relu):
    _lib.call("gf_subm_stage_backward", DEV, o.N, o.cout, pre, grad_out, gamma, beta, int(relu), *o.args())
    return o.results()


def fused(o, rb, grad_next, weight_t, pre, gamma, beta, relu):
    cin = weight_t.shape[1]
    partial, scratch, nscratch = rb._scratch(cin, o.cout, DEV)
    _lib.call("gf_subm_conv_apply_stage_backward", DEV, *rb.dims, cin, o.cout, rb.total, grad_next, weight_t, rb.tables, rb.pair_in, partial,
              scratch, nscratch, pre, gamma, beta, int(relu), *o.args())
    return o.results()


# ---- 3. the saving forward -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("N", [N_ODD, 300, 7])
def test_saving_forward_is_the_epilogue_and_stores_pre(N, cin, cout, spy):
    c = case(N, cin, cout)
    out_g, pre_g = (Guarded(N * cout * 4, DEV, GUARD, sentinel=-77.0, body=-55.0) for _ in range(2))
    partial, scratch, nscratch = c.rb._scratch(cin, cout, DEV)
    out, pre = out_g.floats(N, cout), pre_g.floats(N, cout)
    _lib.call("gf_subm_conv_apply_epilogue_train", DEV, *c.rb.dims, cin, cout, c.rb.total, c.feat, c.weight, c.rb.tables, c.rb.pair_in,
              partial, out, scratch, nscratch, c.bias, c.residual, c.gamma, c.beta, 1, pre)
    torch.cuda.synchronize()
    assert out_g.intact() and pre_g.intact()
    want = c.rb.apply(c.feat, c.weight, bias=c.bias, residual=c.residual, norm=(c.gamma, c.beta), relu=True)
    assert torch.equal(bits(out), bits(want))
    plain = c.rb.apply(c.feat, c.weight)
    assert bool((pre == (plain + c.bias) + c.residual).all()) and plain.abs().max() > 0
    # without bias, residual and ReLU: pre is the convolution itself, bit for bit
    del spy[:]
    out2, pre2 = c.rb.stage_forward(c.feat, c.weight, None, None, c.gamma, c.beta, False)
    assert spy == ["gf_subm_conv_apply_epilogue_train"]
    assert torch.equal(bits(pre2), bits(plain))
    assert torch.equal(bits(out2), bits(c.rb.apply(c.feat, c.weight, norm=(c.gamma, c.beta))))


# ---- 4. the standalone backward against float64 ----------------------------------------------------------------------------------

class Rows:
    """Kink-free rows of a stage and its three results: the float64 truth, torch's fp32 autograd, the native call."""

    def __init__(self, cout, relu, scale, pick=None):
        x = row_ref.planted(row_ref.fixed_input(N_ODD, cout, 40 + cout) * scale)
        sd = row_ref.fixed_weights({"ln.weight": (cout,), "ln.bias": (cout,)}, 900)
        self.gamma, self.beta = sd["ln.weight"], sd["ln.bias"]
        xhat, u = ref.stage_parts(x.double(), self.gamma.double(), self.beta.double())
        keep = ref.outside_margin(u, xhat, self.gamma.double(), self.beta.double(), row_ref.KINK_MARGIN).all(dim=1)
        self.dropped = N_ODD - int(keep.sum())
        print(f"kink filter (Cout = {cout}, scale {scale}): {self.dropped} of {N_ODD} rows dropped")
        assert self.dropped <= N_ODD // 100 and bool(keep[:4].all())          # at most 1 %; the planted rows stay
        pick = slice(None) if pick is None else pick
        self.pre = x[keep][pick]
        n = self.pre.shape[0]
        self.cot = row_ref.output_weights((int(keep.sum()), cout), torch.float32)[pick]
        mask = "own" if relu else None
        self.truth = ref.stage_backward(self.pre, self.cot, self.gamma, self.beta, mask)
        leaves = [t.clone().requires_grad_(True) for t in (self.pre, self.gamma, self.beta)]
        y = F.layer_norm(leaves[0], (cout,), leaves[1], leaves[2], 1e-5)
        g = torch.autograd.grad(((torch.relu(y) if relu else y) * self.cot).sum(), leaves)
        self.torch32 = {"g_pre": g[0], "ln_weight": g[1], "ln_bias": g[2], "bias": g[0].sum(0)}
        d = lambda t: t.to(DEV)
        self.native = {k: v.cpu() for k, v in standalone(Outputs(n, cout), d(self.pre), d(self.cot), d(self.gamma), d(self.beta), relu).items()}
        self.row_yardstick = {"g_pre": max_error(self.torch32["g_pre"], self.truth["g_pre"])}


@functools.lru_cache(maxsize=None)
def family(cout, relu, scale):
    return Rows(cout, relu, scale)


SUMS = lambda key: "column sums"      # the three sums are one kind of leaf


@pytest.mark.parametrize("cout", [128, 32])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("scale", [1.0, 1e-3])       # (at 1e-3 the variance is a tenth of eps)
def test_standalone_backward_against_float64(cout, relu, scale):
    r = family(cout, relu, scale)
    assert float(r.truth["g_pre"].abs().max()) > 0
    judge_leaves(r.native, r.truth, r.torch32, SUMS, f"stage backward {cout} relu={relu} x{scale}", per_row=("g_pre",),
                 row_yardstick=r.row_yardstick)
    if relu:   # u <= 0 passes nothing: those entries of g_u are exact zeros, so ln_bias sums fewer terms than without the ReLU
        assert not torch.equal(r.native["ln_bias"], family(cout, False, scale).native["ln_bias"])


@pytest.mark.parametrize("cout", [128, 32])
@pytest.mark.parametrize("pick", [slice(10, 11), slice(0, 7)], ids=["N1", "N7"])
def test_standalone_backward_on_fewer_rows_than_a_workgroup(cout, pick):
    """One row and seven (the planted rows among them); a row's yardstick is the family's."""
    r = Rows(cout, True, 1.0, pick)
    assert r.pre.shape[0] == pick.stop - pick.start
    judge_leaves(r.native, r.truth, r.torch32, SUMS, f"stage backward {cout} N={r.pre.shape[0]}", per_row=("g_pre",),
                 row_yardstick=family(cout, True, 1.0).row_yardstick)
    # a row's g_pre does not depend on how many rows the call has
    full = family(cout, True, 1.0)
    assert torch.equal(bits(r.native["g_pre"]), bits(full.native["g_pre"][pick]))


def test_no_rows_zero_fills_the_parameter_gradients():
    for name, head in (("gf_subm_stage_backward", (0, 32, None, None)),
                       ("gf_subm_conv_apply_stage_backward", (0, 1, *SHAPE, K, 32, 32, 0, None, None, None, None, None, None, 0, None))):
        g = [torch.full((32,), 7.0, device=DEV) for _ in range(3)]
        _lib.call(name, DEV, *head, g[0], g[1], 1, None, g[0], g[1], g[2], None, 0)
        assert all(not t.any() for t in g), name


# ---- 5. the backward inside the data-gradient convolution is the standalone one, bit for bit ------------------------------------

@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("N", [N_ODD, 300])
def test_fused_backward_equals_standalone(N, cin, cout):
    c = case(N, cin, cout)
    weight_t = c.weight.flip(0).contiguous()          # any [K^3, Cin, Cout] weight: the data gradient's is the next stage's, mirrored
    gy = c.rb.apply(c.grad_next, weight_t)            # gf_subm_conv_apply_scratch
    runs = [standalone(Outputs(N, cout), c.pre, gy, c.gamma, c.beta, 1) for _ in range(2)]
    runs += [fused(Outputs(N, cout), c.rb, c.grad_next, weight_t, c.pre, c.gamma, c.beta, 1) for _ in range(2)]
    assert gy.abs().max() > 0 and runs[0]["g_pre"].abs().max() > 0
    for other in runs[1:]:
        for k, v in runs[0].items():
            assert torch.equal(bits(v), bits(other[k])), k
    # grad_bias is optional: without it the other results are the same bits
    for run in (standalone(Outputs(N, cout, with_bias=False), c.pre, gy, c.gamma, c.beta, 1),
                fused(Outputs(N, cout, with_bias=False), c.rb, c.grad_next, weight_t, c.pre, c.gamma, c.beta, 1)):
        assert set(run) == {"g_pre", "ln_weight", "ln_bias"} and all(torch.equal(bits(v), bits(runs[0][k])) for k, v in run.items())
    # ... and they are the sums of what was stored: g_pre's columns, in double
    assert torch.allclose(runs[0]["bias"].double(), runs[0]["g_pre"].double().sum(0), rtol=0, atol=1e-4 * float(runs[0]["g_pre"].abs().max()))


# ---- 6. NaN rows and graph replay ----------------------------------------------------------------------------------------------

def test_an_over_capacity_rulebook_gives_nan_gradients():
    c = case(300, 64, 32)
    rb = Rulebook(c.idx, 1, SHAPE, K, pair_capacity=1)
    out, pre = rb.stage_forward(c.feat, c.weight, c.bias, c.residual, c.gamma, c.beta, True)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(pre).all())
    gy = torch.randn(300, 32, device=DEV)
    weight_t = c.weight.flip(0).contiguous()
    for relu in (True, False):
        for res in (rb.stage_backward(pre, c.gamma, c.beta, relu, True, grad_out=gy),                     # NaN rows saved by the forward
                    rb.stage_backward(c.pre, c.gamma, c.beta, relu, True, grad_next=c.grad_next, weight_t=weight_t)):   # NaN dL/dy
            assert all(t.shape[-1] == 32 and bool(torch.isnan(t).all()) for t in res), relu
    with pytest.raises(RuntimeError, match="pair_capacity"):
        rb.check()


def test_graph_replay_of_forward_and_backward_equals_eager():
    c = case(300, 128, 128)
    rb = Rulebook(c.idx, 1, SHAPE, K, pair_capacity=128 * 300)      # (sized by a capacity: both gather-GEMM walks are launched)
    x = c.feat.clone().requires_grad_()
    leaves = [t.clone().requires_grad_() for t in (c.weight, c.bias, c.gamma, c.beta)]
    cot = row_ref.output_weights((300, 128), torch.float32).to(DEV)

    def step():
        w, b, g, be = leaves
        out = subm_stages(x, rb, [dict(weight=w, bias=b, norm=(g, be), relu=True)] * 2 + [dict(weight=w, bias=b, residual=c.residual, norm=(g, be))])
        return (out, *torch.autograd.grad((out * cot).sum(), [x, *leaves]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for scale in (1.0, -0.5):
        with torch.no_grad():
            x.copy_(c.feat * scale)
        graph.replay()
        got = [t.clone() for t in captured]
        for a, b in zip(got, step()):
            assert torch.equal(bits(a), bits(b)) and bool(torch.isfinite(a).all()) and a.abs().max() > 0


# ---- 7. the ReLU masks of three chained stages ---------------------------------------------------------------------------------

def _stages_of(m):
    layers = list(m.layer) if isinstance(m.layer, nn.ModuleList) else [m.layer]
    return [l for l in layers if isinstance(l, SubMConv3d)], [l for l in layers if isinstance(l, nn.LayerNorm)]


def _leaves(b):
    """The block's parameters under ``subm_stage_ref.block``'s names."""
    convs, lns = _stages_of(b.m)
    p = {}
    for s, conv in enumerate(convs):
        p[f"conv{s}.weight"] = conv.weight
        if lns:
            p.update({f"conv{s}.bias": conv.bias, f"ln{s}.weight": lns[s].weight, f"ln{s}.bias": lns[s].bias})
    if isinstance(b.m.output_proj, nn.Linear):
        p.update({"proj.weight": b.m.output_proj.weight, "proj.bias": b.m.output_proj.bias})
    p.update({"norm.weight": b.norm.weight, "norm.bias": b.norm.bias})
    return p


def _chain(b, rb, x):
    """``[y_s]``: the stages as chained ``subm_stage`` calls on ``x [N, C]``."""
    convs, lns = _stages_of(b.m)
    ys, out = [], x
    for conv, ln in zip(convs, lns):
        src = out * rb.representative_mask() if b.duplicates == "last" else out
        out = subm_stage(src, rb, conv.weight, bias=conv.bias, norm=ln, relu=True)
        ys.append(out)
    return ys


def test_chained_masks_are_the_float64_masks_outside_the_margin():
    b = block("multi_proj", "sum")
    idx = b.m.voxel_indices(b.anchor)
    rb = Rulebook(idx, BS, b.m._spatial, BLOCK_K)
    d = lambda t: t.detach().cpu().double()
    p64 = {k: d(v) for k, v in _leaves(b).items()}
    _, seen = ref.block(d(b.x), d(b.residual), p64, idx.cpu(), BS, b.m._spatial, BLOCK_K, "own", with_stages=True)
    with torch.no_grad():
        ys = _chain(b, rb, b.x.flatten(0, 1))
    convs, lns = _stages_of(b.m)
    inside = total = 0
    worst = 0.0
    for s, (pre64, u64, xhat64) in enumerate(seen):
        gamma, beta = p64[f"ln{s}.weight"], p64[f"ln{s}.bias"]
        # the native stage's error: its pre and its u (the same stage without the ReLU, on the native input) against the truth
        src = b.x.flatten(0, 1) if s == 0 else ys[s - 1]
        u32, pre32 = rb.stage_forward(src.contiguous(), convs[s].weight.detach(), convs[s].bias.detach(), None, lns[s].weight.detach(),
                                      lns[s].bias.detach(), False)
        scale = 1.0 + (xhat64 * gamma).abs() + beta.abs()
        err_pre, err_u = max_error(pre32.cpu(), pre64), float(((u32.cpu().double() - u64).abs() / scale).max())
        print(f"stage {s}: max|pre - pre64| = {err_pre:.3e} (max|pre64| = {float(pre64.abs().max()):.3e}), max|u - u64| / (1 + |xhat gamma| + |beta|) = {err_u:.3e}")
        worst = max(worst, err_u)
        out = ref.outside_margin(u64, xhat64, gamma, beta, MASK_MARGIN)
        inside, total = inside + int((~out).sum()), total + out.numel()
        assert torch.equal((ys[s].cpu() > 0)[out], (u64 > 0)[out]), s
        assert 0.2 < float((u64 > 0).double().mean()) < 0.8
    print(f"entries inside the margin {MASK_MARGIN:g}: {inside} of {total} ({100.0 * inside / total:.4f} %); 10 x the largest stage error = {10 * worst:.3e}")
    assert inside <= total // 1000                    # depends on the float64 reference alone
    assert MASK_MARGIN >= 10 * worst


# ---- 8. the block ------------------------------------------------------------------------------------------------------------------

TRAIN, BACK, FUSED = "gf_subm_conv_apply_epilogue_train", "gf_subm_stage_backward", "gf_subm_conv_apply_stage_backward"
APPLY, WGRAD = "gf_subm_conv_apply_scratch", "gf_subm_conv_weight_grad"
NATIVE = {("single", "sum"): BUILD + [TRAIN, BACK, WGRAD, APPLY], ("single", "last"): BUILD + [TRAIN, BACK, WGRAD, APPLY],
          ("single_proj", "sum"): BUILD + [APPLY, APPLY, WGRAD], ("single_proj", "last"): BUILD + [APPLY, APPLY, WGRAD],
          ("multi_proj", "sum"): BUILD + [TRAIN] * 3 + [BACK, WGRAD, FUSED, WGRAD, FUSED, WGRAD, APPLY],
          ("multi_proj", "last"): BUILD + [TRAIN] * 3 + [BACK, WGRAD, APPLY] * 3}
TODAY = {"single": BUILD + [APPLY, APPLY, WGRAD], "single_proj": BUILD + [APPLY, APPLY, WGRAD], "multi_proj": BUILD + [APPLY] * 3 + [APPLY, WGRAD] * 3}


def _step(b, native, forward=None):
    """``(out, {"x", "residual", leaf: gradient})`` of the fixed scalar through the module (``native``: the attribute, ``None`` =
    left at its default) or through ``forward(x, residual)``."""
    leaves = _leaves(b)
    for t in leaves.values():
        t.grad = None
    x = b.x.clone().requires_grad_()
    res = None if b.residual is None else b.residual.clone().requires_grad_()
    if native is not None:
        b.m.native_training = native
    try:
        out = forward(x, res) if forward else b.m(x, b.anchor, residual=res, norm=b.norm)
        (out * row_ref.output_weights(out.shape, torch.float32).to(DEV)).sum().backward()
    finally:
        if native is not None:
            del b.m.native_training          # (back to the class attribute)
    grads = {"x": x.grad, **({} if res is None else {"residual": res.grad}), **{k: t.grad for k, t in leaves.items()}}
    assert all(g is not None for g in grads.values())
    return out.detach(), {k: g.detach().clone() for k, g in grads.items()}


@pytest.mark.parametrize("duplicates", ["sum", "last"])
@pytest.mark.parametrize("family_", ["single", "single_proj", "multi_proj"])
def test_block_native_training(family_, duplicates, spy):
    b = block(family_, duplicates)
    m = b.m
    convs, lns = _stages_of(m)
    watched = [l for l in m.modules() if isinstance(l, nn.ReLU)] + lns + ([b.norm] if family_ == "single" else [])
    calls = [0]
    handles = [mod.register_forward_hook(lambda *a: calls.__setitem__(0, calls[0] + 1)) for mod in watched]
    del spy[:]
    out, native = _step(b, True)
    assert spy == NATIVE[family_, duplicates]
    assert calls[0] == 0                                    # the stages' torch LayerNorm / ReLU never ran
    del spy[:]
    out_default, _ = _step(b, None)
    assert spy == TODAY[family_] and calls[0] == len(watched)
    for h in handles:
        h.remove()
    _, torch32 = _step(b, False)
    rb = m.last_rulebook

    # the functional chain: the same bits in the output and in the input gradient
    def functional(x, res):
        feats = x.flatten(0, 1)
        if family_ == "multi_proj":
            y = m.output_proj(_chain(b, rb, feats)[-1].unflatten(0, (BS, G)))
            return b.norm(y if res is None else y + res)
        if family_ == "single":
            src = feats * rb.representative_mask() if duplicates == "last" else feats
            return subm_stage(src, rb, m.layer.weight, residual=None if res is None else res.flatten(0, 1), norm=b.norm).unflatten(0, (BS, G))
        return b.norm(m.output_proj(m.layer(feats, None, BS, m._spatial, rulebook=rb).unflatten(0, (BS, G))))
    out_f, chain = _step(b, None, functional)
    assert torch.equal(bits(out), bits(out_f)) and torch.equal(bits(native["x"]), bits(chain["x"]))
    assert out.shape == (BS, G, E) and bool(torch.isfinite(out).all())

    # the float64 truth with the native route's masks
    masks = None
    if lns:
        with torch.no_grad():
            masks = [(y > 0).double().cpu() for y in _chain(b, rb, b.x.flatten(0, 1))]
    rep = rb.representative_mask() if duplicates == "last" else None
    truth = ref.block_gradients(b.x, b.residual, _leaves(b), rb.indices, BS, m._spatial, BLOCK_K, masks, rep)
    cpu = lambda g: {k: v.cpu() for k, v in g.items()}
    native, torch32 = cpu(native), cpu(torch32)
    assert set(native) == set(truth)
    rows = [k for k in ("x", "residual") if k in truth]
    judge_leaves(native, truth, torch32, lambda k: re.sub(r"\d", "", k), f"block {family_} {duplicates}", per_row=rows,
                 row_yardstick={k: max_error(torch32[k], truth[k]) for k in rows})
