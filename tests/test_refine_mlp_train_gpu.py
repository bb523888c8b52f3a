"""The refinement modules' native training step on the GPU (gf_refine_mlp_forward_train, gf_refine_mlp_backward through raw
library calls, ``RefineFusedFunction`` and the modules' ``native_training``).

1. The saving forward, bitwise: every output and ``mlp_out`` equal ``refine_fused(..., return_mlp_output=True)`` on unfiltered
   rows.
2. The tail, bitwise: ``grad_mlp_out`` and ``grad_anchor`` of a raw backward call equal what ``RefineFunction``'s backward gives
   on (``mlp_out`` of that call, anchor, the same output gradients) -- also with some output gradients NULL, and with
   ``grad_mlp_out`` NULL the other results keep their bits.  This decouples the MLP's check from the tail's amplification
   (version 2's inverse sigmoid, up to 1e4); the tail's own accuracy is tests/test_refine_gpu.py's.
3. The MLP's gradients on rows that pass the kink filter (tests/refine_mlp_train_ref.py).  Truth = the float64 ``vjp`` with the
   cotangent ``grad_mlp_out.double()`` of that very call, yardstick Y = the float32 torch ``vjp`` on the same GPU, rows and
   cotangent.  ``grad_x``: ``max|native - truth| <= 2 Y + 4 eps32 max|truth|`` with Y at the variant's n = 1 000.  A parameter:
   the error relative to the leaf's ``max|truth|`` against ``2 Y + 4 eps32``, Y the largest relative error over the leaves of
   its kind at the same n (the project's rule).
4. Bitwise invariants.
5. The function and the modules.
The measured ratios are in DESIGN.md §3.12c."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import refine_mlp_train_ref as T
import refine_ref
from gaussianformer_amd import _lib
from gaussianformer_amd import refine as R
from refine_ref import VARIANTS, make_module, outputs_of
from row_ref import scalar_gradients
from row_judge import EPS32, Guarded, edge_rows, judge_leaves, max_error, ptr_table

pytestmark = pytest.mark.gpu
E = 128
B, CHUNK = _lib.GF_REFINE_MLP_WGRAD_ROWS, _lib.GF_REFINE_MLP_CHUNK_ROWS
EDGES = edge_rows(B)
FULL = 1000
GUARD = 256          # sentinel bytes behind every buffer the library writes


class Setup:
    """Per variant, computed once and left unchanged: the module on the GPU, the surviving rows and the unfiltered ones."""

    def __init__(self, name):
        self.name = name
        self.cfg, self.extra = VARIANTS[name]
        dev = self.dev = torch.device("cuda:0")
        module, feat, anchor, embed = T.survivors(name)
        self.state64 = {k: v.detach().double() for k, v in module.state_dict().items()}
        self.module = make_module(self.cfg, 200 + list(VARIANTS).index(name)).to(dev)
        self.state = {k: v.detach() for k, v in self.module.state_dict().items()}
        self.params = [self.state[k] for k in R.MLP_KEYS]
        self.rcfg, self.D = self.module._cfg, self.module.output_dim
        self.cpu = (feat, anchor, embed)
        self.feat, self.anchor, self.embed = feat.to(dev), anchor.to(dev), embed.to(dev)
        self.raw_rows = [t.to(dev) for t in T.candidates(name)[1:4]]     # unfiltered
        self.Da = anchor.shape[1]
        self.opa = 1 if self.rcfg.flags & _lib.GF_REFINE_OPACITY else 0
        three = 3 if self.rcfg.version == 2 else 0
        self.widths = dict(zip(refine_ref.NAMES, (self.D, 3, 3, 4, self.opa, self.rcfg.S, three, three)))

    def rows(self, n):
        """The first n surviving rows (repeated where n exceeds their number)."""
        m = self.feat.shape[0]
        if n <= m:
            return self.feat[:n], self.anchor[:n], self.embed[:n]
        idx = torch.arange(n, device=self.dev) % m
        return self.feat[idx], self.anchor[idx], self.embed[idx]

    def out_grads(self, n, names=None):
        """The gradients of the fixed scalar with respect to the eight outputs (its weights); None for an empty output and
        for the names left out."""
        w = refine_ref.fixed_weights({k: torch.empty(n, width) for k, width in self.widths.items()})
        return [w[k].to(self.dev) if self.widths[k] and (names is None or k in names) else None for k in refine_ref.NAMES]

    def step(self, feat, anchor, embed, gouts, want_gmo=True, prefill=None):
        """One raw forward_train + backward.  Every buffer the library writes has sentinel bytes behind it, checked by
        ``finish``."""
        n, D, Da, dev, c = feat.shape[0], self.D, self.Da, self.dev, self.rcfg
        consts = (ctypes.c_double * 11)(*c.consts)
        cp = ctypes.cast(consts, ctypes.c_void_p)
        saved_bytes, work_bytes = R.train_sizes(n, D, Da)
        res = dict(n=n, bufs=[])

        def guarded(nbytes, fill=None):
            res["bufs"].append(Guarded(nbytes, dev, GUARD, 0xA5, body=fill))
            return res["bufs"][-1]

        def new(*shape, fill=None):
            return guarded(4 * int(np.prod(shape)), fill).floats(*shape)

        outs = [new(n, self.widths[k]) for k in refine_ref.NAMES]
        mlp_out = new(n, D)
        saved, work = guarded(saved_bytes).buf, guarded(work_bytes).buf
        table = ptr_table(self.params)
        _lib.call("gf_refine_mlp_forward_train", dev, n, E, D, Da, c.version, c.flags, c.R, c.S, cp, feat, embed, anchor, table,
                  mlp_out, *outs, saved, saved_bytes)
        grad_x, grad_anchor = new(n, E), new(n, Da)
        gmo = new(n, D) if want_gmo else None
        grads = [new(*p.shape, fill=prefill) for p in self.params]
        _lib.call("gf_refine_mlp_backward", dev, n, E, D, Da, c.version, c.flags, c.R, c.S, cp, feat, embed, anchor, table, saved,
                  *gouts, grad_x, grad_anchor, gmo, ptr_table(grads), work, work_bytes)
        res.update(outs=dict(zip(refine_ref.NAMES, outs)), mlp_out=mlp_out, grad_x=grad_x, grad_anchor=grad_anchor, gmo=gmo,
                   grads=dict(zip(R.MLP_KEYS, grads)))
        return res

    @staticmethod
    def finish(res):
        assert all(buf.intact() for buf in res["bufs"]), "sentinel bytes behind a buffer were overwritten"
        return res

    def run(self, n, **kw):
        feat, anchor, embed = self.rows(n)
        return self.finish(self.step(feat, anchor, embed, self.out_grads(n), **kw))

    def tail_reference(self, res, anchor, gouts):
        """(grad of mlp_out, grad of anchor) by RefineFunction's backward on the call's mlp_out and the same output gradients."""
        o, a = res["mlp_out"].clone().requires_grad_(True), anchor.clone().requires_grad_(True)
        outs = R.RefineFunction.apply(o, a, self.rcfg)
        pairs = [(t, g) for t, g in zip(outs, gouts) if g is not None]
        return torch.autograd.grad([t for t, _ in pairs], [o, a], [g for _, g in pairs])

    def mlp_grads(self, res, feat, embed):
        """(native, truth, float32 torch) gradients of the MLP with the call's own cotangent, on the CPU in float64 (the truth is
        computed there)."""
        gmo = res["gmo"]
        def vjp(x, state, cotangent):
            return scalar_gradients(lambda x, leaves: refine_ref.mlp(leaves, x), {"x": x}, {k: state[k] for k in R.MLP_KEYS}, cotangent)
        truth = vjp(feat.double().cpu() + embed.double().cpu(), self.state64, gmo.double().cpu())
        torch32 = vjp(feat + embed, self.state, gmo)
        on_cpu = lambda g: {k: v.double().cpu() for k, v in g.items()}
        return on_cpu(dict(x=res["grad_x"], **res["grads"])), truth, on_cpu(torch32)

    @functools.cached_property
    def full(self):
        return self.run(FULL)

    @functools.cached_property
    def full_grads(self):
        feat, _, embed = self.rows(FULL)
        return self.mlp_grads(self.full, feat, embed)

    def check_mlp(self, res, feat, embed):
        """Rule (3)."""
        native, truth, torch32 = self.full_grads if res is self.full else self.mlp_grads(res, feat, embed)
        _, full_truth, full32 = self.full_grads
        worst = judge_leaves(native, truth, torch32, T.kind, f"{self.name} n={res['n']}", per_row=("x",),
                             row_yardstick={"x": max_error(full32["x"], full_truth["x"])})
        assert sorted(worst) == sorted(("x",) + T.KINDS)


@functools.lru_cache(maxsize=None)
def setup(name):
    return Setup(name)


# ---- 1. the saving forward ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(VARIANTS))
def test_the_saving_forward_has_the_plain_forwards_bits(name):
    s = setup(name)
    feat, anchor, embed = s.raw_rows
    for n in (*EDGES, FULL):
        f, a, e = feat[:n], anchor[:n], embed[:n]
        res = s.finish(s.step(f, a, e, s.out_grads(n)))
        with torch.no_grad():
            anchor_out, pred, mlp_out = R.refine_fused(f, a, e, s.state, s.rcfg, return_mlp_output=True)
        want = outputs_of(anchor_out, pred)
        assert torch.equal(res["mlp_out"], mlp_out), (name, n)
        for k, t in want.items():
            assert res["outs"][k].shape == t.shape and torch.equal(res["outs"][k], t), (name, n, k)


# ---- 2. the tail -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(VARIANTS))
def test_the_tails_gradients_are_the_standalone_tails(name):
    s = setup(name)
    for n in (33, 129, FULL):
        feat, anchor, embed = s.rows(n)
        for names in (None, ("anchor_out",), ("means", "semantics", "delta_means"), ("scales", "rotations", "opacities", "original_means")):
            gouts = s.out_grads(n, names)
            if all(g is None for g in gouts):
                continue
            res = s.finish(s.step(feat, anchor, embed, gouts))
            go, ga = s.tail_reference(res, anchor, gouts)
            assert torch.equal(res["gmo"], go), (name, n, names)
            assert torch.equal(res["grad_anchor"], ga), (name, n, names)
            bare = s.finish(s.step(feat, anchor, embed, gouts, want_gmo=False))
            assert bare["gmo"] is None
            assert torch.equal(bare["grad_x"], res["grad_x"]) and torch.equal(bare["grad_anchor"], res["grad_anchor"])
            for k in R.MLP_KEYS:
                assert torch.equal(bare["grads"][k], res["grads"][k]), (name, n, names, k)


# ---- 3. the MLP's gradients --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(VARIANTS))
def test_mlp_gradients_at_the_family_size(name):
    s = setup(name)
    feat, _, embed = s.rows(FULL)
    s.check_mlp(s.full, feat, embed)


@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("name", ["solid", "prob"])
def test_mlp_gradients_at_the_edges(name, n):
    s = setup(name)
    feat, _, embed = s.rows(n)
    s.check_mlp(s.run(n), feat, embed)


def test_mlp_gradients_across_a_chunk_boundary():
    """n = GF_REFINE_MLP_CHUNK_ROWS + 582: two chunks, the second with a partial weight-gradient block and a partial tile."""
    s = setup("solid")
    n = CHUNK + 582
    feat, _, embed = s.rows(n)
    res = s.run(n)
    s.check_mlp(res, feat, embed)
    for k in ("grad_x", "grad_anchor", "gmo"):
        assert torch.equal(res[k][:FULL], s.full[k]), k


# ---- 4. bitwise invariants ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["solid", "prob", "D43"])
def test_repeatable_row_independent_and_stored_not_accumulated(name):
    s = setup(name)
    full = s.full
    again = s.run(FULL, prefill=float("nan"))       # the parameter gradients prefilled with NaN
    for k in ("grad_x", "grad_anchor", "gmo"):
        assert torch.equal(again[k], full[k]), (name, k)
    for k in R.MLP_KEYS:
        assert bool(torch.isfinite(again["grads"][k]).all()) and torch.equal(again["grads"][k], full["grads"][k]), (name, k)
    for n in (1, 33, 129, B + 1):
        part = s.run(n)
        for k in ("grad_x", "grad_anchor", "gmo"):
            assert torch.equal(part[k], full[k][:n]), (name, n, k)
    # a row permutation permutes the rows' results (the cotangent rows move with them)
    n = 300
    perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).to(s.dev)
    feat, anchor, embed = s.rows(n)
    gouts = s.out_grads(n)
    res = s.finish(s.step(feat[perm], anchor[perm], embed[perm], [None if g is None else g[perm] for g in gouts]))
    for k in ("grad_x", "grad_anchor", "gmo"):
        assert torch.equal(res[k], full[k][:n][perm]), (name, k)


@pytest.mark.parametrize("name", ["solid", "prob"])
def test_replayed_from_a_graph(name):
    s = setup(name)
    n = 700
    feat, anchor, embed = s.rows(n)
    gouts = s.out_grads(n)
    eager = s.finish(s.step(feat, anchor, embed, gouts))
    static = {}

    def body():
        static["res"] = s.step(feat, anchor, embed, gouts)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    res = static["res"]
    for t in (res["grad_x"], res["grad_anchor"], res["gmo"], res["mlp_out"], *res["grads"].values(), *res["outs"].values()):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    s.finish(res)
    for k in ("grad_x", "grad_anchor", "gmo", "mlp_out"):
        assert torch.equal(res[k], eager[k]), (name, k)
    for k in R.MLP_KEYS:
        assert torch.equal(res["grads"][k], eager["grads"][k]), (name, k)
    for k, t in eager["outs"].items():
        assert torch.equal(res["outs"][k], t), (name, k)


@pytest.mark.parametrize("name", ["solid", "prob"])
def test_no_rows_zero_fills_the_gradients(name):
    s = setup(name)
    dev = s.dev
    grads = [torch.full_like(p, float("nan")) for p in s.params]
    consts = (ctypes.c_double * 11)(*s.rcfg.consts)
    c = s.rcfg
    _lib.call("gf_refine_mlp_backward", dev, 0, E, s.D, s.Da, c.version, c.flags, c.R, c.S, ctypes.cast(consts, ctypes.c_void_p),
              None, None, None, None, None, *([None] * 8), None, None, None, ptr_table(grads), None, 0)
    torch.cuda.synchronize()
    for k, g in zip(R.MLP_KEYS, grads):
        assert bool((g == 0).all()), (name, k)


@pytest.mark.parametrize("name", ["solid", "prob"])
def test_a_nan_row_changes_no_other_rows_gradient(name):
    s = setup(name)
    n = 300
    for row in (37, 0, 299, 128):
        feat, anchor, embed = [t.clone() for t in s.rows(n)]
        feat[row] = float("nan")
        res = s.finish(s.step(feat, anchor, embed, s.out_grads(n)))
        keep = torch.arange(n, device=s.dev) != row
        assert bool(torch.isnan(res["grad_x"][row]).all()), (name, row)
        for k in ("grad_x", "grad_anchor", "gmo"):
            assert torch.equal(res[k][keep], s.full[k][:n][keep]), (name, row, k)


# ---- 5. the function and the modules -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(refine_ref.FAMILIES))
def test_modules(name):
    s = setup(name)
    module = s.module
    n = 600
    feat, anchor, embed = s.rows(n)
    raw = s.finish(s.step(feat, anchor, embed, s.out_grads(n)))
    lead = lambda t: t.reshape(2, n // 2, -1)

    def scalar(res):
        outs = {k: v.reshape(n, v.shape[-1]) for k, v in outputs_of(res[0], res[1]).items()}
        return refine_ref.weighted_sum(outs, refine_ref.fixed_weights(outs))

    def leaves():
        return [lead(t).clone().requires_grad_(True) for t in (feat, anchor, embed)]

    def clear():
        for p in module.parameters():
            p.grad = None

    try:
        assert module.native_training is False
        # the attribute off: the parent's route, values and gradients
        clear()
        f, a, e = leaves()
        off = module(f, a, e)
        scalar(off).backward()
        off_grads = [t.grad for t in (f, a, e)] + [p.grad for p in module.parameters()]
        clear()
        f2, a2, e2 = leaves()
        today = R.refine(module.layers(f2 + e2), a2, module._cfg)
        scalar(today).backward()
        for x, y in zip(outputs_of(*off).values(), outputs_of(*today).values()):
            assert torch.equal(x, y)
        for x, y in zip(off_grads, [t.grad for t in (f2, a2, e2)] + [p.grad for p in module.parameters()]):
            assert torch.equal(x, y)

        # the attribute on: the fused forward's bits, the raw call's gradients
        module.native_training = True
        clear()
        with torch.no_grad():
            want = R.refine_fused(lead(feat), lead(anchor), lead(embed), s.state, module._cfg)
            quiet = module(lead(feat), lead(anchor), lead(embed))      # no gradient needed and fused_mlp off: the default route
            assert quiet[0].grad_fn is None
        f, a, e = leaves()
        on = module(f, a, e)
        assert on[0].grad_fn is not None and on[0].shape == (2, n // 2, s.D) and on[1].means.shape == (2, n // 2, 3)
        for x, y in zip(outputs_of(*on).values(), outputs_of(*want).values()):
            assert x.shape == y.shape and torch.equal(x, y)
        scalar(on).backward()
        assert torch.equal(f.grad.reshape(n, E), raw["grad_x"]) and torch.equal(e.grad.reshape(n, E), raw["grad_x"])
        assert torch.equal(a.grad.reshape(n, -1), raw["grad_anchor"])
        named = dict(module.named_parameters())
        for k in R.MLP_KEYS:
            assert named[k].grad is not None and named[k].grad.shape == named[k].shape
            assert torch.equal(named[k].grad, raw["grads"][k]), (name, k)

        # a broadcast anchor_embed gets the column sum of grad_x; a frozen parameter gets no .grad
        clear()
        named["layers.5.weight"].requires_grad_(False)
        row = embed[:1].clone().requires_grad_(True)
        f = feat.clone()
        res = R.refine_fused_autograd(f, anchor, row, module, module._cfg)
        scalar(res).backward()
        assert named["layers.5.weight"].grad is None and named["layers.7.weight"].grad is not None
        one = s.finish(s.step(f, anchor, row.detach().expand(n, E).contiguous(), s.out_grads(n)))
        for x, y in zip(outputs_of(*res).items(), outputs_of(*R.refine_fused(f, anchor, row.detach(), s.state, module._cfg)).values()):
            assert torch.equal(x[1], y) and torch.equal(y, one["outs"][x[0]]), x[0]     # the broadcast row written out, both ways
        exact = one["grad_x"].double().sum(0, keepdim=True)
        size = one["grad_x"].double().abs().sum(0, keepdim=True)
        assert row.grad.shape == (1, E)
        # a float32 sum of n terms in any order: |error| <= (n - 1) (eps32 / 2) sum|terms|, per column
        assert bool(((row.grad.double() - exact).abs() <= (n - 1) * (EPS32 / 2) * size).all())
    finally:
        module.native_training = False
        for p in module.parameters():
            p.requires_grad_(True)
            p.grad = None
