"""The fused refinement step on the GPU (gf_refine_mlp_forward through gaussianformer_amd.refine.refine_fused and the modules'
``fused_mlp``) against the float64 restatement of tests/refine_ref.py.

1. The MLP's result, ``mlp_out``, against the float64 ``refine_ref.mlp`` with the project's rule, per variant:
       max|native - truth| <= 2 Y + 4 eps32 max|truth|,    Y = max|fp32 torch composition on this GPU - truth| at n = 1 000.
   Both are fp32 evaluations of one formula that differ in the order of their sums.
2. The tail, bitwise: every output of the fused call equals ``RefineFunction.apply(mlp_out of that call, anchor, cfg)`` -- the
   fused tail and the standalone tail are one piece of code on the same bits -- and a call without ``mlp_out`` gives the same
   bits.  This replaces an end-to-end bound: version 2's inverse sigmoid amplifies an fp32 rounding of the MLP by up to 1e4, so
   a max-error comparison of two fp32 MLPs would be decided by chance at the amplified rows.  The end-to-end distance to the
   float64 module is printed, not asserted.
3. Invariants, bitwise: a row's result does not depend on n; n = 40 000; graph replay; repetition; a NaN row stays alone.
4. The modules with ``fused_mlp``.
The measured ratios are in DESIGN.md §3.12b."""
import functools

import pytest
import torch

import refine_ref
from gaussianformer_amd import refine as R
from refine_ref import VARIANTS, make_inputs, make_module, outputs_of
from row_judge import bound

pytestmark = pytest.mark.gpu
NS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000)


class Setup:
    """Per variant, computed once and left unchanged: the module on the GPU, the inputs, the float64 truth of the MLP and of the
    module, the composition's distance Y, and the fused call at the full n."""

    def __init__(self, name, n=1000):
        cfg, extra = VARIANTS[name]
        dev = torch.device("cuda:0")
        seed = 200 + list(VARIANTS).index(name)
        self.name, self.cfg, self.n = name, cfg, n
        module = make_module(cfg, seed)
        state64 = {k: v.detach().double() for k, v in module.state_dict().items()}
        self.module = module.to(dev).eval()
        self.state = {k: v.detach() for k, v in self.module.state_dict().items()}
        self.rcfg = self.module._cfg
        self.D = self.module.output_dim
        feat, anchor, embed = make_inputs(self.D, extra, n, seed + 1000)
        self.truth_mlp = refine_ref.mlp(state64, feat.double() + embed.double())
        self.truth = refine_ref.refine_tail(self.truth_mlp, anchor.double(), cfg)
        self.feat, self.anchor, self.embed = feat.to(dev), anchor.to(dev), embed.to(dev)
        with torch.no_grad():
            comp = refine_ref.mlp(self.state, self.feat + self.embed)
        self.Y = float((comp.double().cpu() - self.truth_mlp).abs().max())
        self.full = self.run(n)

    def run(self, n, with_mlp=True):
        """(outputs dict, mlp_out) of the fused call on the first n rows."""
        with torch.no_grad():
            res = R.refine_fused(self.feat[:n], self.anchor[:n], self.embed[:n], self.state, self.rcfg, return_mlp_output=with_mlp)
        return outputs_of(res[0], res[1]), (res[2] if with_mlp else None)

    def check_values(self, mlp_out, rows=None):
        """Rule (1) on mlp_out against the first rows of the truth."""
        t = self.truth_mlp[:mlp_out.shape[0]] if rows is None else rows
        err = float((mlp_out.double().cpu() - t).abs().max())
        limit = bound(self.Y, t)
        print(f"{self.name} n={mlp_out.shape[0]}: mlp_out native {err:.3e} composition(n={self.n}) {self.Y:.3e} bound {limit:.3e} ratio {err / limit:.3f}")
        assert torch.isfinite(mlp_out).all()
        assert err <= limit, (self.name, mlp_out.shape[0], err, self.Y, limit)

    def check_tail(self, outs, mlp_out, anchor):
        """Rule (2): the fused outputs against the standalone tail on the bits the fused tail consumed."""
        alone = R.RefineFunction.apply(mlp_out, anchor, self.rcfg)
        names = refine_ref.NAMES[:6 if self.cfg["version"] == 1 else 8]
        assert sorted(outs) == sorted(names)
        for k, name in enumerate(names):
            assert outs[name].shape == alone[k].shape and torch.equal(outs[name], alone[k]), (self.name, name)


@functools.lru_cache(maxsize=None)
def setup(name):
    return Setup(name)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", list(VARIANTS))
def test_mlp_values_tail_bits_and_row_independence(name, n):
    s = setup(name)
    outs, mlp_out = s.run(n)
    assert mlp_out.shape == (n, s.D)
    s.check_values(mlp_out)
    s.check_tail(outs, mlp_out, s.anchor[:n])
    # without mlp_out: the same bits
    bare, none = s.run(n, with_mlp=False)
    assert none is None
    for k in outs:
        assert torch.equal(bare[k], outs[k]), (name, n, k)
    # a row's result does not depend on n: the rows of the n = 1 000 call
    full, full_mlp = s.full
    assert torch.equal(full_mlp[:n], mlp_out)
    for k in outs:
        assert torch.equal(full[k][:n], outs[k]), (name, n, k)
    if n == s.n:   # the end-to-end distance to the float64 module: recorded, not asserted (see the module's docstring)
        for k, t in s.truth.items():
            if t.numel():
                err, ref = float((outs[k].double().cpu() - t).abs().max()), float(t.abs().max())
                print(f"{name} end to end {k}: max|native - truth| {err:.3e} (max|truth| {ref:.3e})")


def test_refined_columns_beyond_xyz_reach_anchor_out():
    """refine_manual beyond the first three columns (refine_module.py:82-84): anchor_out carries the refined scale columns and
    the refined columns from 10 on -- one fp32 addition each, so bit for bit -- and the heads are taken from them."""
    s = setup("R12")
    full, mlp_out = s.full
    refined = mlp_out[:, 3:12] + s.anchor[:, 3:12]
    assert torch.equal(full["anchor_out"][:, 3:6], refined[:, :3])
    assert torch.equal(full["anchor_out"][:, 10:12], refined[:, 7:9])
    assert torch.equal(full["anchor_out"][:, 12:], mlp_out[:, 12:])
    truth = s.truth["anchor_out"]
    assert float((full["anchor_out"].double().cpu() - truth)[:, 3:6].abs().max()) <= 1e-5 * float(truth[:, 3:6].abs().max())


def test_more_workgroups_than_the_chip_holds():
    """n = 40 000: 313 workgroups.  Its first 1 000 rows are the n = 1 000 case's; the yardstick Y is that case's."""
    s = setup("solid")
    n = 40000
    dev = s.feat.device
    feat, anchor, embed = make_inputs(s.D, 0, n, 77)
    feat[:s.n], anchor[:s.n], embed[:s.n] = s.feat.cpu(), s.anchor.cpu(), s.embed.cpu()
    state64 = {k: v.double().cpu() for k, v in s.state.items()}
    truth = refine_ref.mlp(state64, feat.double() + embed.double())
    feat, anchor, embed = feat.to(dev), anchor.to(dev), embed.to(dev)
    with torch.no_grad():
        anchor_out, pred, mlp_out = R.refine_fused(feat, anchor, embed, s.state, s.rcfg, return_mlp_output=True)
    outs = outputs_of(anchor_out, pred)
    s.check_values(mlp_out, truth)
    s.check_tail(outs, mlp_out, anchor)
    full, full_mlp = s.full
    assert torch.equal(mlp_out[:s.n], full_mlp)
    for k in outs:
        assert torch.equal(outs[k][:s.n], full[k])


@pytest.mark.parametrize("name", ["solid", "prob", "D43"])
def test_repeated_and_replayed_from_a_graph(name):
    s = setup(name)
    full, full_mlp = s.full
    again, again_mlp = s.run(s.n)
    assert torch.equal(again_mlp, full_mlp) and all(torch.equal(again[k], full[k]) for k in full)
    static = {}

    def body():
        static["res"] = s.run(s.n)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    outs, mlp_out = static["res"]
    for t in (*outs.values(), mlp_out):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(mlp_out, full_mlp)
    for k in full:
        assert torch.equal(outs[k], full[k]), (name, k)


@pytest.mark.parametrize("name", ["solid", "prob", "D43"])
def test_a_nan_row_changes_no_other_row(name):
    s = setup(name)
    full, full_mlp = s.full
    n = 300
    for which, row in (("feat", 37), ("embed", 0), ("anchor", 299), ("feat", 128)):
        args = dict(feat=s.feat[:n].clone(), anchor=s.anchor[:n].clone(), embed=s.embed[:n].clone())
        args[which][row] = float("nan")
        with torch.no_grad():
            anchor_out, pred, mlp_out = R.refine_fused(args["feat"], args["anchor"], args["embed"], s.state, s.rcfg, return_mlp_output=True)
        outs = outputs_of(anchor_out, pred)
        keep = torch.arange(n, device=mlp_out.device) != row
        assert torch.equal(mlp_out[keep], full_mlp[:n][keep])
        for k in outs:
            assert torch.equal(outs[k][keep], full[k][:n][keep]), (name, which, k)
        if which != "anchor":
            assert torch.isnan(mlp_out[row]).all()


@pytest.mark.parametrize("name", list(refine_ref.FAMILIES))
def test_modules(name):
    s = setup(name)
    module = s.module
    assert module.fused_mlp is False
    lead = lambda t: t.reshape(2, s.n // 2, -1)
    feat, anchor, embed = lead(s.feat), lead(s.anchor), lead(s.embed)

    def today(f, a, e):
        return R.refine(module.layers(f + e), a, module._cfg)

    def same(x, y):
        assert torch.equal(x[0], y[0]) and x[0].shape == y[0].shape
        assert len(x[1]) == len(y[1])
        for p, q in zip(x[1], y[1]):
            assert (p is None and q is None) or (p.shape == q.shape and torch.equal(p, q))

    try:
        with torch.no_grad():
            off = module(feat, anchor, embed)
            same(off, today(feat, anchor, embed))
            module.fused_mlp = True
            on = module(feat, anchor, embed)
            want = R.refine_fused(feat, anchor, embed, module.state_dict(), module._cfg)
            same(on, want)
            assert on[0].shape == (2, s.n // 2, s.D) and on[1].means.shape == (2, s.n // 2, 3)
            full, _ = s.full
            assert torch.equal(on[0].reshape(s.n, -1), full["anchor_out"])
        # autograd is recording and the parameters require grad: today's route, with its graph
        rec = module(feat, anchor, embed)
        assert rec[0].grad_fn is not None
        same(rec, today(feat, anchor, embed))
        with torch.no_grad():
            f2 = feat.clone()
        for p in module.parameters():
            p.requires_grad_(False)
        same(module(feat, anchor, embed), want)                                   # nothing requires grad: fused without no_grad
        rec = module(f2.requires_grad_(True), anchor, embed)                      # an input requires grad: today's route
        assert rec[0].grad_fn is not None
        same(rec, off)
    finally:
        module.fused_mlp = False
        for p in module.parameters():
            p.requires_grad_(True)
