"""The refinement step on the GPU (gaussianformer_amd.refine, gf_refine_forward / gf_refine_backward) against the float64
restatement of tests/refine_ref.py, with the float32 torch composition of the same restatement as the yardstick.

The rule, per output tensor and per column group (xyz, scale, rotation, opacity, semantics) of anchor_out, grad_output and
grad_anchor:   max|native - truth| <= 2 max|fp32 composition - truth| + 4 eps32 max|truth|.
Both are fp32 evaluations of one formula that differ in operation order and in exp / log, so a correct kernel lands in the
composition's error class, while a wrong clamp, column or sign is off by orders of magnitude; a fixed tolerance cannot serve,
because version 2's inverse sigmoid amplifies a rounding by up to 1e4 near its clamp.  Where the truth's gradient is exactly 0
(a clamp blocks it, or the column is not read) the native gradient is exactly 0.0.  The measured ratios are in DESIGN.md §3.12."""
import os

import numpy as np
import pytest
import torch

import refine_ref
from gaussianformer_amd import refine as R
from row_judge import EPS32, bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PC = [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0]


def case(version, n, S=17, opa=True, sem="softplus", xyz="sigmoid", restrict=True, Rn=3, extra_anchor=0, seed=0):
    cfg = dict(version=version, pc_range=PC, scale_range=[0.08, 0.64] if version == 1 else [0.01, 3.2], unit_xyz=[4.0, 4.0, 1.0],
               semantics=S > 0, semantic_dim=S, include_opa=opa, semantics_activation=sem, xyz_activation=xyz)
    if version == 1:
        cfg.update(restrict_xyz=restrict, refine_manual=list(range(Rn)))
    return dict(cfg=cfg, n=n, extra_anchor=extra_anchor, seed=seed)


def case_id(c):
    g = c["cfg"]
    return (f"v{g['version']}-n{c['n']}-D{10 + int(g['include_opa']) + g['semantic_dim']}-{g['xyz_activation']}-"
            f"{g['semantics_activation']}-r{int(g.get('restrict_xyz', False))}-R{len(g.get('refine_manual', []))}")


CASES = [case(v, n) if v == 1 else case(v, n, sem="identity") for v in (1, 2) for n in (1, 63, 64, 65, 1000, 25600)] + [
    case(1, 1000, S=18, sem="softmax", restrict=False, Rn=0),                                   # D 29
    case(1, 1000, S=0, opa=False, sem="softmax", xyz="identity", restrict=True, Rn=0),          # D 10
    case(1, 1000, S=0, sem="identity", xyz="identity", restrict=False, Rn=3, extra_anchor=3),   # D 11, a wider anchor
    case(1, 1000, S=18, opa=False, sem="identity"),                                             # gs144000's settings
    case(1, 1000, S=32, sem="softmax", restrict=False),                                         # D 43, the widest
    case(2, 1000, sem="softmax", xyz="identity"),
    case(2, 1000, S=0, opa=False, sem="softplus"),                                              # D 10
    case(2, 1000, S=0, sem="softmax"),                                                          # D 11
    case(2, 1000, S=18, sem="softplus", xyz="identity", extra_anchor=5),                        # D 29
]
BS = 2
PLANTS = 8


def inputs(c):
    """float64 (output, anchor) of [BS, n, .] whose values are float32 numbers, with the adversarial rows planted in the first
    rows (as many of the PLANTS as there are rows), and the number of planted rows."""
    g, n = c["cfg"], c["n"]
    opa, S = int(g["include_opa"]), g["semantic_dim"]
    D = 10 + opa + S
    Da = D + c["extra_anchor"]
    rng = np.random.default_rng(1000 + c["seed"] + 7 * n + D)
    o = rng.standard_normal((BS * n, D)) * 1.5
    a = rng.standard_normal((BS * n, Da)) * 1.5
    if g["xyz_activation"] == "sigmoid":
        # version 2: the moved centre of an unplanted row stays well inside the range (units 4, 4, 1 m of 100, 100, 8 m)
        a[:, :3] = rng.uniform(-1.0, 1.0, (BS * n, 3)) * np.array([2.5, 2.5, 1.5])
    else:                  # the columns are unit coordinates themselves
        o[:, :3] = rng.uniform(0.1, 0.4, (BS * n, 3))
        a[:, :3] = rng.uniform(0.1, 0.5, (BS * n, 3))
    planted = min(BS * n, PLANTS)
    sem0 = 10 + opa
    for k in range(planted):
        if k == 0:
            o[k, :sem0] = 12.0                      # beyond +9.21 in every safe_sigmoid
        elif k == 1:
            o[k, :sem0] = -12.0
        elif k == 2:
            o[k, sem0:] = 25.0                      # softplus above its threshold 20
            o[k, sem0::2] = 31.0
        elif k == 3:
            o[k, sem0:] = 80.0                      # softmax logits at +-80
            o[k, sem0 + 1::2] = -80.0
        elif k == 4:
            o[k, 6:10] = 0.0                        # zero quaternion
        elif k == 5:
            o[k, 6:10] = 5e-14                      # quaternion of norm 1e-13
        elif k == 6:
            o[k, :3], a[k, :3] = -12.0, -9.0        # version 2: the moved centre leaves the range below ...
        elif k == 7:
            o[k, :3], a[k, :3] = 12.0, 9.0          # ... and above
    f = lambda t: torch.from_numpy(t.astype(np.float32).astype(np.float64)).reshape(BS, n, -1)
    return f(o), f(a), planted


def clamp_sites(c, o, a):
    """[(name, float64 values [rows, k], bounds)] of every clamp (and softplus's switch, and normalize's eps) the step
    applies, from the float64 inputs."""
    g = c["cfg"]
    o, a = o.reshape(-1, o.shape[-1]), a.reshape(-1, a.shape[-1])
    sig = g["xyz_activation"] == "sigmoid"
    opa, S = int(g["include_opa"]), g["semantic_dim"]
    ss, unit_box = (-9.21, 9.21), (1e-6, 1 - 1e-6)
    sites = [("scale", o[:, 3:6], ss), ("quaternion norm", o[:, 6:10].norm(dim=-1, keepdim=True), (1e-12,))]
    if opa:
        sites.append(("opacity", o[:, 10:11], ss))
    if g["semantics_activation"] == "softplus" and S:
        sites.append(("softplus", o[:, 10 + opa:], (20.0,)))
    span = torch.tensor([PC[3 + i] - PC[i] for i in range(3)], dtype=torch.float64)
    if g["version"] == 1:
        x = o[:, :3]
        if g["restrict_xyz"]:
            sites.append(("restrict", x, ss))
            x = (2 * refine_ref.safe_sigmoid(x) - 1) * torch.tensor(refine_ref.unit_of(g), dtype=torch.float64)
        if len(g["refine_manual"]):
            assert g["refine_manual"] == [0, 1, 2]
            x = x + a[:, :3]
        sites.append(("xyz", x, ss if sig else unit_box))
    else:
        sites.append(("delta", o[:, :3], ss))
        sites.append(("anchor xyz", a[:, :3], ss if sig else unit_box))
        c0 = refine_ref.safe_sigmoid(a[:, :3]) if sig else a[:, :3].clamp(1e-6, 1 - 1e-6)
        delta = (2 * refine_ref.safe_sigmoid(o[:, :3]) - 1) * torch.tensor(refine_ref.unit_of(g), dtype=torch.float64)
        sites.append(("moved centre", c0 + delta / span, (1 - 0.9999, 0.9999) if sig else unit_box))
    return sites


def assert_margins(c, o, a, planted):
    """No value -- planted or not -- lies within 1e-3 (relative) of a clamp bound, so float32 and float64 take the same side
    everywhere; and the planted rows lie well beyond the bounds they are there for."""
    sites = dict((name, (v, b)) for name, v, b in clamp_sites(c, o, a))
    for name, (v, bounds) in sites.items():
        for b in bounds:
            gap = ((v - b).abs() / abs(b)).min()
            assert gap > 1e-3, (case_id(c), name, b, float(gap))
    beyond = lambda name, row, b, up: bool(((sites[name][0][row] > b * 1.05) if up else (sites[name][0][row] < b * 1.05)).all())
    assert beyond("scale", 0, 9.21, True) and (planted < 2 or beyond("scale", 1, -9.21, False))
    if "softplus" in sites and planted > 2:
        assert beyond("softplus", 2, 20.0, True)
    if planted > 5:
        assert float(sites["quaternion norm"][0][4]) == 0.0 and 0 < float(sites["quaternion norm"][0][5]) < 2e-13
    if planted > 7 and c["cfg"]["version"] == 2:
        lo, hi = sites["moved centre"][1]
        assert bool((sites["moved centre"][0][6] < lo * 0.5).all()) and bool((sites["moved centre"][0][7] > 1 + (1 - hi)).all())


def groups(c, name, t):
    """[(label, columns)] a tensor is judged by."""
    g = c["cfg"]
    opa, S = int(g["include_opa"]), g["semantic_dim"]
    if name not in ("anchor_out", "grad_output", "grad_anchor"):
        return [(name, t)] if t.numel() else []
    parts = [("xyz", t[..., :3]), ("scale", t[..., 3:6]), ("rotation", t[..., 6:10]), ("opacity", t[..., 10:10 + opa]),
             ("semantics", t[..., 10 + opa:10 + opa + S])]
    if t.shape[-1] > 10 + opa + S:
        parts.append(("beyond", t[..., 10 + opa + S:]))
    return [(f"{name}.{k}", v) for k, v in parts if v.numel()]


def run_all(c, o64, a64):
    """{name: tensor} of outputs and input gradients for truth (float64, CPU), composition (float32, GPU) and native."""
    dev = torch.device("cuda:0")
    g = c["cfg"]
    res = {}
    w64 = None
    for which in ("truth", "composition", "native"):
        dt, where = (torch.float64, "cpu") if which == "truth" else (torch.float32, dev)
        o = o64.detach().clone().to(dt).to(where).requires_grad_(True)
        a = a64.detach().clone().to(dt).to(where).requires_grad_(True)
        if which == "native":
            cfg = R.refine_config(g["version"], g["pc_range"], g["scale_range"], refine_ref.unit_of(g), g.get("restrict_xyz", False),
                                  g.get("refine_manual", ()), g["semantic_dim"], g["include_opa"], g["semantics_activation"],
                                  g["xyz_activation"])
            anchor_out, pred = R.refine(o, a, cfg)
            outs = dict(anchor_out=anchor_out, **{k: v for k, v in pred._asdict().items() if v is not None})
        else:
            outs = refine_ref.refine_tail(o, a, g)
        if w64 is None:
            rng = np.random.default_rng(5)
            w64 = {k: torch.from_numpy(rng.standard_normal(tuple(v.shape)).astype(np.float32).astype(np.float64)) for k, v in outs.items()}
        assert sorted(outs) == sorted(w64)
        refine_ref.weighted_sum(outs, {k: v.to(dt).to(where) for k, v in w64.items()}).backward()
        r = {k: v.detach().double().cpu() for k, v in outs.items()}
        # (an anchor the composition never reads -- version 1 with R = 0 -- gets no gradient from autograd: a zero one)
        r["grad_output"] = o.grad.double().cpu()
        r["grad_anchor"] = (torch.zeros_like(a) if a.grad is None else a.grad).double().cpu()
        res[which] = r
    return res


def judge(c, res, report=None):
    bad = []
    for name, truth in res["truth"].items():
        assert res["native"][name].shape == truth.shape, name
        for label, t in groups(c, name, truth):
            nat = dict(groups(c, name, res["native"][name]))[label]
            comp = dict(groups(c, name, res["composition"][name]))[label]
            assert torch.isfinite(nat).all(), label
            err, ref = float((nat - t).abs().max()), float((comp - t).abs().max())
            limit = bound(ref, t)
            print(f"{case_id(c)} {label}: native {err:.3e} composition {ref:.3e} bound {limit:.3e} "
                  f"ratio {err / limit if limit else 0.0:.3f}")
            if report is not None:
                report.append((case_id(c), label, err, ref, limit))
            if not err <= limit:
                bad.append((label, err, ref, limit))
            if name.startswith("grad_"):
                zero = t == 0
                if not bool((nat[zero] == 0).all()):
                    bad.append((label, "non-zero where the truth's gradient is exactly 0"))
    assert not bad, (case_id(c), bad)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_margins_hold_on_the_float64_inputs(c):
    o, a, planted = inputs(c)
    assert_margins(c, o, a, planted)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_values_and_gradients_against_float64(c):
    o, a, planted = inputs(c)
    assert_margins(c, o, a, planted)
    judge(c, run_all(c, o, a))


def _fixture(name):
    with np.load(os.path.join(ROOT, "tests", "golden", "refine.npz")) as z:
        return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + ".")}


@pytest.mark.parametrize("name", list(refine_ref.FAMILIES))
def test_modules_against_the_fixture(name):
    """The drop-in modules with the reference's weights: outputs, input gradients and every parameter gradient.  Truth: the
    float64 whole-module restatement; yardstick: the reference's own fp32 results (the fixture)."""
    dev = torch.device("cuda:0")
    fx, cfg = _fixture(name), refine_ref.FAMILIES[name]
    keys = [str(k) for k in fx["keys"]]
    cls = R.SparseGaussian3DRefinementModule if cfg["version"] == 1 else R.SparseGaussian3DRefinementModuleV2
    module = cls(embed_dims=32, phi_activation="sigmoid", xyz_coordinate="cartesian", **{k: v for k, v in cfg.items() if k != "version"})
    module.load_state_dict({k: torch.from_numpy(fx["state." + k]) for k in keys}, strict=True)
    module.to(dev)
    leaf = lambda k, dt, where: torch.from_numpy(fx[k]).to(dt).to(where).requires_grad_(True)
    # truth
    state = {k: torch.from_numpy(fx["state." + k]).double().requires_grad_(True) for k in keys}
    t_in = [leaf(k, torch.float64, "cpu") for k in ("instance_feature", "anchor", "anchor_embed")]
    t_out = refine_ref.refine_module(state, *t_in, cfg)
    refine_ref.weighted_sum(t_out, refine_ref.fixed_weights(t_out)).backward()
    truth = {"out." + k: v.detach() for k, v in t_out.items()}
    truth.update({"grad.instance_feature": t_in[0].grad, "grad.anchor": t_in[1].grad})
    truth.update({"grad.param." + k: v.grad for k, v in state.items()})
    # native
    n_in = [leaf(k, torch.float32, dev) for k in ("instance_feature", "anchor", "anchor_embed")]
    anchor_out, pred = module(*n_in)
    n_out = dict(anchor_out=anchor_out, **{k: v for k, v in pred._asdict().items() if v is not None})
    assert sorted(n_out) == sorted(t_out)
    refine_ref.weighted_sum(n_out, refine_ref.fixed_weights(n_out)).backward()
    native = {"out." + k: v.detach() for k, v in n_out.items()}
    native.update({"grad.instance_feature": n_in[0].grad, "grad.anchor": n_in[1].grad})
    native.update({"grad.param." + k: p.grad for k, p in module.named_parameters()})
    assert torch.equal(n_in[2].grad, n_in[0].grad)
    bad = []
    c = dict(cfg=cfg, n=0)
    for k, t in truth.items():
        nat, comp = native[k].double().cpu(), torch.from_numpy(fx[k]).double()
        assert nat.shape == t.shape == comp.shape, k
        short = {"out.anchor_out": "anchor_out", "grad.anchor": "grad_anchor"}.get(k, k)
        for (label, tt), (_, nn_), (_, cc) in zip(groups(c, short, t), groups(c, short, nat), groups(c, short, comp)):
            err, ref = float((nn_ - tt).abs().max()), float((cc - tt).abs().max())
            limit = bound(ref, tt)
            print(f"{name} {label}: native {err:.3e} reference fp32 {ref:.3e} bound {limit:.3e}")
            if not err <= limit:
                bad.append((label, err, ref, limit))
    assert not bad, bad


def _solid(n=1000):
    c = case(1, n)
    o, a, _ = inputs(c)
    g = c["cfg"]
    cfg = R.refine_config(1, g["pc_range"], g["scale_range"], refine_ref.unit_of(g), True, [0, 1, 2], 17, True, "softplus")
    return c, o.float().cuda(), a.float().cuda(), cfg


def _flat(o, a, cfg):
    o = o.reshape(-1, o.shape[-1]).clone().requires_grad_(True)
    a = a.reshape(-1, a.shape[-1]).clone().requires_grad_(True)
    outs = R.RefineFunction.apply(o, a, cfg)
    return o, a, outs


def test_backward_with_any_subset_of_gradients_absent():
    """Each output alone, and all but each, as the scalar's terms: an absent gradient equals a zero one, so the gradients are
    additive over the outputs -- the sum of the single-output gradients equals the all-outputs gradient up to fp32 addition."""
    for version in (1, 2):
        c = case(version, 300, sem="softmax")
        o64, a64, _ = inputs(c)
        g = c["cfg"]
        cfg = R.refine_config(version, g["pc_range"], g["scale_range"], refine_ref.unit_of(g), g.get("restrict_xyz", False),
                              g.get("refine_manual", ()), 17, True, "softmax")
        rng = torch.Generator().manual_seed(3)
        names = refine_ref.NAMES[:6 if version == 1 else 8]
        singles = []
        weights = None
        for subset in [[k] for k in range(len(names))] + [list(range(len(names)))]:
            o, a, outs = _flat(o64.float().cuda(), a64.float().cuda(), cfg)
            if weights is None:
                weights = [torch.randn(t.shape, generator=rng).cuda() for t in outs]
            sum((outs[k] * weights[k]).sum() for k in subset).backward()
            assert torch.isfinite(o.grad).all() and torch.isfinite(a.grad).all()
            singles.append((o.grad.double(), a.grad.double()))
        (go_all, ga_all), parts = singles[-1], singles[:-1]
        go_sum, ga_sum = sum(p[0] for p in parts), sum(p[1] for p in parts)
        scale = float(sum(p[0].abs() for p in parts).max())
        assert float((go_sum - go_all).abs().max()) <= 16 * EPS32 * scale
        assert float((ga_sum - ga_all).abs().max()) <= 16 * EPS32 * float(sum(p[1].abs() for p in parts).max())
        # and the truth of one single-output case: means only
        o, a, outs = _flat(o64.float().cuda(), a64.float().cuda(), cfg)
        outs[1].sum().backward()
        ot, at = o64.clone().requires_grad_(True), a64.clone().requires_grad_(True)
        refine_ref.refine_tail(ot, at, g)["means"].sum().backward()
        assert float((o.grad.double().cpu() - ot.grad.reshape(o.shape)).abs().max()) <= 1e-4 * float(ot.grad.abs().max())


def test_null_gradient_pointers_equal_zero_tensors():
    """gf_refine_backward called directly: every subset pattern of NULL grad_* pointers (each alone, each alone absent, all
    absent) gives the very bits of the call with tensors of zeros in their place; and autograd hands the entry point NULL for
    an unused output (set_materialize_grads(False)), which the additivity test above relies on."""
    import ctypes
    from gaussianformer_amd import _lib
    for version in (1, 2):
        c = case(version, 200, sem="softmax")
        o64, a64, _ = inputs(c)
        g = c["cfg"]
        cfg = R.refine_config(version, g["pc_range"], g["scale_range"], refine_ref.unit_of(g), g.get("restrict_xyz", False),
                              g.get("refine_manual", ()), 17, True, "softmax")
        o = o64.float().cuda().reshape(-1, 28).contiguous()
        a = a64.float().cuda().reshape(-1, 28).contiguous()
        n = o.shape[0]
        widths = [28, 3, 3, 4, 1, 17] + ([3, 3] if version == 2 else [0, 0])
        gen = torch.Generator().manual_seed(11)
        grads = [torch.randn(n, w, generator=gen).cuda() for w in widths]
        consts = (ctypes.c_double * 11)(*cfg.consts)

        def backward(present):
            go, ga = torch.full_like(o, float("nan")), torch.full_like(a, float("nan"))
            _lib.call("gf_refine_backward", o.device, n, 28, 28, version, cfg.flags, cfg.R, cfg.S, ctypes.cast(consts, ctypes.c_void_p),
                      o, a, *[t if t is not None and t.numel() else None for t in present], go, ga)
            return go, ga

        live = [k for k, w in enumerate(widths) if w]
        patterns = [[k] for k in live] + [[j for j in live if j != k] for k in live] + [[]]
        for keep in patterns:
            null = backward([grads[k] if k in keep else None for k in range(8)])
            zero = backward([grads[k] if k in keep else torch.zeros_like(grads[k]) for k in range(8)])
            assert torch.equal(null[0], zero[0]) and torch.equal(null[1], zero[1]), (version, keep)
            assert torch.isfinite(null[0]).all() and torch.isfinite(null[1]).all()
        assert not backward([None] * 8)[0].any()
        # through autograd: only the used output's gradient arrives
        seen = []
        orig = _lib.call

        def spy(name, device, *args):
            if name == "gf_refine_backward":
                seen.append([x is None for x in args[10:18]])
            return orig(name, device, *args)

        _lib.call = spy
        try:
            oo, aa, outs = _flat(o, a, cfg)
            outs[1].sum().backward()
        finally:
            _lib.call = orig
        assert seen == [[True, False] + [True] * 6]


def test_bitwise_reproducible_graph_and_stream():
    c, o, a, cfg = _solid(1000)
    w = None

    def step(o_, a_):
        o1, a1, outs = _flat(o_, a_, cfg)
        nonlocal w
        if w is None:
            w = [torch.randn_like(t) for t in outs]
        sum((t * k).sum() for t, k in zip(outs, w)).backward()
        return [t.detach() for t in outs] + [o1.grad, a1.grad]

    first, second = step(o, a), step(o, a)
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    # another stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        third = step(o, a)
    s.synchronize()
    for x, y in zip(first, third):
        assert torch.equal(x, y)
    # captured graph: forward and backward entry points through the Function's two halves
    of, af = o.reshape(-1, o.shape[-1]).contiguous(), a.reshape(-1, a.shape[-1]).contiguous()
    static = {}

    def body():
        oo = of.detach().requires_grad_(True)
        aa = af.detach().requires_grad_(True)
        outs = R.RefineFunction.apply(oo, aa, cfg)
        grads = torch.autograd.grad(outs, (oo, aa), w)
        static["res"] = [t.detach() for t in outs] + list(grads)

    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            body()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for t in static["res"]:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(first, static["res"]):
        assert torch.equal(x, y)


def test_chain_without_copies():
    """anchor_out feeds the key points, the prediction feeds the splat, as they are: contiguous, of the reference's shapes."""
    from gaussianformer_amd.key_points import SparseGaussian3DKeyPointsGenerator
    import local_aggregate
    dev = torch.device("cuda:0")
    bs, A, E = 1, 600, 32
    module = R.SparseGaussian3DRefinementModule(
        embed_dims=E, pc_range=[-8.0, -8.0, -2.0, 8.0, 8.0, 2.0], scale_range=[0.1, 0.6], restrict_xyz=True,
        unit_xyz=[1.0, 1.0, 0.5], refine_manual=[0, 1, 2], semantics=True, semantic_dim=18, include_opa=True,
        semantics_activation="softplus").to(dev)
    g = torch.Generator().manual_seed(0)
    feat, embed = (torch.randn(bs, A, E, generator=g).to(dev) for _ in range(2))
    anchor = torch.randn(bs, A, 29, generator=g).to(dev)
    anchor_out, pred = module(feat, anchor, embed)
    assert anchor_out.shape == (bs, A, 29) and pred.means.shape == (bs, A, 3) and pred.scales.shape == (bs, A, 3)
    assert pred.rotations.shape == (bs, A, 4) and pred.opacities.shape == (bs, A, 1) and pred.semantics.shape == (bs, A, 18)
    assert pred.original_means is None and pred.delta_means is None
    for t in (anchor_out, *pred[:5]):
        assert t.is_contiguous() and torch.isfinite(t).all()
    kps = SparseGaussian3DKeyPointsGenerator(embed_dims=E, num_learnable_pts=2, fix_scale=[[0, 0, 0], [0.45, 0, 0]],
                                             pc_range=module.pc_range, scale_range=module.scale_range).to(dev)
    ptr = anchor_out.data_ptr()
    kp = kps(anchor_out, feat)
    assert kp.shape == (bs, A, 4, 3) and torch.isfinite(kp).all() and anchor_out.data_ptr() == ptr
    H, W, D = 32, 32, 8
    agg = local_aggregate.LocalAggregator(3, H, W, D, [-8.0, -8.0, -2.0], 0.5, check_inputs=False).to(dev)
    ax = [(torch.arange(k, dtype=torch.float32) + 0.5) * 0.5 + lo for k, lo in zip((H, W, D), (-8.0, -8.0, -2.0))]
    pts = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(1, -1, 3).to(dev)
    out = agg.forward_from_rotations(pts, pred.means, pred.opacities.squeeze(-1), pred.semantics, pred.scales, pred.rotations)
    assert torch.isfinite(out).all()
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in module.parameters())
