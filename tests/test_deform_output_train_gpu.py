"""The training step of the deformable block's dense back on the GPU: ``gf_deform_output_forward_train`` /
``gf_deform_output_backward`` under ``deformable_output_autograd``, the deformable block's ``native_training``, the sparse
block's ``native_tail_training`` and the encoder's ``fold_training`` above them.

Values.  The truth is float64 autograd of ``sum(out * w)`` through the restatement (tests/deform_output_train_ref.py).  The op
has no ReLU: no row is exempt.  Per tensor ``max|native - truth| <= 2 Y + 4 eps32 max|truth|`` (tests/row_judge.py): for ``out``
and the three per-row gradients Y is ``max|float32 torch composition on this GPU - truth|`` over the variant's 1 000 rows
(every smaller n is a prefix of them, the 8 449-row case starts with them); for a parameter, relative to the leaf's
``max|truth|``, the largest relative error of the float32 composition over the leaves of its kind at the same n.  The
variant's first four rows of ``features`` are planted (zeros, 1e-30, +-1e4) and the +-1e4 rows set both sides of the per-row
bounds, so the rule is applied a second time to the ordinary rows alone.  The measured ratios are printed (-s) and recorded in
DESIGN.md §3.13f.

Invariants are bitwise.  Nothing here reads past a buffer's end or inspects code."""
import functools
import re

import pytest
import torch
import torch.nn as nn

import deform_block_ref as ref
import deform_output_train_ref as tr
from gaussianformer_amd import _lib
from gaussianformer_amd.deformable_block import deformable_output, deformable_output_autograd, output_train_sizes
from row_judge import EPS32, Guarded, bound, held, judge_leaves, max_error, ptr_table, spy  # noqa: F401  (spy is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B = _lib.GF_DEFORM_OUTPUT_WGRAD_ROWS
N_VARIANT, N_BIG, PLANTED = 1000, 8449, 4
EDGES = (1, 31, 32, 33, 127, 128, 129, N_VARIANT, B - 1, B, B + 1)
PER_ROW = tr.PER_ROW


class Case:
    """A variant's weights and its 8 449 rows on the GPU (the first 1 000 are the family), and per n the three sets of results."""

    def __init__(self, name, seed=0):
        self.name = name
        self.mode, self.has_res, self.has_norm = tr.VARIANTS[name]
        sd = tr.weights(self.has_norm, seed)
        self.sd, self.sd64 = tr.cast(sd, device=DEV), tr.cast(sd, torch.float64, DEV)
        self.x = tr.planted(tr.fixed_input(N_BIG, 128, 61 + seed)).to(DEV)
        self.f = tr.fixed_input(N_BIG, 128, 71 + seed).to(DEV) if self.mode != "none" else None
        self.res = tr.fixed_input(N_BIG, 128, 81 + seed).to(DEV) if self.has_res else None
        self.width = 256 if self.mode == "cat" else 128

    def inputs(self, n, rows=None):
        pick = (lambda t: t[:n].contiguous()) if rows is None else (lambda t: t[rows].contiguous())
        return tuple(None if t is None else pick(t) for t in (self.x, self.f, self.res))

    def restated(self, x, f, res, sd):
        return tr.output_train_ref(x, f, res, sd, self.mode)

    def native(self, x, f, res, sd):
        return deformable_output_autograd(x, (sd["output_proj.weight"], sd["output_proj.bias"]), f, self.mode, res, tr.norm_of(sd))

    def plain(self, x, f, res):
        with torch.no_grad():
            return deformable_output(x, (self.sd["output_proj.weight"], self.sd["output_proj.bias"]), f, self.mode, res, tr.norm_of(self.sd))

    @functools.lru_cache(maxsize=None)
    def grads(self, n):
        x, f, res = self.inputs(n)
        d = lambda t: None if t is None else t.double()
        return (tr.gradients(self.restated, d(x), d(f), d(res), self.sd64), tr.gradients(self.restated, x, f, res, self.sd),
                tr.gradients(self.native, x, f, res, self.sd))

    def step(self, x, f, res, go, sd=None):
        """The native results for an explicit cotangent ``go``: ``{"out", per-row gradients, parameter gradients}``."""
        sd = self.sd if sd is None else sd
        ins = {"features": x, "instance_feature": f, "residual": res}
        ins = {k: v.detach().clone().requires_grad_(True) for k, v in ins.items() if v is not None}
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
        out = self.native(ins["features"], ins.get("instance_feature"), ins.get("residual"), leaves)
        wanted = {**ins, **leaves}
        got = dict(zip(wanted, torch.autograd.grad(out, list(wanted.values()), grad_outputs=go)))
        return {"out": out.detach(), **got}


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def cotangent(n, width):
    return tr.output_weights((n, width), torch.float32).to(DEV)


def judged(c, n):
    """Every result of case ``c`` at ``n`` rows against its bound, the per-row tensors a second time on the ordinary rows."""
    truth, t32, native = c.grads(n)
    ytruth, y32, _ = c.grads(N_VARIANT)
    rows = [k for k in PER_ROW if k in truth]
    what = f"{c.name} n={n}"
    worst = judge_leaves(native, truth, t32, tr.kind, what, per_row=PER_ROW, row_yardstick={k: max_error(y32[k], ytruth[k]) for k in rows})
    if n > PLANTED:
        for k in rows:
            b = bound(max_error(y32[k][PLANTED:], ytruth[k][PLANTED:]), truth[k][PLANTED:])
            held(f"{what} {k}, ordinary rows", native[k][PLANTED:], truth[k][PLANTED:], b)
    assert set(native) == set(truth)
    return native, worst


# ---- 1. values ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("name", list(tr.VARIANTS))
def test_values(name, n):
    judged(case(name), n)


def test_values_on_the_128_row_kernels():
    """n = 8 449: beyond 32 rows per compute unit the plain forward is its 128-row kernel; seventeen weight-gradient blocks
    with a ragged tail of one tile and one row."""
    for name in ("none_res_norm", "cat"):
        c = case(name)
        native, _ = judged(c, N_BIG)
        assert torch.equal(native["out"], c.plain(*c.inputs(N_BIG)))


# ---- 2. bitwise --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(tr.VARIANTS))
def test_out_is_the_plain_forward_s(name):
    c = case(name)
    for n in EDGES + (N_BIG,):
        x, f, res = c.inputs(n)
        out = c.native(x.clone().requires_grad_(True), f, res, c.sd)
        assert out.requires_grad and torch.equal(out.detach(), c.plain(x, f, res)), n


@pytest.mark.parametrize("name", ["none_res_norm", "cat", "add_norm"])
def test_two_calls_agree(name):
    c = case(name)
    n = 2 * B + 77      # three weight-gradient blocks, the last ragged
    x, f, res = c.inputs(n)
    go = cotangent(n, c.width)
    a, b = c.step(x, f, res, go), c.step(x, f, res, go)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", ["none_res_norm", "cat", "add_norm", "add"])
def test_a_row_alone_is_the_row_among_others(name):
    """n = 1 against the same row at rows 0, 127, 128, 999 of 1 000 and at rows of 8 449 (the 128-row forward)."""
    c = case(name)
    for n, rows in ((N_VARIANT, (0, 127, 128, 999)), (N_BIG, (0, 4097, N_BIG - 1))):
        go = cotangent(n, c.width)
        full = c.step(*c.inputs(n), go)
        for r in rows:
            one = c.step(*c.inputs(1, rows=slice(r, r + 1)), go[r:r + 1].contiguous())
            for k in PER_ROW:
                if k in full:
                    assert torch.equal(one[k], full[k][r:r + 1]), (k, n, r)


def test_the_instance_gradient_is_what_the_mode_says():
    c = case("cat")
    n = 777
    go = cotangent(n, 256)
    got = c.step(*c.inputs(n), go)
    assert torch.equal(got["instance_feature"], go[:, 128:])
    # "add" with a residual and a norm: both receive g_s
    a = case("add_norm")
    x, f, _ = a.inputs(n)
    res = case("none_res_norm").res[:n].contiguous()
    got = a.step(x, f, res, cotangent(n, 128))
    assert torch.equal(got["instance_feature"], got["residual"]) and bool(got["residual"].abs().sum() > 0)
    # ... and without a norm g_s is grad_out itself
    p = case("add")
    got = p.step(*p.inputs(n)[:2], res, cotangent(n, 128))
    assert torch.equal(got["instance_feature"], cotangent(n, 128)) and torch.equal(got["residual"], cotangent(n, 128))


def _raw_step(c, n, tail=4096, fill=12345.0, garbage=float("nan")):
    """Both launching entry points on caller-made buffers with ``tail`` sentinel elements behind every output, ``saved`` and the
    workspace, the parameter gradients prefilled with ``garbage``: the results and whether every sentinel survived."""
    x, f, res = c.inputs(n)
    params = [c.sd.get(k) for k in tr.KEYS]
    table = ptr_table(params)
    grads = [None if p is None else Guarded(4 * p.numel(), DEV, 4 * tail, fill, body=garbage) for p in params]
    saved_bytes, work_bytes = output_train_sizes(n, c.mode, c.has_norm)
    out = Guarded(4 * n * c.width, DEV, 4 * tail, fill, body=fill)
    gx, gi, gr = [Guarded(4 * n * 128, DEV, 4 * tail, fill, body=fill) for _ in range(3)]
    saved, work = [Guarded(nbytes, DEV, tail, 0x5A, body=0x5A) for nbytes in (saved_bytes, work_bytes)]
    mode = {"none": 0, "add": 1, "cat": 2}[c.mode]
    _lib.call("gf_deform_output_forward_train", DEV, n, 128, mode, x, f, table, res, out.buf, saved.buf if saved_bytes else None, saved_bytes)
    go = cotangent(n, c.width)
    _lib.call("gf_deform_output_backward", DEV, n, 128, mode, x, table, saved.buf if saved_bytes else None, go, gx.buf,
              gi.buf if f is not None else None, gr.buf if res is not None else None,
              ptr_table([None if g is None else g.buf for g in grads]), work.buf, work_bytes)
    regions = [out, gx, gi, gr, saved, work] + [g for g in grads if g is not None]
    intact = all(g.intact() for g in regions)
    untouched = (f is not None or bool((gi.floats(n, 128) == fill).all())) and (res is not None or bool((gr.floats(n, 128) == fill).all()))
    results = {"out": out.floats(n, c.width), "features": gx.floats(n, 128), "instance_feature": gi.floats(n, 128), "residual": gr.floats(n, 128)}
    results.update({k: g.floats(*p.shape) for k, g, p in zip(tr.KEYS, grads, params) if g is not None})
    return results, intact and untouched


@pytest.mark.parametrize("n", [1, 33, 129, B + 1])
@pytest.mark.parametrize("name", list(tr.VARIANTS))
def test_nothing_is_written_beyond_an_end_and_garbage_is_overwritten(name, n):
    """Sentinels behind every output, the saved region and the workspace survive; every present parameter's gradient, its
    buffer prefilled with NaN, is the function's bit for bit: stored, not accumulated."""
    c = case(name)
    raw, intact = _raw_step(c, n)
    assert intact
    native = c.step(*c.inputs(n), cotangent(n, c.width))
    for k in native:
        assert torch.equal(raw[k], native[k]), k
    assert set(native) - set(PER_ROW) == set(c.sd)


def test_no_rows_zero_fill_the_parameter_gradients():
    for name in ("none_res_norm", "cat"):
        c = case(name)
        params = [c.sd.get(k) for k in tr.KEYS]
        grads = [None if p is None else torch.full_like(p, float("nan")) for p in params]
        mode = {"none": 0, "add": 1, "cat": 2}[c.mode]
        assert output_train_sizes(0, c.mode, c.has_norm) == (0, 0)
        _lib.call("gf_deform_output_forward_train", DEV, 0, 128, mode, None, None, ptr_table(params), None, None, None, 0)
        _lib.call("gf_deform_output_backward", DEV, 0, 128, mode, None, ptr_table(params), None, None, None, None, None, ptr_table(grads), None, 0)
        assert all(g is None or bool((g == 0).all()) for g in grads)
        empty = c.native(torch.empty(0, 128, device=DEV, requires_grad=True), None if c.f is None else c.f[:0], None if c.res is None else c.res[:0], c.sd)
        assert empty.shape == (0, c.width)


@pytest.mark.parametrize("name", ["none_res_norm", "cat", "add_norm"])
def test_a_nan_stays_in_its_row(name):
    """A NaN in one row of grad_out, and one in features: exactly that row of the per-row outputs changes, the others stay bit
    for bit; the parameter gradients are NaN where the float32 torch composition's are."""
    c = case(name)
    n, bad = 300, 77
    x, f, res = c.inputs(n)
    go = cotangent(n, c.width)
    clean = c.step(x, f, res, go)
    keep = torch.arange(n, device=DEV) != bad
    rows = [k for k in PER_ROW if k in clean]
    # in grad_out (its left half with "cat")
    g2 = go.clone()
    g2[bad, 5] = float("nan")
    got = c.step(x, f, res, g2)
    assert torch.equal(got["out"], clean["out"])
    for k in rows[1:]:
        assert torch.equal(got[k][keep], clean[k][keep]), k
    assert bool(torch.isnan(got["features"][bad]).all())
    if c.has_norm:
        assert all(bool(torch.isnan(got[k][bad]).all()) for k in rows[1:])
    elif c.mode == "cat":      # the right half was clean: so is grad_instance
        assert torch.equal(got["instance_feature"], clean["instance_feature"])
    # in features: the forward's row, and through the saved row the backward's where there is a norm
    x2 = x.clone()
    x2[bad, 100] = float("nan")
    got = c.step(x2, f, res, go)
    for k in rows:
        assert torch.equal(got[k][keep], clean[k][keep]), k
    assert bool(torch.isnan(got["out"][bad, :128]).all())
    if c.has_norm:
        assert all(bool(torch.isnan(got[k][bad]).all()) for k in rows[1:])
    else:                      # linear: the data gradients do not read features
        assert all(torch.equal(got[k], clean[k]) for k in rows[1:])
    t32 = tr.gradients(c.restated, x2, f, res, c.sd)
    for k in c.sd:
        assert torch.equal(torch.isnan(got[k]), torch.isnan(t32[k])), k


def test_graph_replay_equals_eager():
    c = case("none_res_norm")
    n = 777
    x, f, res = c.inputs(n)
    go = cotangent(n, 128)
    eager = c.step(x, f, res, go)
    xl, rl = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in c.sd.items()}
    keys = list(leaves)

    def step():
        out = c.native(xl, None, rl, leaves)
        return out, torch.autograd.grad(out, [xl, rl] + [leaves[k] for k in keys], grad_outputs=go)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, got = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), eager["out"]) and torch.equal(got[0], eager["features"]) and torch.equal(got[1], eager["residual"])
    for k, g in zip(keys, got[2:]):
        assert torch.equal(g, eager[k]), k


def test_entry_points_refuse_on_the_device_too():
    c = case("add_norm")
    n = 64
    x, f, _ = c.inputs(n)
    params = [c.sd.get(k) for k in tr.KEYS]
    grads = [torch.empty_like(p) for p in params]
    saved_bytes, work_bytes = output_train_sizes(n, "add", True)
    saved, work = torch.empty(saved_bytes, dtype=torch.uint8, device=DEV), torch.empty(work_bytes, dtype=torch.uint8, device=DEV)
    fail = r"failed \(code -1\): .*"
    with pytest.raises(RuntimeError, match=fail + "grad_features aliases an input"):
        _lib.call("gf_deform_output_backward", DEV, n, 128, 1, x, ptr_table(params), saved, f, x, None, None, ptr_table(grads), work, work_bytes)
    with pytest.raises(RuntimeError, match=fail + "grad_instance aliases the workspace"):
        _lib.call("gf_deform_output_backward", DEV, n, 128, 1, x, ptr_table(params), saved, f, torch.empty_like(x), work, None, ptr_table(grads),
                  work, work_bytes)
    with pytest.raises(RuntimeError, match=r"failed \(code -2\): .*workspace of"):
        _lib.call("gf_deform_output_backward", DEV, n, 128, 1, x, ptr_table(params), saved, f, torch.empty_like(x), None, None, ptr_table(grads),
                  work, work_bytes - 1)


# ---- 3. the deformable block ---------------------------------------------------------------------------------------------------

def _module_step(m, s, cfg, post, norm_pair, native):
    """``(out, {leaf name: gradient})`` of the fixed scalar through the module: the inputs, the maps and every parameter."""
    leaves = {"inst": s["inst"], "anchor": s["anchor"], "emb": s["emb"], **{f"map{i}": f for i, f in enumerate(s["maps"])}}
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
    params = dict(m.named_parameters())
    norm = None
    if post:
        norm = nn.LayerNorm(128).to(DEV)
        norm.load_state_dict({"weight": norm_pair[0], "bias": norm_pair[1]})
        params.update({"norm.weight": norm.weight, "norm.bias": norm.bias})
    for p in params.values():
        p.grad = None
    ran = []
    hooks = [mod.register_forward_hook(lambda *a: ran.append(1)) for mod in [m.output_proj] + ([norm] if post else [])]
    m.native_training = native
    try:
        metas = dict(projection_mat=s["pm"], image_wh=s["wh"])
        kw = dict(residual=leaves["inst"], norm=norm) if post else {}
        out = m(leaves["inst"], leaves["anchor"], leaves["emb"], [leaves[f"map{i}"] for i in range(len(s["maps"]))], metas, **kw)
        wanted = {**leaves, **params}
        grads = dict(zip(wanted, torch.autograd.grad((out * tr.output_weights(out.shape, torch.float32).to(DEV)).sum(), list(wanted.values()))))
    finally:
        del m.native_training
        for h in hooks:
            h.remove()
    return out.detach(), grads, len(ran)


@pytest.mark.parametrize("name", ["solid", "prob"])
def test_deformable_block_trains_its_back_end_natively(name, spy):
    """A = 300 on the synthetic pyramid, solid ("cat") and prob ("none" + residual + norm): the launches, no call of
    ``output_proj`` or of the norm module, and the output and every gradient held to the float64 module restatement with the
    same module's torch route (``native_training = False``) as the yardstick."""
    from test_deform_block_gpu import SHAPES, module_of, scene
    m, cfg, sd = module_of(name)
    s = scene()
    post = SHAPES[name]["post"]
    pair = (sd["norm.weight"].to(DEV), sd["norm.bias"].to(DEV)) if post else None
    del spy[:]
    out, native, ran = _module_step(m, s, cfg, post, pair, True)
    assert ran == 0
    assert spy.count("gf_deform_output_forward_train") == 1 and spy.count("gf_deform_output_backward") == 1
    assert spy.index("gf_deform_output_forward_train") < spy.index("gf_deform_output_backward") and "gf_deform_output_forward" not in spy
    assert spy.index("gf_deform_output_backward") < spy.index("gf_daf_fused_backward")     # the tail's backward comes first
    today = [n for n in spy if not n.startswith("gf_deform_output")]
    del spy[:]
    out32, torch32, ran = _module_step(m, s, cfg, post, pair, False)
    assert ran == (2 if post else 1) and spy == today                # with the attribute False: today's launch list
    assert m.native_training is False

    d = lambda t: t.detach().double()
    sd64 = tr.cast(sd, torch.float64, DEV)
    inputs = {"inst": d(s["inst"]), "anchor": d(s["anchor"]), "emb": d(s["emb"]), **{f"map{i}": d(f) for i, f in enumerate(s["maps"])}}

    def restated(inst, anchor, emb, *rest):
        maps, leaves = list(rest[:-1]), rest[-1]
        return ref.module_ref(leaves, cfg, inst, anchor, emb, maps, d(s["pm"]), d(s["wh"]), residual=inst if post else None)
    import row_ref
    truth = row_ref.scalar_gradients(restated, inputs, sd64, with_out=True)
    held(f"module {name} out", out, truth["out"], bound(max_error(out32, truth["out"]), truth["out"]))
    assert set(native) == set(truth) - {"out"}
    for k in native:
        held(f"module {name} d/d {k}", native[k], truth[k], bound(max_error(torch32[k], truth[k]), truth[k]))


# ---- 4. the sparse block -------------------------------------------------------------------------------------------------------

FWD, BWD = "gf_deform_output_forward_train", "gf_deform_output_backward"


@pytest.mark.parametrize("family", ["single_proj", "multi_proj"])
def test_sparse_block_trains_its_tail_natively(family, spy):
    """602 points, width 128 (tests/test_subm_stage_train_gpu.py's block): with ``native_tail_training`` the tail is the new
    Function behind the stages -- ``output_proj`` and the passed norm never run as torch layers -- and every gradient is held
    to the float64 block with the native stages' masks, the all-torch module as the yardstick; without it the launch lists
    are today's."""
    from test_sparse_block_tail_gpu import BS, BUILD, G, block
    from test_sparse_block_tail_gpu import K as BLOCK_K
    import test_subm_stage_train_gpu as st
    b = block(family, "sum")
    m = b.m
    ran = []
    hooks = [mod.register_forward_hook(lambda *a: ran.append(1)) for mod in (m.output_proj, b.norm)]
    m.native_tail_training = True
    try:
        del spy[:]
        out, native = st._step(b, True)
    finally:
        del m.native_tail_training
    stages = {"single_proj": [st.APPLY], "multi_proj": [st.TRAIN] * 3}[family]
    behind = {"single_proj": [st.APPLY, st.WGRAD], "multi_proj": [st.BACK, st.WGRAD, st.FUSED, st.WGRAD, st.FUSED, st.WGRAD, st.APPLY]}[family]
    assert spy == BUILD + stages + [FWD, BWD] + behind
    assert not ran
    del spy[:]
    st._step(b, True)                                               # the stages' switch alone: today's route
    assert spy == st.NATIVE[family, "sum"] and len(ran) == 2
    for h in hooks:
        h.remove()
    _, torch32 = st._step(b, False)
    rb = m.last_rulebook
    masks = None
    if family == "multi_proj":
        with torch.no_grad():
            masks = [(y > 0).double().cpu() for y in st._chain(b, rb, b.x.flatten(0, 1))]
    truth = tr.sparse_block_gradients(b.x, b.residual, st._leaves(b), rb.indices, BS, m._spatial, BLOCK_K, masks)
    cpu = lambda g: {k: v.cpu() for k, v in g.items()}
    native, torch32 = cpu(native), cpu(torch32)
    assert set(native) == set(truth) and out.shape == (BS, G, 128)
    rows = [k for k in ("x", "residual") if k in truth]
    judge_leaves(native, truth, torch32, lambda k: re.sub(r"\d", "", k), f"sparse block {family}", per_row=rows,
                 row_yardstick={k: max_error(torch32[k], truth[k]) for k in rows})


# ---- 5. the encoder ------------------------------------------------------------------------------------------------------------

def _encoder_step(enc, s, seed=9):
    """``(predictions, input gradient)`` of one training frame at ``seed``."""
    from test_encoder_gpu import run
    feats = s["feats"].clone().requires_grad_()
    torch.manual_seed(seed)
    preds, anchor = run(enc, s, feats)
    sum(t.square().mean() for t in preds).backward()
    enc.zero_grad(set_to_none=True)
    return [t.detach() for t in preds] + [anchor.detach()], feats.grad.detach()


@pytest.mark.parametrize("style", ["prob", "solid"])
def test_encoder_folds_while_training(style, monkeypatch):
    """Train mode with ``set_native(training=True, fold_training=True)``: every absorbed "add" / "norm" is inside its step's
    launch.  At the same seed the outputs and the input gradient lie within ``2 Y_enc + 4 eps32 max|.|`` of the all-torch
    encoder (``set_native(training=False)``), Y_enc the distance of the UNFOLDED ``set_native(training=True)`` encoder from that
    same run -- two routes that exist without the fold.  (The torch feed-forward block draws float masks and the native one
    uint8 masks, so with ``ffn_drop = 0.1`` Y_enc is the distance between two dropout draws.)  The fold itself draws what the
    unfolded native route draws, in its order: against THAT route it may differ by rounding only.  A mask drawn out of order
    would move the outputs by about ``ffn_drop`` of their size, the tails' rounding (a few float32 ulp per LayerNorm, through
    two decoder blocks) by orders of magnitude less; ``1e-3 max|.|`` lies between the two."""
    from test_encoder_gpu import encoder, loop_by_hand, scene
    enc, s = encoder(style), scene()
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    names = lambda: [c[0] for c in calls]
    norms = [m for m, op in zip(enc.layers, enc.operation_order) if op == "norm"]
    absorbed = [enc.layers[st.norm] for st in enc.steps if st.norm is not None]
    ran = []
    hooks = [m.register_forward_hook(lambda mod, *a: ran.append(mod)) for m in norms]
    enc.train()
    try:
        enc.set_native(training=False, fold_training=False)
        torch_out, torch_grad = _encoder_step(enc, s)
        enc.set_native(training=True)
        del calls[:], ran[:]
        unfolded_out, unfolded_grad = _encoder_step(enc, s)
        unfolded_names = names()
        assert len(ran) == len(norms)                                 # fold_training = False: every "norm" is the layer it is ...
        del calls[:]
        torch.manual_seed(9)
        loop_by_hand(enc, s, s["feats"].clone().requires_grad_())
        # ... and the launches are the op-by-op loop's, exactly (which formats the maps in every block, not once)
        forward_only = [n for n in names() if n != "gf_feature_maps_format"]
        assert [n for n in unfolded_names if n != "gf_feature_maps_format"][:len(forward_only)] == forward_only
        enc.set_native(fold_training=True)
        del calls[:], ran[:]
        folded_out, folded_grad = _encoder_step(enc, s)
        assert not any(m in absorbed for m in ran) and len(ran) == len(norms) - len(absorbed)
        ffn = [a for name, a in calls if name == "gf_ffn_forward_train"]
        assert len(ffn) == sum(st.op == "ffn" for st in enc.steps)
        assert all((a[7] is not None) == st.add for a, st in zip(ffn, [st for st in enc.steps if st.op == "ffn"]))
        assert names().count("gf_deform_output_forward_train") == sum(st.op in ("deformable", "spconv") for st in enc.steps)
        assert names().count("gf_deform_output_backward") == names().count("gf_deform_output_forward_train")
    finally:
        enc.set_native(training=False, fold_training=False)
        enc.eval()
        enc.zero_grad(set_to_none=True)
        for h in hooks:
            h.remove()
    for what, got, want, yard in [(f"prediction {i}", g, w, y) for i, (g, w, y) in enumerate(zip(folded_out, torch_out, unfolded_out))] + \
                                 [("input gradient", folded_grad, torch_grad, unfolded_grad)]:
        held(f"encoder {style} {what}", got, want, bound(max_error(yard, want), want))
        err, scale = max_error(got, yard), yard.abs().max().item()
        print(f"encoder {style} {what}: max|folded - unfolded native| = {err:.3e} = {err / scale:.3e} max|.|")
        if what != "input gradient":       # (a forward is continuous in its roundings; a gradient is not, at a ReLU's kink)
            assert err <= 1e-3 * scale, what
