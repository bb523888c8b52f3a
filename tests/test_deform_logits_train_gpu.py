"""The training step of the deformable block's dense front on the GPU: ``gf_deform_logits_forward`` /
``gf_deform_logits_backward`` under ``deformable_logits_autograd``, the deformable block's ``native_front_training`` and the
encoder's ``front_training`` above them.

Values.  The truth is float64 autograd of ``sum(raw * w) + sum(learned * w)`` through the restatement
(tests/deform_logits_train_ref.py).  The op is linear: no row is exempt.  Per tensor ``max|native - truth| <= 2 Y + 4 eps32
max|truth|`` (tests/row_judge.py): for ``out`` (``[raw | learned]``) and the two per-row gradients Y is ``max|float32 torch
composition on this GPU - truth|`` over the variant's 1 000 rows (every smaller n is a prefix of them, the larger ones start
with them); for a parameter, relative to the leaf's ``max|truth|``, the largest relative error of the float32 composition over
the leaves of its kind (weight, bias) at the same n.  The variant's first four rows of ``instance_feature`` are planted (zeros,
1e-30, +-1e4); the per-row tensors are judged a second time without them.  The measured ratios are printed (-s) and recorded in
DESIGN.md §3.13g.

Invariants are bitwise.  Nothing here reads past a buffer's end or inspects code."""
import functools

import pytest
import torch
import torch.nn as nn

import deform_block_ref as ref
import deform_logits_train_ref as tr
import row_ref
from gaussianformer_amd import _lib
from gaussianformer_amd.deformable_block import deformable_logits, deformable_logits_autograd, logits_train_sizes
from row_judge import Guarded, bound, edge_rows, held, judge_leaves, max_error, ptr_table, spy  # noqa: F401  (spy is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B = _lib.GF_DEFORM_LOGITS_WGRAD_ROWS
N_VARIANT, PLANTED = 1000, 4
ROWS = tuple(sorted(set(edge_rows(B)) | {N_VARIANT}))
N_ALL = max(max(ROWS), 2 * B + 77)
PER_ROW = tr.PER_ROW
NAN = float("nan")


class Case:
    """A width's weights and its rows on the GPU (the first 1 000 are the family), and per n the three sets of results."""

    def __init__(self, name, seed=0):
        self.name = name
        self.k3, self.nw, with_e = tr.FRONT[name]
        sd = tr.weights(self.k3, self.nw, seed)
        self.sd, self.sd64 = tr.cast(sd, device=DEV), tr.cast(sd, torch.float64, DEV)
        self.f = tr.planted(tr.fixed_input(N_ALL, 128, 61 + seed)).to(DEV)
        self.e = tr.fixed_input(N_ALL, 128, 71 + seed).to(DEV) if with_e else None

    def inputs(self, n, rows=None):
        pick = (lambda t: t[:n].contiguous()) if rows is None else (lambda t: t[rows].contiguous())
        return tuple(None if t is None else pick(t) for t in (self.f, self.e))

    def native(self, f, e, sd):
        raw, learned = deformable_logits_autograd(f, e, *tr.pairs(sd))
        return raw if learned is None else torch.cat([raw, learned.flatten(-2)], dim=-1)

    def plain(self, f, e):
        with torch.no_grad():
            raw, learned = deformable_logits(f, e, *tr.pairs(self.sd))
        return raw, None if learned is None else learned.flatten(-2)

    @functools.lru_cache(maxsize=None)
    def grads(self, n):
        f, e = self.inputs(n)
        d = lambda t: None if t is None else t.double()
        return (tr.gradients(tr.logits_train_ref, d(f), d(e), self.sd64), tr.gradients(tr.logits_train_ref, f, e, self.sd),
                tr.gradients(self.native, f, e, self.sd))

    def cotangents(self, n):
        cot = tr.cotangent(n, self.k3, self.nw, torch.float32).to(DEV)
        return cot[:, :self.nw].contiguous(), cot[:, self.nw:].contiguous() if self.k3 else None

    def step(self, f, e, go_raw, go_learned):
        """The native results for explicit cotangents (``None``: that output is not used): ``{"raw", "learned", per-row
        gradients, parameter gradients}``."""
        ins = {"instance_feature": f, "anchor_embed": e}
        ins = {k: v.detach().clone().requires_grad_(True) for k, v in ins.items() if v is not None}
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in self.sd.items()}
        raw, learned = deformable_logits_autograd(ins["instance_feature"], ins.get("anchor_embed"), *tr.pairs(leaves))
        outs = [(raw, go_raw)] + ([] if learned is None else [(learned.flatten(-2), go_learned)])
        outs = [(o, g) for o, g in outs if g is not None]
        wanted = {**ins, **leaves}
        got = dict(zip(wanted, torch.autograd.grad([o for o, _ in outs], list(wanted.values()), grad_outputs=[g for _, g in outs],
                                                   allow_unused=True)))
        return {"raw": raw.detach(), "learned": None if learned is None else learned.detach().flatten(-2), **got}


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


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

@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", list(tr.FRONT))
def test_values(name, n):
    judged(case(name), n)


# ---- 2. bitwise --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(tr.FRONT))
def test_outputs_are_the_plain_forward_s(name):
    c = case(name)
    for n in ROWS:
        f, e = c.inputs(n)
        raw, learned = deformable_logits_autograd(f.clone().requires_grad_(True), e, *tr.pairs(c.sd))
        want_raw, want_learned = c.plain(f, e)
        assert raw.requires_grad and torch.equal(raw.detach(), want_raw), n
        assert (learned is None) == (c.k3 == 0)
        if c.k3:
            assert learned.requires_grad and learned.shape == (n, c.k3 // 3, 3) and torch.equal(learned.detach().flatten(-2), want_learned), n


@pytest.mark.parametrize("name", list(tr.FRONT))
def test_two_calls_agree(name):
    c = case(name)
    n = 2 * B + 77      # three weight-gradient blocks, the last ragged
    f, e = c.inputs(n)
    a, b = c.step(f, e, *c.cotangents(n)), c.step(f, e, *c.cotangents(n))
    assert sorted(a) == sorted(b) and all(a[k] is None and b[k] is None or torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", list(tr.FRONT))
def test_a_row_alone_is_the_row_among_others(name):
    """n = 1 against the same row at rows 0, 127, 128, 999 of 1 000."""
    c = case(name)
    gr, gl = c.cotangents(N_VARIANT)
    full = c.step(*c.inputs(N_VARIANT), gr, gl)
    for r in (0, 127, 128, 999):
        one = c.step(*c.inputs(1, rows=slice(r, r + 1)), gr[r:r + 1].contiguous(), None if gl is None else gl[r:r + 1].contiguous())
        for k in ("instance_feature", "anchor_embed"):
            if k in full:
                assert torch.equal(one[k], full[k][r:r + 1]), (k, r)


def _raw_backward(c, n, gr, gl, gf=True, ge=True, slots=(True,) * 4, tail=4096, fill=12345.0, garbage=NAN):
    """``gf_deform_logits_backward`` on caller-made buffers with ``tail`` sentinel elements behind every output and the
    workspace, the outputs prefilled with ``garbage``: the results and whether every sentinel survived."""
    f, e = c.inputs(n)
    params = [c.sd.get(k) for k in tr.KEYS]
    grads = [None if p is None or not want else Guarded(4 * p.numel(), DEV, 4 * tail, fill, body=garbage) for p, want in zip(params, slots)]
    _, work_bytes = logits_train_sizes(n, c.k3, c.nw)
    out_f, out_e = [Guarded(4 * n * 128, DEV, 4 * tail, fill, body=garbage) if want else None for want in (gf, ge and e is not None)]
    work = Guarded(work_bytes, DEV, tail, 0x5A, body=0x5A)
    _lib.call("gf_deform_logits_backward", DEV, n, 128, c.k3, c.nw, f, e, ptr_table(params), gl, gr, None if out_f is None else out_f.buf,
              None if out_e is None else out_e.buf, ptr_table([None if g is None else g.buf for g in grads]), work.buf, work_bytes)
    regions = [g for g in [out_f, out_e, work] + grads if g is not None]
    results = {"instance_feature": None if out_f is None else out_f.floats(n, 128), "anchor_embed": None if out_e is None else out_e.floats(n, 128)}
    results.update({k: g.floats(*p.shape) for k, g, p in zip(tr.KEYS, grads, params) if g is not None})
    return results, all(g.intact() for g in regions)


def _raw_forward(c, n, tail=4096, fill=12345.0):
    f, e = c.inputs(n)
    raw = Guarded(4 * n * c.nw, DEV, 4 * tail, fill, body=NAN)
    learned = Guarded(4 * n * c.k3, DEV, 4 * tail, fill, body=NAN) if c.k3 else None
    _lib.call("gf_deform_logits_forward", DEV, n, 128, c.k3, c.nw, f, e, ptr_table([c.sd.get(k) for k in tr.KEYS]),
              None if learned is None else learned.buf, raw.buf)
    return raw.floats(n, c.nw), None if learned is None else learned.floats(n, c.k3), raw.intact() and (learned is None or learned.intact())


@pytest.mark.parametrize("n", [1, 33, 129, B + 1])
@pytest.mark.parametrize("name", list(tr.FRONT))
def test_nothing_is_written_beyond_an_end_and_garbage_is_overwritten(name, n):
    """Sentinels behind every output and the workspace survive; every gradient, its buffer prefilled with NaN, is the
    function's bit for bit: stored in full, not accumulated."""
    c = case(name)
    gr, gl = c.cotangents(n)
    raw, learned, intact = _raw_forward(c, n)
    assert intact
    got, intact = _raw_backward(c, n, gr, gl)
    assert intact
    native = c.step(*c.inputs(n), gr, gl)
    assert torch.equal(raw, native["raw"]) and (learned is None or torch.equal(learned, native["learned"]))
    for k in ("instance_feature", "anchor_embed") + tr.KEYS:
        if k in native:
            assert torch.equal(got[k], native[k]) and bool(torch.isfinite(got[k]).all()), k
    assert set(native) - {"raw", "learned", "instance_feature", "anchor_embed"} == set(c.sd)


@pytest.mark.parametrize("name", ["solid", "nocam_solid", "nocam_base", "edge"])
def test_null_cotangents_and_null_slots(name):
    c = case(name)
    n = 300
    gr, gl = c.cotangents(n)
    both, _ = _raw_backward(c, n, gr, gl)
    # without a learned term grad_feature is grad_embed, bit for bit
    no_l, intact = _raw_backward(c, n, gr, None)
    assert intact and torch.equal(no_l["instance_feature"], no_l["anchor_embed"]) and torch.equal(no_l["anchor_embed"], both["anchor_embed"])
    assert torch.equal(no_l[tr.WW], both[tr.WW]) and torch.equal(no_l[tr.BW], both[tr.BW])
    if c.k3 == 0:
        assert torch.equal(both["instance_feature"], both["anchor_embed"])
    else:
        assert not torch.equal(both["instance_feature"], both["anchor_embed"])
        assert bool((no_l[tr.WL] == 0).all()) and bool((no_l[tr.BL] == 0).all())      # a zero cotangent: zeros are stored
    # a NULL grad_raw: dWw and dbw are zeros, grad_embed too, grad_feature is the learned term alone
    no_r, intact = _raw_backward(c, n, None, gl)
    assert intact and bool((no_r[tr.WW] == 0).all()) and bool((no_r[tr.BW] == 0).all()) and bool((no_r["anchor_embed"] == 0).all())
    if c.k3:
        assert torch.equal(no_r[tr.WL], both[tr.WL]) and torch.equal(no_r[tr.BL], both[tr.BL])
        want = (gl.double() @ c.sd64[tr.WL])
        held(f"{name} grad_feature of the learned term alone", no_r["instance_feature"], want, bound(max_error((gl @ c.sd[tr.WL]), want), want))
    else:
        assert bool((no_r["instance_feature"] == 0).all())
    # NULL output slots are skipped, the others keep their bits
    for gf, ge, slots in ((True, False, (False, True, True, False)), (False, True, (True, False, False, True)), (False, False, (True,) * 4),
                          (True, True, (False,) * 4)):
        got, intact = _raw_backward(c, n, gr, gl, gf, ge, slots)
        assert intact
        for k, v in got.items():
            if v is not None:
                assert torch.equal(v, both[k]), (k, gf, ge, slots)


def test_no_rows_zero_fill_the_parameter_gradients():
    for name in ("base", "nocam_solid"):
        c = case(name)
        params = [c.sd.get(k) for k in tr.KEYS]
        grads = [None if p is None else torch.full_like(p, NAN) for p in params]
        assert logits_train_sizes(0, c.k3, c.nw) == (0, 0)
        _lib.call("gf_deform_logits_backward", DEV, 0, 128, c.k3, c.nw, None, None, ptr_table(params), None, None, None, None, ptr_table(grads), None, 0)
        assert all(g is None or bool((g == 0).all()) for g in grads)
        f = torch.empty(0, 128, device=DEV, requires_grad=True)
        raw, learned = deformable_logits_autograd(f, None if c.e is None else c.e[:0], *tr.pairs({k: v.clone().requires_grad_(True) for k, v in c.sd.items()}))
        assert raw.shape == (0, c.nw) and (learned is None or learned.shape == (0, c.k3 // 3, 3))


@pytest.mark.parametrize("name", ["base", "nocam_base", "narrow"])
def test_a_nan_stays_in_its_row(name):
    """A NaN in one row of grad_raw, of grad_learned or of instance_feature: every other row of the data gradients stays bit for
    bit; the parameter gradients are NaN where the float32 torch composition's are."""
    c = case(name)
    n, bad = 300, 77
    f, e = c.inputs(n)
    gr, gl = c.cotangents(n)
    clean = c.step(f, e, gr, gl)
    keep = torch.arange(n, device=DEV) != bad
    rows = [k for k in ("instance_feature", "anchor_embed") if k in clean]
    g2 = gr.clone()
    g2[bad, c.nw - 1] = NAN
    got = c.step(f, e, g2, gl)
    for k in rows:
        assert torch.equal(got[k][keep], clean[k][keep]) and bool(torch.isnan(got[k][bad]).all()), k
    assert torch.equal(got[tr.WL], clean[tr.WL]) and torch.equal(got[tr.BL], clean[tr.BL])
    assert bool(torch.isnan(got[tr.WW][c.nw - 1]).all()) and not bool(torch.isnan(got[tr.WW][:c.nw - 1]).any())
    assert bool(torch.isnan(got[tr.BW][c.nw - 1])) and int(torch.isnan(got[tr.BW]).sum()) == 1
    l2 = gl.clone()
    l2[bad, 1] = NAN
    got = c.step(f, e, gr, l2)
    assert torch.equal(got["instance_feature"][keep], clean["instance_feature"][keep]) and bool(torch.isnan(got["instance_feature"][bad]).all())
    if "anchor_embed" in clean:
        assert torch.equal(got["anchor_embed"], clean["anchor_embed"])          # the learned columns are not part of it
    assert torch.equal(got[tr.WW], clean[tr.WW]) and bool(torch.isnan(got[tr.WL][1]).all()) and int(torch.isnan(got[tr.BL]).sum()) == 1
    # in instance_feature: the forward's row; linear, so the data gradients do not read it
    f2 = f.clone()
    f2[bad, 100] = NAN
    got = c.step(f2, e, gr, gl)
    assert torch.equal(got["raw"][keep], clean["raw"][keep]) and bool(torch.isnan(got["raw"][bad]).all())
    assert all(torch.equal(got[k], clean[k]) for k in rows)
    t32 = tr.gradients(tr.logits_train_ref, f2, e, c.sd)
    for k in c.sd:
        assert torch.equal(torch.isnan(got[k]), torch.isnan(t32[k])), k


def test_graph_replay_equals_eager():
    c = case("base")
    n = 777
    f, e = c.inputs(n)
    gr, gl = c.cotangents(n)
    eager = c.step(f, e, gr, gl)
    fl, el = f.clone().requires_grad_(True), e.clone().requires_grad_(True)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in c.sd.items()}
    keys = list(leaves)

    def step():
        raw, learned = deformable_logits_autograd(fl, el, *tr.pairs(leaves))
        return raw, learned, torch.autograd.grad([raw, learned.flatten(-2)], [fl, el] + [leaves[k] for k in keys], grad_outputs=[gr, gl])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw, learned, got = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(raw.detach(), eager["raw"]) and torch.equal(learned.detach().flatten(-2), eager["learned"])
    assert torch.equal(got[0], eager["instance_feature"]) and torch.equal(got[1], eager["anchor_embed"])
    for k, g in zip(keys, got[2:]):
        assert torch.equal(g, eager[k]), k


def test_entry_point_refuses_on_the_device_too():
    c = case("solid")
    n = 64
    f, e = c.inputs(n)
    gr, gl = c.cotangents(n)
    params = [c.sd.get(k) for k in tr.KEYS]
    grads = [torch.empty_like(p) for p in params]
    _, work_bytes = logits_train_sizes(n, c.k3, c.nw)
    work = torch.empty(work_bytes, dtype=torch.uint8, device=DEV)
    fail = r"failed \(code -1\): .*"
    new = lambda: torch.empty(n, 128, device=DEV)
    with pytest.raises(RuntimeError, match=fail + "grad_feature aliases an input"):
        _lib.call("gf_deform_logits_backward", DEV, n, 128, c.k3, c.nw, f, e, ptr_table(params), gl, gr, e, None, ptr_table(grads), work, work_bytes)
    with pytest.raises(RuntimeError, match=fail + "grad_embed aliases the workspace"):
        _lib.call("gf_deform_logits_backward", DEV, n, 128, c.k3, c.nw, f, e, ptr_table(params), gl, gr, new(), work, ptr_table(grads), work, work_bytes)
    with pytest.raises(RuntimeError, match=r"failed \(code -2\): .*workspace of"):
        _lib.call("gf_deform_logits_backward", DEV, n, 128, c.k3, c.nw, f, e, ptr_table(params), gl, gr, new(), new(), ptr_table(grads), work, work_bytes - 1)


# ---- 3. the deformable block ---------------------------------------------------------------------------------------------------

def _module_step(m, s, post, norm_pair, front, back=False, train=False, seed=None):
    """``(out, {leaf name: gradient}, the submodules that ran)`` of the fixed scalar through the module: the inputs, the maps
    and every parameter."""
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
    watched = [mod for mod in m.modules() if mod is not m] + ([norm] if post else [])
    hooks = [mod.register_forward_hook(lambda mod, *a: ran.append(mod)) for mod in watched]
    m.native_front_training, m.native_training = front, back
    m.train(train)
    try:
        if seed is not None:
            torch.manual_seed(seed)
        metas = dict(projection_mat=s["pm"], image_wh=s["wh"])
        kw = dict(residual=leaves["inst"], norm=norm) if post else {}
        out = m(leaves["inst"], leaves["anchor"], leaves["emb"], [leaves[f"map{i}"] for i in range(len(s["maps"]))], metas, **kw)
        wanted = {**leaves, **params}
        grads = dict(zip(wanted, torch.autograd.grad((out * tr.output_weights(out.shape, torch.float32).to(DEV)).sum(), list(wanted.values()))))
    finally:
        del m.native_front_training, m.native_training
        m.eval()
        for h in hooks:
            h.remove()
    return out.detach(), grads, ran


def _module_truth(s, cfg, sd, post, weight_mask=None):
    d = lambda t: t.detach().double()
    sd64 = tr.cast(sd, torch.float64, DEV)
    inputs = {"inst": d(s["inst"]), "anchor": d(s["anchor"]), "emb": d(s["emb"]), **{f"map{i}": d(f) for i, f in enumerate(s["maps"])}}
    import daf_fused_ref

    def restated(inst, anchor, emb, *rest):
        maps, leaves = list(rest[:-1]), rest[-1]
        middle = None
        if weight_mask is not None:
            middle = lambda kp, raw: daf_fused_ref.block(kp, d(s["pm"]), d(s["wh"]), maps, raw, weight_mask=weight_mask)
        return ref.module_ref(leaves, cfg, inst, anchor, emb, maps, d(s["pm"]), d(s["wh"]), residual=inst if post else None, middle=middle)
    return row_ref.scalar_gradients(restated, inputs, sd64, with_out=True)


@pytest.mark.parametrize("name", ["solid", "prob"])
def test_deformable_block_trains_its_front_end_natively(name, spy):
    """A = 300 on the synthetic pyramid, solid and prob: the launches, no call of ``weights_fc``, ``learnable_fc`` or the
    generator as modules, and the output and every gradient held to the float64 module restatement with the same module's
    switch-off route as the yardstick -- with the front's switch alone and with the back end's beside it."""
    from test_deform_block_gpu import SHAPES, module_of, scene
    m, cfg, sd = module_of(name)
    s = scene()
    post = SHAPES[name]["post"]
    pair = (sd["norm.weight"].to(DEV), sd["norm.bias"].to(DEV)) if post else None
    front_mods = {m.weights_fc, m.kps_generator, m.kps_generator.learnable_fc}
    del spy[:]
    out, native, ran = _module_step(m, s, post, pair, True)
    assert not front_mods & set(ran) and m.output_proj in ran
    assert spy.count("gf_deform_logits_forward") == 1 and spy.count("gf_deform_logits_backward") == 1
    assert spy.index("gf_deform_logits_forward") < spy.index("gf_deform_logits_backward")
    assert spy.index("gf_daf_fused_backward") < spy.index("gf_deform_logits_backward")        # the front's backward comes last
    with_front = [n for n in spy if not n.startswith("gf_deform_logits")]
    del spy[:]
    out32, torch32, ran32 = _module_step(m, s, post, pair, False)
    assert front_mods <= set(ran32) and spy == with_front          # with the attribute False: the torch route's launches, in its order
    assert m.native_front_training is False and m.native_training is False
    del spy[:]
    out_both, both, ran_both = _module_step(m, s, post, pair, True, back=True)
    assert ran_both and set(ran_both) <= set(m.camera_encoder.modules())                       # only the camera encoder is left on torch
    assert spy.count("gf_deform_logits_backward") == 1 and spy.count("gf_deform_output_backward") == 1

    truth = _module_truth(s, cfg, sd, post)
    for what, o, g in (("front", out, native), ("front + back", out_both, both)):
        held(f"module {name} {what} out", o, truth["out"], bound(max_error(out32, truth["out"]), truth["out"]))
        assert set(g) == set(truth) - {"out"}
        for k in g:
            held(f"module {name} {what} d/d {k}", g[k], truth[k], bound(max_error(torch32[k], truth[k]), truth[k]))


def test_attention_dropout_draws_the_same_mask():
    """``attn_drop = 0.1`` in train mode: the front's switch draws nothing and moves no draw, so at the same generator state
    the output is the switch-off route's up to the two routes' rounding -- both held to the float64 restatement with THAT
    mask."""
    from test_deform_block_gpu import module_of, scene
    m, cfg, sd = module_of("solid")
    s = scene()
    m.attn_drop = 0.1
    out, _, _ = _module_step(m, s, False, None, True, train=True, seed=5)
    out32, _, _ = _module_step(m, s, False, None, False, train=True, seed=5)
    torch.manual_seed(5)
    mask = torch.rand(1, 300, 6, 4, m.num_pts, 4, device=DEV) > 0.1
    assert not bool(mask.all())
    truth = _module_truth(s, cfg, sd, False, weight_mask=mask)["out"]
    held("module solid attn_drop out", out, truth, bound(max_error(out32, truth), truth))
    err = max_error(out, out32)
    print(f"attn_drop: max|front - switch-off| = {err:.3e}")
    assert err <= 1e-3 * out32.abs().max().item()                  # (another mask moves a tenth of the weights)


# ---- 4. the encoder ------------------------------------------------------------------------------------------------------------

def test_encoder_trains_the_front_natively(monkeypatch):
    """``encoder("prob")`` in train mode with every native training switch: one ``gf_deform_logits_backward`` per deformable step,
    and predictions within ``1e-3 max|.|`` of the same encoder without ``front_training`` at the same seed (the margin
    tests/test_deform_output_train_gpu.py uses to tell rounding from a mask drawn out of order)."""
    from test_encoder_gpu import encoder, run, scene
    enc, s = encoder("prob"), scene()
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])

    def step():
        feats = s["feats"].clone().requires_grad_()
        torch.manual_seed(9)
        preds, anchor = run(enc, s, feats)
        sum(t.square().mean() for t in preds).backward()
        enc.zero_grad(set_to_none=True)
        return [t.detach() for t in preds] + [anchor.detach()], feats.grad.detach()
    enc.train()
    try:
        enc.set_native(training=True, fold_training=True, front_training=False)
        want, want_grad = step()
        assert "gf_deform_logits_backward" not in names
        del names[:]
        enc.set_native(front_training=True)
        got, got_grad = step()
        steps = sum(op == "deformable" for op in enc.operation_order)
        assert steps > 0 and names.count("gf_deform_logits_backward") == steps and names.count("gf_deform_logits_forward") == steps
    finally:
        enc.set_native(training=False, fold_training=False, front_training=False)
        enc.eval()
        enc.zero_grad(set_to_none=True)
    for i, (g, w) in enumerate(zip(got, want)):
        err, scale = max_error(g, w), w.abs().max().item()
        print(f"encoder prob prediction {i}: max|front - without| = {err:.3e} = {err / scale:.3e} max|.|")
        assert bool(torch.isfinite(g).all()) and err <= 1e-3 * scale, i
    assert bool(torch.isfinite(got_grad).all()) and got_grad.shape == want_grad.shape
