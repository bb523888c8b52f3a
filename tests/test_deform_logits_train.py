"""The training step of the deformable block's dense front without a GPU (``gf_deform_logits_train_sizes``,
``gf_deform_logits_backward``, ``deformable_logits_autograd``, the module's ``native_front_training`` and the encoder's
``front_training``): the restatement against torch's float64 autograd, every refusal of the two entries on
host buffers (they come before any HIP call), the sizes query, and the routing conditions with the library call stubbed."""
import ctypes
import inspect
import json

import pytest
import torch
import torch.nn as nn

import deform_logits_train_ref as tr
import gaussianformer_amd
from gaussianformer_amd import GaussianOccEncoder, _lib
from gaussianformer_amd import deformable_block as db
from gaussianformer_amd.deformable_block import (DeformableFeatureAggregation, DeformLogitsFunction, deformable_logits,
                                                 deformable_logits_autograd, logits_train_sizes)
from row_judge import ptr_table
from test_encoder import GOLDEN, _encoder

CPU = torch.device("cpu")
B = _lib.GF_DEFORM_LOGITS_WGRAD_ROWS


# ---- the restatement -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(tr.FRONT))
def test_restatement_is_torch_s_float64_autograd(name):
    """``logits_train_ref`` and ``gradients`` against two nn.Linear and the add under autograd."""
    k3, nw, with_e = tr.FRONT[name]
    n = 37
    sd = tr.weights(k3, nw, dtype=torch.float64)
    f = tr.planted(tr.fixed_input(n, 128, 1)).double()
    e = tr.fixed_input(n, 128, 2).double() if with_e else None
    got = tr.gradients(tr.logits_train_ref, f, e, sd)

    wfc = nn.Linear(128, nw).double()
    lfc = nn.Linear(128, k3).double() if k3 else None
    with torch.no_grad():
        wfc.weight.copy_(sd[tr.WW])
        wfc.bias.copy_(sd[tr.BW])
        if k3:
            lfc.weight.copy_(sd[tr.WL])
            lfc.bias.copy_(sd[tr.BL])
    fl = f.clone().requires_grad_(True)
    el = None if e is None else e.clone().requires_grad_(True)
    raw = wfc(fl if el is None else fl + el)
    scalar = (raw * tr.output_weights(raw.shape)).sum()
    want_out = raw
    if k3:
        learned = lfc(fl)
        scalar = scalar + (learned * tr.output_weights(learned.shape)).sum()
        want_out = torch.cat([raw, learned], dim=-1)
    scalar.backward()
    want = {"out": want_out.detach(), "instance_feature": fl.grad, tr.WW: wfc.weight.grad, tr.BW: wfc.bias.grad}
    if el is not None:
        want["anchor_embed"] = el.grad
    if k3:
        want.update({tr.WL: lfc.weight.grad, tr.BL: lfc.bias.grad})
    assert set(got) == set(want)
    for k in want:
        scale = max(want[k].abs().max().item(), 1e-30)
        assert got[k].shape == want[k].shape and (got[k] - want[k]).abs().max().item() <= 1e-12 * scale, k
    assert {tr.kind(tr.WW), tr.kind(tr.WL)} == {"weight"} and {tr.kind(tr.BW), tr.kind(tr.BL)} == {"bias"}


# ---- the entries on host buffers -----------------------------------------------------------------------------------------------

def _bufs(count, floats=1 << 15):
    """``count`` disjoint 16-byte aligned host tensors."""
    bufs = [torch.zeros(floats) for _ in range(count)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    return bufs


class Host:
    """One call's host buffers: every tensor its own allocation, so that only the aliasing a case asks for is there."""

    def __init__(self):
        (self.f, self.e, self.gl, self.gr, self.gf, self.ge, self.work) = _bufs(7)
        self.params, self.grads = _bufs(4, 1 << 15), _bufs(4, 1 << 15)

    def table(self, tensors, drop=(), misalign=None, off=4):
        entries = [None if i in drop else t.data_ptr() + (off if i == misalign else 0) for i, t in enumerate(tensors)]
        return ptr_table(entries)


def _at(t, off):
    return None if t is None else t.data_ptr() + off


def _bwd(n=4, width=128, k3=6, nw=144, drop=None, misalign=None, gdrop=None, gmisalign=None, goff=4, null_params=False, null_grads=False,
         work_bytes=None, offs=None, **over):
    h = Host()
    t = dict(f=h.f, e=h.e, gl=h.gl if k3 else None, gr=h.gr, gf=h.gf, ge=h.ge, work=h.work)
    t.update(over)
    offs = offs or {}
    drop = ((0, 1) if k3 == 0 else ()) if drop is None else drop
    gdrop = drop if gdrop is None else gdrop
    need = logits_train_sizes(max(n, 0), k3, nw)[1] if 0 <= k3 <= 32 and nw >= 4 and nw % 4 == 0 and width == 128 else 1 << 16
    at = lambda k: _at(t[k], offs.get(k, 0))
    _lib.call("gf_deform_logits_backward", CPU, n, width, k3, nw, at("f"), at("e"), None if null_params else h.table(h.params, drop, misalign),
              at("gl"), at("gr"), at("gf"), at("ge"), None if null_grads else h.table(h.grads, gdrop, gmisalign, goff), at("work"),
              need if work_bytes is None else work_bytes)
    return h


FAIL = r"gf_deform_logits_backward failed \(code -1\): gf_deform_logits_backward: "


def test_what_the_forward_refuses():
    for kw, msg in ((dict(width=32), r"E = 32: only embed_dims = 128"), (dict(k3=33), r"K3 = 33: the learned columns 3 K must be 0 \.\. 32"),
                    (dict(k3=-3), r"K3 = -3"), (dict(nw=0), r"Nw = 0: the logits' width must be a positive multiple of 4"),
                    (dict(nw=146), r"Nw = 146"), (dict(n=-2), r"n = -2 is negative"), (dict(null_params=True), r"null params"),
                    (dict(drop=(0,), gdrop=()), r"kps_generator.learnable_fc.weight is missing"),
                    (dict(drop=(1,), gdrop=()), r"kps_generator.learnable_fc.bias is missing"),
                    (dict(drop=(2,), gdrop=()), r"weights_fc.weight is missing"), (dict(k3=0, drop=(0, 1, 3)), r"weights_fc.bias is missing"),
                    (dict(misalign=0), r"kps_generator.learnable_fc.weight is not 16-byte aligned"),
                    (dict(misalign=3), r"weights_fc.bias is not 16-byte aligned"),
                    (dict(offs=dict(f=4)), r"instance_feature is not 16-byte aligned"), (dict(offs=dict(e=8)), r"anchor_embed is not 16-byte aligned")):
        with pytest.raises(RuntimeError, match=FAIL + msg):
            _bwd(**kw)


def test_backward_refusals():
    for kw, msg in ((dict(k3=0, gl=Host().gl), r"grad_learned with K3 = 0"),
                    (dict(null_grads=True), r"null grad_params"),
                    (dict(k3=0, gdrop=(1,)), r"a gradient for kps_generator.learnable_fc.weight, which is absent"),
                    (dict(k3=0, gdrop=(0,)), r"a gradient for kps_generator.learnable_fc.bias, which is absent"),
                    (dict(gmisalign=2), r"the gradient of weights_fc.weight is not 16-byte aligned"),
                    (dict(gmisalign=3, goff=8), r"the gradient of weights_fc.bias is not 16-byte aligned"),
                    (dict(gmisalign=0, goff=2), r"the gradient of kps_generator.learnable_fc.weight is not 4-byte aligned"),
                    (dict(gmisalign=1, goff=1), r"the gradient of kps_generator.learnable_fc.bias is not 4-byte aligned"),
                    (dict(offs=dict(gl=2)), r"grad_learned is not 4-byte aligned"), (dict(offs=dict(gr=4)), r"grad_raw is not 16-byte aligned"),
                    (dict(offs=dict(gf=4)), r"grad_feature is not 16-byte aligned"), (dict(offs=dict(ge=12)), r"grad_embed is not 16-byte aligned"),
                    (dict(offs=dict(work=4)), r"workspace is not 16-byte aligned"), (dict(work=None), r"workspace is null"),
                    (dict(f=None), r"null pointer: instance_feature")):
        with pytest.raises(RuntimeError, match=FAIL + msg):
            _bwd(**kw)
    # grad_learned and learnable_fc's gradients are rows of K3 floats: 4-byte alignment is enough, and the next refusal follows
    with pytest.raises(RuntimeError, match=FAIL + r"workspace is null"):
        _bwd(offs=dict(gl=4), gmisalign=0, work=None)
    need = logits_train_sizes(4, 6, 144)[1]
    with pytest.raises(RuntimeError, match=rf"backward failed \(code -2\): gf_deform_logits_backward: workspace of {need - 1} bytes, {need} needed"):
        _bwd(work_bytes=need - 1)
    # an output that aliases an input, the workspace or an earlier output
    s = torch.zeros(1 << 15)
    for kw, msg in ((dict(f=s, gf=s[256:]), r"grad_feature aliases an input"), (dict(e=s, ge=s[128:]), r"grad_embed aliases an input"),
                    (dict(gr=s, gf=s[512:]), r"grad_feature aliases an input"), (dict(gl=s, ge=s[20:]), r"grad_embed aliases an input"),
                    (dict(work=s, gf=s[512:]), r"grad_feature aliases the workspace"), (dict(gf=s, ge=s[256:]), r"grad_embed aliases grad_feature")):
        with pytest.raises(RuntimeError, match=FAIL + msg):
            _bwd(**kw)
    h = Host()
    call = lambda grads, params=None: _lib.call("gf_deform_logits_backward", CPU, 4, 128, 6, 144, h.f, h.e, h.table(params or h.params), h.gl, h.gr,
                                                h.gf, h.ge, h.table(grads), h.work, 1 << 17)
    with pytest.raises(RuntimeError, match=FAIL + r"the gradient of kps_generator.learnable_fc.bias aliases an input"):
        call([h.grads[0], h.params[1], h.grads[2], h.grads[3]])
    with pytest.raises(RuntimeError, match=FAIL + r"the gradient of weights_fc.weight aliases an input"):
        call([h.grads[0], h.grads[1], h.params[2][128:], h.grads[3]])
    with pytest.raises(RuntimeError, match=FAIL + r"the gradient of weights_fc.weight aliases the gradient of kps_generator.learnable_fc.weight"):
        call([h.grads[0], h.grads[1], h.grads[0][512:], h.grads[3]])
    with pytest.raises(RuntimeError, match=FAIL + r"the gradient of weights_fc.bias aliases grad_feature"):
        call([h.grads[0], h.grads[1], h.grads[2], h.gf[64:]])
    with pytest.raises(RuntimeError, match=FAIL + r"the gradient of weights_fc.bias aliases the workspace"):
        call([h.grads[0], h.grads[1], h.grads[2], h.work[64:]])
    # a NULL slot is a gradient nobody asked for: with none asked for no workspace is needed, and the refusal that follows is
    # the next one
    with pytest.raises(RuntimeError, match=FAIL + r"grad_embed aliases grad_feature"):
        _bwd(gdrop=(0, 1, 2, 3), work=None, gf=s, ge=s[256:])
    # n == 0 is GF_OK without a workspace: the asked-for parameter gradients are zero-filled by a launch, so on host buffers
    # only the call without a gradient slot runs to its end
    _bwd(n=0, gdrop=(0, 1, 2, 3), work=None, f=None, e=None, gl=None, gr=None, gf=None, ge=None)


def test_train_sizes():
    lib = _lib.load()
    assert B == 512 and B % 128 == 0
    for k3, nw, _ in tr.FRONT.values():
        assert logits_train_sizes(0, k3, nw) == (0, 0)
        last = 0
        for n in sorted({1, 31, 32, 33, 128, 129, 1000, B - 1, B, B + 1, 6400, 25600, 144000}):
            saved, work = logits_train_sizes(n, k3, nw)
            assert saved == 0                                             # linear: nothing is saved
            blocks, tiles, pad = (n + B - 1) // B, (n + 127) // 128, 32 if k3 else 0
            partials = blocks * (nw + pad) * 128 * 4 + tiles * (pad + (nw + 127) // 128 * 128) * 4
            assert partials <= work <= partials + 512, (n, work)
            assert work >= last and work > 0 and work % 16 == 0
            last = work
    for n in (1, 1000, 144000):      # monotone in Nw as well
        last = 0
        for nw in (4, 16, 128, 132, 144, 208, 256, 260, 864, 1248, 4096):
            work = logits_train_sizes(n, 18, nw)[1]
            assert work >= last
            last = work
    assert logits_train_sizes(144000, 6, 144)[1] < 32 << 20 and logits_train_sizes(25600, 18, 1248)[1] < 40 << 20
    out = ctypes.c_size_t(0)
    a = ctypes.addressof(out)
    for args, message in (((-1, 128, 6, 144, a, a), b"n = -1 is negative"), ((4, 256, 6, 144, a, a), b"E = 256"), ((4, 128, 33, 144, a, a), b"K3 = 33"),
                          ((4, 128, 6, 0, a, a), b"Nw = 0"), ((4, 128, 6, 10, a, a), b"Nw = 10"), ((4, 128, 6, 144, None, a), b"null pointer"),
                          ((4, 128, 6, 144, a, None), b"null pointer")):
        assert lib.gf_deform_logits_train_sizes(*args) == -1 and message in lib.gf_last_error()


def test_constants_and_build_list():
    from gaussianformer_amd import build as build_mod
    assert "deform_logits_train.hip" in build_mod.SOURCES and "deform_logits_train.hip" not in build_mod.FP_ATOMICS
    for name in ("gf_deform_logits_train_sizes", "gf_deform_logits_backward"):
        assert name in _lib.SIGNATURES
    assert _lib.GF_ABI_VERSION == 10 and _lib.load().gf_abi_version() == 10
    assert gaussianformer_amd.deformable_logits_autograd is deformable_logits_autograd
    assert gaussianformer_amd.DeformLogitsFunction is DeformLogitsFunction


# ---- the Python function ---------------------------------------------------------------------------------------------------------

def _layers(k=2, nw=144):
    return nn.Linear(128, nw), nn.Linear(128, 3 * k) if k else None


def test_the_function_refuses_cpu_tensors_and_bad_arguments():
    wfc, lfc = _layers()
    f, e = tr.fixed_input(4, 128, 1), tr.fixed_input(4, 128, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        deformable_logits_autograd(f.clone().requires_grad_(True), e, wfc, lfc)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        deformable_logits_autograd(f, e, wfc, lfc)
    with pytest.raises(ValueError, match="weights_fc is a LayerNorm without weight and bias, not an Linear"):
        deformable_logits_autograd(f, e, nn.LayerNorm(128), lfc)
    # deformable_logits itself keeps refusing autograd, with its message
    with pytest.raises(RuntimeError, match="deformable_logits is a forward without a native backward"):
        deformable_logits(f.clone().requires_grad_(True), e, wfc, lfc)
    assert issubclass(DeformLogitsFunction, torch.autograd.Function)
    sig = inspect.signature
    assert list(sig(deformable_logits_autograd).parameters) == list(sig(deformable_logits).parameters)
    assert [p.default for p in sig(deformable_logits_autograd).parameters.values()] == [p.default for p in sig(deformable_logits).parameters.values()]


def test_the_shape_checks_are_the_plain_function_s(monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu", lambda *a: None)
    monkeypatch.setattr(_lib, "call", lambda name, *a: None)
    wfc, lfc = _layers()
    f = tr.fixed_input(4, 128, 1)
    for fn, grad in ((deformable_logits_autograd, True), (deformable_logits_autograd, False), (deformable_logits, False)):
        name = fn.__name__
        x = f.clone().requires_grad_(grad)
        for p in [*wfc.parameters(), *lfc.parameters()]:
            p.requires_grad_(grad)
        with pytest.raises(ValueError, match=name + r": instance_feature \[\.\.\., 128\] against weights_fc \(144, 64\)"):
            fn(x, None, (torch.zeros(144, 64), torch.zeros(144)), lfc)
        with pytest.raises(ValueError, match=name + r": instance_feature .* and learnable_fc \(5, 128\), \(5,\)"):
            fn(x, None, wfc, (torch.zeros(5, 128), torch.zeros(5)))
        with pytest.raises(ValueError, match=name + r": anchor_embed \(3, 128\) is not \(4, 128\)"):
            fn(x, f[:3], wfc, lfc)


def test_with_nothing_that_needs_autograd_it_is_the_inference_launch(monkeypatch):
    names = []
    monkeypatch.setattr(_lib, "require_gpu", lambda *a: None)
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name))
    wfc, lfc = _layers()
    f, e = tr.fixed_input(2 * 3, 128, 1).view(2, 3, 128), tr.fixed_input(2 * 3, 128, 2).view(2, 3, 128)
    with torch.no_grad():
        raw, learned = deformable_logits_autograd(f, e, wfc, lfc)
        assert raw.shape == (2, 3, 144) and learned.shape == (2, 3, 2, 3) and not raw.requires_grad
    for p in [*wfc.parameters(), *lfc.parameters()]:
        p.requires_grad_(False)
    raw, learned = deformable_logits_autograd(f, None, wfc)
    assert learned is None and not raw.requires_grad
    assert names == ["gf_deform_logits_forward"] * 2
    del names[:]
    # anything that requires grad: the same forward launch under the Function; a gradient nobody needs gets None and the
    # library a NULL slot
    wfc.weight.requires_grad_(True)
    seen = {}
    real_table = _lib.out_table
    monkeypatch.setattr(_lib, "out_table", lambda tensors, count: seen.setdefault("grads", list(tensors)) and real_table(tensors, count))
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.setdefault(name, a), real_call(name, *a))[1])
    fg = f.clone().requires_grad_(True)
    raw, learned = deformable_logits_autograd(fg, e, wfc, lfc)
    assert names == ["gf_deform_logits_forward"] and raw.requires_grad and learned.requires_grad
    assert raw.shape == (2, 3, 144) and learned.shape == (2, 3, 2, 3)
    (raw.sum() + learned.sum()).backward()
    assert names == ["gf_deform_logits_forward", "gf_deform_logits_backward"]
    assert [g is not None for g in seen["grads"]] == [False, False, True, False]          # the table's order: Wl, bl, Ww, bw
    args = seen["gf_deform_logits_backward"]
    assert args[1:5] == (6, 128, 6, 144) and args[8] is not None and args[9] is not None
    assert args[10] is not None and args[11] is None                                          # grad_feature asked for, grad_embed not
    assert fg.grad is not None and fg.grad.shape == (2, 3, 128) and wfc.weight.grad is not None
    assert wfc.bias.grad is None and lfc.weight.grad is None and e.grad is None
    # an output nobody used is a NULL cotangent
    seen.clear()
    raw, learned = deformable_logits_autograd(fg, e, wfc, lfc)
    raw.sum().backward()
    assert seen["gf_deform_logits_backward"][8] is None and seen["gf_deform_logits_backward"][9] is not None
    # ... and it is once-differentiable: the gradient carries no graph
    raw, _ = deformable_logits_autograd(fg, e, wfc, lfc)
    g, = torch.autograd.grad(raw.sum(), fg, create_graph=True)
    assert not g.requires_grad


# ---- the switches ----------------------------------------------------------------------------------------------------------------

KPS = dict(type="SparseGaussian3DKeyPointsGenerator", num_learnable_pts=2, fix_scale=[[0, 0, 0], [0.45, 0, 0]],
           pc_range=[-50.0, -50.0, -5.0, 50.0, 50.0, 3.0], scale_range=[0.08, 0.64])


def _deformable(learnable=2, **over):
    cfg = dict(embed_dims=128, num_groups=4, num_levels=2, num_cams=2, use_deformable_func=True, use_camera_embed=False, residual_mode="none",
               kps_generator=dict(KPS, num_learnable_pts=learnable))
    cfg.update(over)
    return DeformableFeatureAggregation(**cfg)


def test_defaults_and_what_set_native_touches():
    m = _deformable()
    assert DeformableFeatureAggregation.native_front_training is False and m.native_front_training is False
    assert "native_front_training" not in inspect.signature(DeformableFeatureAggregation.__init__).parameters
    m.native_front_training = True
    assert not any("native_front_training" in k for k in m.state_dict()) and _deformable().native_front_training is False
    assert "front_training" in inspect.signature(GaussianOccEncoder.set_native).parameters
    assert inspect.signature(GaussianOccEncoder.set_native).parameters["front_training"].default is None

    with open(GOLDEN) as f:
        enc = _encoder(json.load(f)["prob/nuscenes_gs6400"])
    blocks = [m for m in enc.modules() if isinstance(m, DeformableFeatureAggregation)]
    assert blocks and all(m.native_front_training is False for m in blocks)
    before = {id(m): dict(vars(m)) for m in enc.modules()}
    changed = lambda: {k for m in enc.modules() for k, v in vars(m).items() if k not in before[id(m)] or before[id(m)][k] is not v}
    assert enc.set_native(front_training=True) is enc and changed() == {"native_front_training"}
    assert all(m.native_front_training is True and m.native_training is False for m in blocks) and enc.fold_training is False
    enc.set_native(front_training=False)
    # training= and fold_training= do not touch it
    enc.set_native(training=True, fold_training=True)
    assert all(m.native_front_training is False and m.native_training is True for m in blocks)
    enc.set_native(front_training=True)
    enc.set_native(training=False, fold_training=False)
    assert all(m.native_front_training is True and m.native_training is False for m in blocks)
    assert DeformableFeatureAggregation.native_front_training is False


class _Gpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the routing questions look at ``is_cuda`` and ``dtype`` only."""
    is_cuda = True


def _gpu(t, grad=False):
    return t.as_subclass(_Gpu).requires_grad_(grad)


def test_routing_conditions(monkeypatch):
    def ask(m, grad=True, dtype=torch.float32, cuda=True):
        wrap = _gpu if cuda else (lambda t, g=False: t.requires_grad_(g))
        monkeypatch.setattr(m, "parameters", lambda recurse=True: iter([wrap(torch.zeros(2, dtype=dtype))]))
        inst = wrap(torch.zeros(1, 3, 128, dtype=dtype), grad)
        other = wrap(torch.zeros(1, 3, 128, dtype=dtype))
        return m._native_front_training(inst, other, other, other)

    m = _deformable()
    assert ask(m) is False                                          # off by default: the torch layers
    m.native_front_training = True
    assert ask(m) is True
    assert ask(m, grad=False) is False                              # nothing requires grad: the inference route's business
    with torch.no_grad():
        assert ask(m) is False
    assert ask(m, dtype=torch.float64) is False and ask(m, cuda=False) is False
    m.train()
    m.attn_drop, m.proj_drop.p = 0.1, 0.1
    assert ask(m) is True                                           # train or eval, any dropout: the front lies before them
    ten, eleven = _deformable(learnable=10), _deformable(learnable=11)
    ten.native_front_training = eleven.native_front_training = True
    assert ask(ten) is True and ask(eleven) is False                # 3 K <= 32
    zero = _deformable(learnable=0)
    zero.native_front_training = True
    assert ask(zero) is True
    wide = _deformable(embed_dims=256)
    wide.native_front_training = True
    assert ask(wide) is False
    # independent of the back end's switch
    m.native_training = True
    assert ask(m) is True
    m.native_front_training = False
    assert ask(m) is False


@pytest.mark.parametrize("learnable", [2, 0])
def test_the_block_hands_its_front_to_the_function(learnable, monkeypatch):
    """With the switch, ``forward_torch`` takes ``raw`` and ``learned`` from ``deformable_logits_autograd`` and the key points
    from the functional ``key_points``; ``weights_fc``, ``learnable_fc`` and the generator never run as modules."""
    m = _deformable(learnable).eval()
    m.native_front_training = True
    calls, kps, ran = [], [], []
    feats = torch.zeros(1, 3, 128)
    pts = m.num_pts
    raw, learned = torch.zeros(1, 3, 2 * 2 * pts * 4), torch.zeros(1, 3, learnable, 3) if learnable else None
    monkeypatch.setattr(db, "deformable_fused", lambda *a, **k: calls.append(("fused", a, k)) or feats)
    monkeypatch.setattr(db, "deformable_fused_forward", lambda *a, **k: calls.append(("fused", a, k)) or feats)
    monkeypatch.setattr(db, "deformable_logits_autograd", lambda *a: calls.append(("logits", a)) or (raw, learned))
    kp = torch.zeros(1, 3, pts, 3)
    monkeypatch.setattr(db, "key_points", lambda *a: kps.append(a) or kp)
    monkeypatch.setattr(m, "_native", lambda *a: False)
    monkeypatch.setattr(m, "_native_front_training", lambda *a: True)
    mods = [m.weights_fc, m.kps_generator] + ([m.kps_generator.learnable_fc] if learnable else [])
    for mod in mods:
        mod.register_forward_hook(lambda *a: ran.append(1))
    inst, anchor, emb = torch.zeros(1, 3, 128, requires_grad=True), torch.zeros(1, 3, 11), torch.zeros(1, 3, 128)
    table = (torch.zeros(4, 128), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    metas = dict(projection_mat=torch.eye(4).repeat(1, 2, 1, 1), image_wh=torch.ones(1, 2, 2))
    out = m(inst, anchor, emb, table, metas)
    assert out.shape == (1, 3, 128) and not ran
    assert [c[0] for c in calls] == ["logits", "fused"]
    got = calls[0][1]
    assert got[0] is inst and got[1] is emb and got[2] is m.weights_fc and got[3] is (m.kps_generator.learnable_fc if learnable else None)
    gen = m.kps_generator
    assert len(kps) == 1 and kps[0][0] is anchor and kps[0][1] is learned and kps[0][2] is gen._fix
    assert kps[0][3:] == (gen.pc_range, gen.scale_range, gen.learnable_fixed_scale, gen.xyz_act, gen.scale_act)
    fused = calls[1]
    assert fused[1][0] is kp and fused[2]["raw_weights"].shape == (1, 3, 2, 2, pts, 4)
    assert fused[2]["raw_weights"].data_ptr() == raw.data_ptr()
    # without the switch: the torch layers
    monkeypatch.setattr(m, "_native_front_training", lambda *a: False)
    del calls[:]
    monkeypatch.setattr(gen, "forward", lambda anchor, feature: kp)
    m(inst, anchor, emb, table, metas)
    assert [c[0] for c in calls] == ["fused"] and len(ran) == 2 and len(kps) == 1       # weights_fc and the generator ran


# ---- why the bias gradients are summed in double -----------------------------------------------------------------------------------

def test_a_float_tree_cannot_hold_the_cancelling_column():
    """DESIGN.md §3.13g's figures, on the CPU: at Nw = 864, n = 511 the fixed cotangent ``cos(0.37 i)`` cancels over a column to
    0.074 out of 511 terms.  ``tile_sum``'s order in float32 (a pairwise tree over a wave's 32 rows, the four waves, then the
    tiles) is 4.7e-5 of ``max|truth|`` off, while the float32 rounding of the cotangent
    alone is 1.4e-5: summed in double, that rounding is all that is left."""
    n, nw = 511, 864
    w64 = tr.output_weights((n, nw))
    truth = w64.sum(0)
    scale = truth.abs().max().item()
    w32 = w64.float()
    rows = torch.cat([w32, torch.zeros(-n % 128, nw)]).view(-1, 4, 32, nw)

    def tree(x):
        while x.shape[0] > 1:
            x = x[0::2] + x[1::2]
        return x[0]
    waves = torch.stack([torch.stack([tree(rows[t, w]) for w in range(4)]) for t in range(rows.shape[0])])
    tiles = (waves[:, 0] + waves[:, 1]) + (waves[:, 2] + waves[:, 3])
    assert tiles.shape[0] == 4
    in_float = (tiles[0] + tiles[1]) + (tiles[2] + tiles[3])
    rel = lambda got: (got.double() - truth).abs().max().item() / scale
    assert 0.07 < scale < 0.08
    assert 4.5e-5 < rel(in_float) < 4.9e-5
    assert 1.3e-5 < rel(w32.double().sum(0).float()) < 1.6e-5
