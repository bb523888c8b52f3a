"""The training step of the deformable block's dense back without a GPU (``gf_deform_output_train_sizes``,
``gf_deform_output_forward_train``, ``gf_deform_output_backward``, ``deformable_output_autograd``, the modules'
``native_training`` / ``native_tail_training`` and the encoder's ``fold_training``): the restatement against torch's float64
autograd, every refusal of the three entries on host buffers (they come before any HIP call), the sizes query, and the
routing conditions with the library call stubbed."""
import ctypes
import inspect
import json

import pytest
import torch
import torch.nn as nn

import deform_output_train_ref as tr
from gaussianformer_amd import GaussianOccEncoder, _lib
from gaussianformer_amd import deformable_block as db
from gaussianformer_amd.deformable_block import (DeformableFeatureAggregation, DeformOutputFunction, deformable_output,
                                                 deformable_output_autograd, output_train_sizes)
from gaussianformer_amd.ffn import AsymmetricFFN
from gaussianformer_amd.sparse_conv import SparseConv3D
from row_judge import ptr_table
from test_encoder import GOLDEN, _encoder

CPU = torch.device("cpu")
B = _lib.GF_DEFORM_OUTPUT_WGRAD_ROWS
NONE, ADD, CAT = _lib.GF_DEFORM_NONE, _lib.GF_DEFORM_ADD, _lib.GF_DEFORM_CAT


# ---- the restatement -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(tr.VARIANTS))
def test_restatement_is_torch_s_float64_autograd(name):
    """``output_train_ref`` and ``scalar_gradients`` against nn.Linear, the add or the cat and nn.LayerNorm under autograd."""
    mode, has_res, has_norm = tr.VARIANTS[name]
    n = 37
    sd = tr.weights(has_norm, dtype=torch.float64)
    x, f = tr.planted(tr.fixed_input(n, 128, 1)).double(), tr.fixed_input(n, 128, 2).double()
    res = tr.fixed_input(n, 128, 3).double() if has_res else None
    inst = None if mode == "none" else f
    got = tr.gradients(lambda x_, f_, r_, leaves: tr.output_train_ref(x_, f_, r_, leaves, mode), x, inst, res, sd)

    proj, norm = nn.Linear(128, 128).double(), nn.LayerNorm(128).double()
    with torch.no_grad():
        proj.weight.copy_(sd["output_proj.weight"])
        proj.bias.copy_(sd["output_proj.bias"])
        if has_norm:
            norm.weight.copy_(sd["norm.weight"])
            norm.bias.copy_(sd["norm.bias"])
    xl, fl = x.clone().requires_grad_(True), f.clone().requires_grad_(True)
    rl = None if res is None else res.clone().requires_grad_(True)
    y = proj(xl)
    y = y + fl if mode == "add" else torch.cat([y, fl], dim=-1) if mode == "cat" else y
    y = y if rl is None else y + rl
    y = norm(y) if has_norm else y
    (y * tr.output_weights(y.shape)).sum().backward()
    want = {"out": y.detach(), "features": xl.grad, "output_proj.weight": proj.weight.grad, "output_proj.bias": proj.bias.grad}
    if mode != "none":
        want["instance_feature"] = fl.grad
    if rl is not None:
        want["residual"] = rl.grad
    if has_norm:
        want.update({"norm.weight": norm.weight.grad, "norm.bias": norm.bias.grad})
    assert set(got) == set(want)
    for k in want:
        scale = max(want[k].abs().max().item(), 1e-30)
        assert got[k].shape == want[k].shape and (got[k] - want[k]).abs().max().item() <= 1e-12 * scale, k
    if mode == "cat":       # the right half's gradient is the cotangent's right half
        assert torch.equal(got["instance_feature"], tr.output_weights((n, 256))[:, 128:])
    assert tr.kind("output_proj.weight") == "matrix" and {tr.kind(k) for k in tr.KEYS[1:]} == {"vector"}


# ---- the entries on host buffers -----------------------------------------------------------------------------------------------

def _bufs(count, floats=1 << 15):
    """``count`` disjoint 16-byte aligned host tensors."""
    bufs = [torch.zeros(floats) for _ in range(count)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    return bufs


class Host:
    """One call's host buffers: every tensor its own allocation, so that only the aliasing a case asks for is there."""

    def __init__(self):
        (self.x, self.f, self.res, self.out, self.go, self.gx, self.gi, self.gr, self.saved, self.work) = _bufs(10)
        self.params, self.grads = _bufs(4, 1 << 14), _bufs(4, 1 << 14)

    def table(self, tensors, drop=(), misalign=None):
        entries = [None if i in drop else t.data_ptr() + (4 if i == misalign else 0) for i, t in enumerate(tensors)]
        return ptr_table(entries)


def _at(t, off):
    return None if t is None else t.data_ptr() + off


def _fwd(n=4, e=128, mode=ADD, drop=(), misalign=None, null_params=False, saved_bytes=None, saved_off=0, **over):
    h = Host()
    t = dict(x=h.x, f=h.f, res=None, out=h.out, saved=h.saved)
    t.update(over)
    need = output_train_sizes(max(n, 0), "none", with_norm=2 not in drop)[0]      # (the sizes do not depend on the mode)
    _lib.call("gf_deform_output_forward_train", CPU, n, e, mode, _at(t["x"], 0), _at(t["f"], 0), None if null_params else h.table(h.params, drop, misalign),
              _at(t["res"], 0), _at(t["out"], 0), _at(t["saved"], saved_off), need if saved_bytes is None else saved_bytes)


def _bwd(n=4, e=128, mode=ADD, drop=(), misalign=None, gdrop=None, gmisalign=None, null_params=False, null_grads=False, work_bytes=None,
         offs=None, **over):
    h = Host()
    t = dict(x=h.x, saved=h.saved, go=h.go, gx=h.gx, gi=h.gi if mode != NONE else None, gr=h.gr if mode != CAT else None, work=h.work)
    t.update(over)
    offs = offs or {}
    need = output_train_sizes(max(n, 0), "none", with_norm=2 not in drop)[1]
    gdrop = drop if gdrop is None else gdrop
    at = lambda k: _at(t[k], offs.get(k, 0))
    _lib.call("gf_deform_output_backward", CPU, n, e, mode, at("x"), None if null_params else h.table(h.params, drop, misalign), at("saved"),
              at("go"), at("gx"), at("gi"), at("gr"), None if null_grads else h.table(h.grads, gdrop, gmisalign), at("work"),
              need if work_bytes is None else work_bytes)
    return h


@pytest.mark.parametrize("entry, run", [("gf_deform_output_forward_train", _fwd), ("gf_deform_output_backward", _bwd)])
def test_what_the_plain_forward_refuses(entry, run):
    fail = entry + r" failed \(code -1\): " + entry + ": "
    for kw, msg in ((dict(e=32), r"E = 32: only embed_dims = 128"), (dict(mode=3), r"mode = 3 is not GF_DEFORM_NONE / ADD / CAT"),
                    (dict(n=-2), r"n = -2 is negative"), (dict(null_params=True), r"null params"),
                    (dict(drop=(0, 2, 3)), r"output_proj.weight is missing"), (dict(drop=(1, 2, 3)), r"output_proj.bias is missing"),
                    (dict(drop=(2,)), r"a half-present pair: norm.weight is null and norm.bias is not"),
                    (dict(drop=(3,)), r"a half-present pair: norm.bias is null and norm.weight is not"),
                    (dict(mode=CAT), r"a post norm with mode = 2 \(GF_DEFORM_CAT\)"),
                    (dict(misalign=0), r"output_proj.weight is not 16-byte aligned"), (dict(misalign=3), r"norm.bias is not 16-byte aligned")):
        with pytest.raises(RuntimeError, match=fail + msg):
            run(**kw)


def test_forward_train_refusals():
    fail = r"gf_deform_output_forward_train failed \(code -1\): gf_deform_output_forward_train: "
    h = Host()
    for kw, msg in ((dict(mode=CAT, drop=(2, 3), res=h.res), r"a residual with mode = 2"),
                    (dict(x=h.x[1:]), r"features is not 16-byte aligned"), (dict(f=h.f[2:]), r"instance_feature is not 16-byte aligned"),
                    (dict(res=h.res[3:]), r"residual is not 16-byte aligned"), (dict(out=h.out[1:]), r"out is not 16-byte aligned"),
                    (dict(saved_off=4), r"saved is not 16-byte aligned"), (dict(saved=None), r"saved is null"),
                    (dict(x=None), r"null pointer"), (dict(f=None), r"null pointer"), (dict(out=None), r"null pointer")):
        with pytest.raises(RuntimeError, match=fail + msg):
            _fwd(**kw)
    shared = torch.zeros(1 << 15)
    for kw, msg in ((dict(x=shared, out=shared[256:]), r"out aliases an input"), (dict(res=shared, out=shared[128:]), r"out aliases an input"),
                    (dict(out=shared, saved=shared[256:]), r"saved aliases out"), (dict(f=shared, saved=shared[128:]), r"saved aliases an input")):
        with pytest.raises(RuntimeError, match=fail + msg):
            _fwd(**kw)
    need = output_train_sizes(4, "add", True)[0]
    with pytest.raises(RuntimeError, match=rf"forward_train failed \(code -2\): gf_deform_output_forward_train: saved of {need - 1} bytes, {need} needed"):
        _fwd(saved_bytes=need - 1)
    # n == 0 is GF_OK without a launch, with or without a saved region
    _fwd(n=0)
    _fwd(n=0, saved=None, drop=(2, 3), mode=NONE, f=None)


def test_backward_refusals():
    fail = r"gf_deform_output_backward failed \(code -1\): gf_deform_output_backward: "
    for kw, msg in ((dict(mode=NONE, gi=Host().gi), r"grad_instance with mode = 0 \(GF_DEFORM_NONE\)"),
                    (dict(mode=CAT, drop=(2, 3), gr=Host().gr), r"grad_residual with mode = 2 \(GF_DEFORM_CAT\)"),
                    (dict(null_grads=True), r"null grad_params"),
                    (dict(drop=(2, 3), gdrop=(3,)), r"a gradient for norm.weight, which is absent"),
                    (dict(gmisalign=0), r"the gradient of output_proj.weight is not 16-byte aligned"),
                    (dict(gmisalign=3), r"the gradient of norm.bias is not 16-byte aligned"),
                    (dict(offs=dict(x=4)), r"features is not 16-byte aligned"), (dict(offs=dict(go=8)), r"grad_out is not 16-byte aligned"),
                    (dict(offs=dict(gx=4)), r"grad_features is not 16-byte aligned"), (dict(offs=dict(gi=12)), r"grad_instance is not 16-byte aligned"),
                    (dict(offs=dict(gr=4)), r"grad_residual is not 16-byte aligned"), (dict(offs=dict(saved=8)), r"saved is not 16-byte aligned"),
                    (dict(offs=dict(work=4)), r"workspace is not 16-byte aligned"),
                    (dict(saved=None), r"saved is null"), (dict(work=None), r"workspace is null"),
                    (dict(x=None), r"null pointer"), (dict(go=None), r"null pointer"), (dict(gx=None), r"null pointer")):
        with pytest.raises(RuntimeError, match=fail + msg):
            _bwd(**kw)
    need = output_train_sizes(4, "add", True)[1]
    with pytest.raises(RuntimeError, match=rf"backward failed \(code -2\): gf_deform_output_backward: workspace of {need - 1} bytes, {need} needed"):
        _bwd(work_bytes=need - 1)
    # an output that aliases an input, the saved region, the workspace or another output
    s = torch.zeros(1 << 15)
    for kw, msg in ((dict(x=s, gx=s[256:]), r"grad_features aliases an input"), (dict(go=s, gi=s[128:]), r"grad_instance aliases an input"),
                    (dict(saved=s, gr=s[256:]), r"grad_residual aliases the saved region"), (dict(work=s, gx=s[512:]), r"grad_features aliases the workspace"),
                    (dict(gx=s, gi=s[256:]), r"grad_instance aliases grad_features"), (dict(gi=s, gr=s[128:]), r"grad_residual aliases grad_instance")):
        with pytest.raises(RuntimeError, match=fail + msg):
            _bwd(**kw)
    h = Host()
    with pytest.raises(RuntimeError, match=fail + r"the gradient of output_proj.bias aliases an input"):
        _lib.call("gf_deform_output_backward", CPU, 4, 128, ADD, h.x, h.table(h.params), h.saved, h.go, h.gx, h.gi, h.gr,
                  h.table([h.grads[0], h.params[1], h.grads[2], h.grads[3]]), h.work, 1 << 17)
    with pytest.raises(RuntimeError, match=fail + r"the gradient of norm.weight aliases the gradient of output_proj.weight"):
        _lib.call("gf_deform_output_backward", CPU, 4, 128, ADD, h.x, h.table(h.params), h.saved, h.go, h.gx, h.gi, h.gr,
                  h.table([h.grads[0], h.grads[1], h.grads[0][4096:], h.grads[3]]), h.work, 1 << 17)
    # a NULL slot is a gradient nobody asked for: the refusal that follows is the next one
    with pytest.raises(RuntimeError, match=fail + r"workspace is null"):
        _bwd(gdrop=(0, 1, 2, 3), work=None)
    # without a post norm no saved region is needed
    with pytest.raises(RuntimeError, match=fail + r"workspace is null"):
        _bwd(drop=(2, 3), saved=None, work=None)


def test_train_sizes():
    lib = _lib.load()
    assert B == 512 and B % 128 == 0
    for mode, with_norm in (("none", False), ("add", False), ("cat", False), ("none", True), ("add", True)):
        assert output_train_sizes(0, mode, with_norm) == (0, 0)
        last = (0, 0)
        for n in sorted({1, 31, 32, 33, 128, 129, 1000, B - 1, B, B + 1, 6400, 25600, 144000}):
            saved, work = output_train_sizes(n, mode, with_norm)
            if with_norm:
                assert 520 * n <= saved <= 520 * n + 4096, (n, saved)      # the row the norm reads and (mean, rstd)
            else:
                assert saved == 0                                         # linear: the backward needs features and Wo only
            blocks, tiles = (n + B - 1) // B, (n + 127) // 128
            partials = blocks * 128 * 128 * 4 + tiles * 3 * 128 * 4
            assert partials <= work <= partials + (512 * n if with_norm else 0) + 1024, (n, work)
            assert saved >= last[0] and work >= last[1] and work > 0 and saved % 16 == 0 and work % 16 == 0
            last = (saved, work)
    out = ctypes.c_size_t(0)
    a = ctypes.addressof(out)
    for args, message in (((-1, 128, 1, 0, a, a), b"n = -1 is negative"), ((4, 256, 1, 0, a, a), b"E = 256"), ((4, 128, 5, 0, a, a), b"mode = 5"),
                          ((4, 128, 2, 1, a, a), b"a post norm with mode = 2"), ((4, 128, 1, 0, None, a), b"null pointer")):
        assert lib.gf_deform_output_train_sizes(*args) == -1 and message in lib.gf_last_error()


def test_constants_and_build_list():
    from gaussianformer_amd import build as build_mod
    assert "deform_dense_train.hip" in build_mod.SOURCES and "deform_dense_train.hip" not in build_mod.FP_ATOMICS
    assert "gf_deform.hpp" in build_mod.HEADERS and "gf_rows_bwd.hpp" in build_mod.HEADERS
    for name in ("gf_deform_output_train_sizes", "gf_deform_output_forward_train", "gf_deform_output_backward"):
        assert name in _lib.SIGNATURES
    assert _lib.GF_ABI_VERSION == 10 and _lib.load().gf_abi_version() == 10


# ---- the Python function ---------------------------------------------------------------------------------------------------------

def test_the_function_refuses_cpu_tensors_and_bad_arguments():
    proj, norm = nn.Linear(128, 128), nn.LayerNorm(128)
    x, f = tr.fixed_input(4, 128, 1), tr.fixed_input(4, 128, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        deformable_output_autograd(x.clone().requires_grad_(True), proj, f, "add")
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        deformable_output_autograd(x, proj, f, "add")
    with pytest.raises(ValueError, match="deformable_output_autograd: residual_mode 'mul' is not one of"):
        deformable_output_autograd(x, proj, f, "mul")
    with pytest.raises(ValueError, match="deformable_output_autograd: residual_mode 'cat' needs instance_feature"):
        deformable_output_autograd(x, proj, None, "cat")
    with pytest.raises(ValueError, match="eps = 1e-5"):
        deformable_output_autograd(x, proj, f, "add", norm=nn.LayerNorm(128, eps=1e-6))
    # deformable_output itself keeps refusing autograd, with its message
    with pytest.raises(RuntimeError, match="deformable_output is a forward without a native backward"):
        deformable_output(x.clone().requires_grad_(True), proj, f, "add", norm=norm)
    assert issubclass(DeformOutputFunction, torch.autograd.Function)
    sig = inspect.signature
    assert list(sig(deformable_output_autograd).parameters) == list(sig(deformable_output).parameters)
    assert [p.default for p in sig(deformable_output_autograd).parameters.values()] == [p.default for p in sig(deformable_output).parameters.values()]


def test_with_nothing_that_needs_autograd_it_is_the_inference_launch(monkeypatch):
    names = []
    monkeypatch.setattr(_lib, "require_gpu", lambda *a: None)
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name))
    proj, norm = nn.Linear(128, 128), nn.LayerNorm(128)
    x, f = tr.fixed_input(4, 128, 1), tr.fixed_input(4, 128, 2)
    with torch.no_grad():
        assert deformable_output_autograd(x, proj, f, "cat").shape == (4, 256)
    for p in [*proj.parameters(), *norm.parameters()]:
        p.requires_grad_(False)
    deformable_output_autograd(x, proj, None, "none", residual=f, norm=norm)
    assert names == ["gf_deform_output_forward"] * 2
    del names[:]
    # anything that requires grad: the saving launch; a gradient nobody needs gets None and the library a NULL slot
    proj.weight.requires_grad_(True)
    seen = {}
    real_table = _lib.out_table
    monkeypatch.setattr(_lib, "out_table", lambda tensors, count: seen.setdefault("grads", list(tensors)) and real_table(tensors, count))
    xg = x.clone().requires_grad_(True)
    out = deformable_output_autograd(xg, proj, f, "add", residual=f.clone(), norm=norm)
    assert names == ["gf_deform_output_forward_train"] and out.requires_grad and out.shape == (4, 128)
    out.sum().backward()
    assert names == ["gf_deform_output_forward_train", "gf_deform_output_backward"]
    assert [g is not None for g in seen["grads"]] == [True, False, False, False]
    assert xg.grad is not None and proj.weight.grad is not None and proj.bias.grad is None and norm.weight.grad is None


# ---- the modules' switches ---------------------------------------------------------------------------------------------------------

KPS = dict(type="SparseGaussian3DKeyPointsGenerator", num_learnable_pts=2, fix_scale=[[0, 0, 0], [0.45, 0, 0]],
           pc_range=[-50.0, -50.0, -5.0, 50.0, 50.0, 3.0], scale_range=[0.08, 0.64])


def _deformable(**over):
    cfg = dict(embed_dims=128, num_groups=4, num_levels=2, num_cams=2, use_deformable_func=True, use_camera_embed=False, residual_mode="none",
               kps_generator=dict(KPS))
    cfg.update(over)
    return DeformableFeatureAggregation(**cfg)


def test_defaults_and_what_set_native_touches():
    m = _deformable()
    assert DeformableFeatureAggregation.native_training is False and m.native_training is False
    assert "native_training" not in inspect.signature(DeformableFeatureAggregation.__init__).parameters
    m.native_training = True
    assert not any("native_training" in k for k in m.state_dict()) and _deformable().native_training is False
    kw = dict(pc_range=[-5.0, -5.0, -2.5, 5.0, 5.0, 2.5], grid_size=[2.0, 2.0, 1.0])
    s = SparseConv3D(128, 128, use_out_proj=True, **kw)
    assert SparseConv3D.native_tail_training is False and s.native_tail_training is False and SparseConv3D.native_training is False
    assert "native_tail_training" not in inspect.signature(SparseConv3D.__init__).parameters
    assert not any("native_tail_training" in k for k in s.state_dict())
    assert GaussianOccEncoder.fold_training is False and "fold_training" not in inspect.signature(GaussianOccEncoder.__init__).parameters

    with open(GOLDEN) as f:
        enc = _encoder(json.load(f)["prob/nuscenes_gs6400"])
    assert enc.fold_training is False and not any("fold_training" in k for k in enc.state_dict())
    blocks = [m for m in enc.modules() if isinstance(m, DeformableFeatureAggregation)]
    sparse = [m for m in enc.modules() if isinstance(m, SparseConv3D)]
    assert blocks and sparse
    before = {id(m): dict(vars(m)) for m in enc.modules()}
    changed = lambda: {k for m in enc.modules() for k, v in vars(m).items() if k not in before[id(m)] or before[id(m)][k] is not v}
    # training= picks the deformable block up by the hasattr rule and leaves the fold alone
    assert enc.set_native(training=True) is enc and changed() == {"native_training"}
    assert all(m.native_training is True for m in blocks + sparse) and enc.fold_training is False
    assert all(m.native_tail_training is False for m in sparse)
    # fold_training= sets the encoder's attribute and the sparse blocks' tail switch, nothing else
    assert enc.set_native(fold_training=True) is enc and changed() == {"native_training", "fold_training", "native_tail_training"}
    assert enc.fold_training is True and all(m.native_tail_training is True for m in sparse)
    enc.set_native(training=False)
    assert enc.fold_training is True and all(m.native_training is False for m in blocks)
    enc.set_native(fold_training=False)
    assert enc.fold_training is False and all(m.native_tail_training is False for m in sparse)
    assert GaussianOccEncoder.fold_training is False and SparseConv3D.native_tail_training is False


class _Gpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the routing questions look at ``is_cuda`` and ``dtype`` only."""
    is_cuda = True


def _gpu(t, grad=False):
    return t.as_subclass(_Gpu).requires_grad_(grad)


def test_deformable_block_routing_conditions(monkeypatch):
    def ask(m, grad=True, dtype=torch.float32, residual=True, norm=True, cuda=True):
        wrap = _gpu if cuda else (lambda t, g=False: t.requires_grad_(g))
        monkeypatch.setattr(m, "parameters", lambda recurse=True: iter([wrap(torch.zeros(2, dtype=dtype))]))
        inst = wrap(torch.zeros(1, 3, 128, dtype=dtype), grad)
        other = wrap(torch.zeros(1, 3, 128, dtype=dtype))
        ln = nn.LayerNorm(128) if norm is True else norm
        if isinstance(ln, nn.LayerNorm) and ln.weight is not None:
            ln.weight, ln.bias = (nn.Parameter(wrap(v), requires_grad=grad) for v in (torch.ones(128, dtype=dtype), torch.zeros(128, dtype=dtype)))
        args = (inst, other, other, other, other if residual else None, ln)
        return m._native_training(*args), m._native(*args)

    m = _deformable()
    assert ask(m) == (False, False)                               # off by default: today's torch route
    m.native_training = True
    assert ask(m) == (True, False)
    assert ask(m, grad=False) == (False, True)                    # nothing needs autograd: the inference route
    with torch.no_grad():
        assert ask(m)[0] is False
    assert ask(m, dtype=torch.float64)[0] is False and ask(m, cuda=False)[0] is False
    assert ask(m, norm=nn.LayerNorm(128, eps=1e-6))[0] is False
    assert ask(m, norm=nn.LayerNorm(128, elementwise_affine=False))[0] is False
    assert ask(m, norm=nn.Identity())[0] is False
    assert ask(m, norm=None, residual=False)[0] is True
    m.train()
    m.proj_drop.p = 0.1
    assert ask(m)[0] is False                                     # an active proj_drop keeps its torch route
    m.eval()
    assert ask(m)[0] is True
    m.residual_mode = "mul"
    assert ask(m)[0] is False
    c = _deformable(residual_mode="cat")
    c.native_training = True
    assert ask(c, residual=False, norm=None)[0] is True and ask(c)[0] is False          # no add or norm behind a cat
    w = _deformable(embed_dims=64)
    w.native_training = True
    assert ask(w)[0] is False


def test_deformable_block_hands_features_to_the_function(monkeypatch):
    """With the switch, ``forward_torch`` runs as it is up to ``features``; ``output_proj``, ``proj_drop`` and the norm module
    are never called."""
    m = _deformable().eval()
    m.native_training = True
    calls, ran = [], []
    feats = torch.zeros(1, 3, 128)
    monkeypatch.setattr(db, "deformable_fused", lambda *a, **k: feats)
    monkeypatch.setattr(m.kps_generator, "forward", lambda anchor, feature: torch.zeros(1, 3, 4, 3))
    monkeypatch.setattr(db, "deformable_output_autograd", lambda *a: calls.append(a) or "out")
    monkeypatch.setattr(m, "_native", lambda *a: False)
    monkeypatch.setattr(m, "_native_training", lambda *a: True)
    norm = nn.LayerNorm(128)
    for mod in (m.output_proj, m.proj_drop, norm):
        mod.register_forward_hook(lambda *a: ran.append(1))
    inst, anchor = torch.zeros(1, 3, 128, requires_grad=True), torch.zeros(1, 3, 11)
    table = (torch.zeros(4, 128), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    metas = dict(projection_mat=torch.eye(4).repeat(1, 2, 1, 1), image_wh=torch.ones(1, 2, 2))
    res = torch.zeros(1, 3, 128)
    assert m(inst, anchor, inst, table, metas, residual=res, norm=norm) == "out"
    assert len(calls) == 1 and not ran
    got = calls[0]
    assert got[0] is feats and got[1] is m.output_proj and got[2] is inst and got[3] == "none" and got[4] is res and got[5] is norm
    # without the switch: today's torch layers
    monkeypatch.setattr(m, "_native_training", lambda *a: False)
    out = m(inst, anchor, inst, table, metas, residual=res, norm=norm)
    assert len(calls) == 1 and len(ran) == 3 and out.shape == (1, 3, 128)


def test_sparse_block_routing_conditions():
    kw = dict(pc_range=[-5.0, -5.0, -2.5, 5.0, 5.0, 2.5], grid_size=[2.0, 2.0, 1.0], kernel_size=3)
    norm = nn.LayerNorm(128)
    multi = SparseConv3D(128, 128, use_out_proj=True, use_multi_layer=True, **kw)
    single = SparseConv3D(128, 128, use_out_proj=True, **kw)
    assert not multi._tail_training(norm) and not single._tail_training(norm)
    for m in (multi, single):
        m.native_training = True
    assert not multi._tail_training(norm) and not single._tail_training(norm)          # the stages' switch alone: today's route
    for m in (multi, single):
        m.native_tail_training = True
        assert m._tail_training(norm) and m._tail_training(None) and m._tail_training((norm.weight, norm.bias))
        assert not m._tail_training(nn.LayerNorm(128, eps=1e-6)) and not m._tail_training(nn.Identity())
    assert not SparseConv3D(128, 128, use_out_proj=False, **kw)._tail_training(norm)
    narrow = SparseConv3D(64, 64, use_out_proj=True, **kw)
    narrow.native_tail_training = True
    assert not narrow._tail_training(nn.LayerNorm(64))
    nobias = SparseConv3D(128, 128, use_out_proj=True, **kw)
    nobias.native_tail_training = True
    nobias.output_proj = nn.Linear(128, 128, bias=False)
    assert not nobias._tail_training(norm)
    # the tail alone does nothing: a call on CPU tensors, or with native_training off, is not the training route
    x, anchor = torch.zeros(1, 3, 128, requires_grad=True), torch.zeros(1, 3, 11)
    assert single._native_training(x, anchor, None, norm) is False
    single.native_training = False
    assert single._native_training(_gpu(torch.zeros(1, 3, 128), True), anchor, None, norm) is False


def test_encoder_step_routing():
    ask = GaussianOccEncoder._step_folds_training
    x = torch.zeros(1, 3, 128)
    norm = nn.LayerNorm(128)
    ffn = AsymmetricFFN(in_channels=128, pre_norm=dict(type="LN"), embed_dims=128, feedforward_channels=512, ffn_drop=0.1)
    args = (x, x, x, None, x, norm)
    assert ask("ffn", ffn, *args) is False                    # no native_training: the ops one by one
    ffn.native_training = True
    assert ask("ffn", ffn, *args) is False                    # CPU tensors
    g = _gpu(torch.zeros(1, 3, 128))
    ffn.layers[0][0].weight = nn.Parameter(_gpu(torch.zeros(512, 128)))
    gargs = (g, g, g, None, g, norm)
    assert ask("ffn", ffn, *gargs) is True
    ffn.dropout_layer = nn.Dropout(0.2)
    assert ask("ffn", ffn.train(), *gargs) is False and ask("ffn", ffn.eval(), *gargs) is True
    ffn.dropout_layer = nn.Identity()
    assert ask("ffn", ffn, g, g, g, None, g, nn.LayerNorm(128, eps=1e-6)) is False
    assert ask("deformable", _deformable(), *gargs) is False and ask("spconv", nn.Identity(), *gargs) is False
