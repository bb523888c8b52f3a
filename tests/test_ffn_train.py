"""The feed-forward block's training step without a GPU: the restatement with masks against torch's own modules in float64,
the kink filter's survivor count, the refusals of the three entry points (which come before any HIP call), the size query,
and the drop-in module's ``native_training`` switch."""
import ctypes
import inspect

import pytest
import torch
import torch.nn as nn

import ffn_ref as ref
import ffn_train_ref as tr
from gaussianformer_amd import _lib
from gaussianformer_amd.ffn import AsymmetricFFN, FFNBlockFunction, ffn_block_autograd, train_sizes
from row_judge import host_table

CPU = torch.device("cpu")
FAMILY_ARGS = {"base": (256, True, True), "prob": (128, False, False)}    # Cin, pre_norm, identity_fc


def _module64(name, sd):
    m = AsymmetricFFN(**ref.FAMILIES[name]).double()
    m.load_state_dict(ref.module_state(sd), strict=True)
    return m


@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_restatement_with_masks_equals_the_module_in_train_mode(name):
    """The module's torch layers in train mode, float64, draw their two masks from the generator; the same masks, drawn first
    by the same ``nn.Dropout`` on ones, go into the restatement.  Then the post norm on ``+ residual``."""
    cin, pre, ident = FAMILY_ARGS[name]
    sd = ref.fixed_weights(cin, pre, ident, seed=1, dtype=torch.float64)
    m = _module64(name, sd).train()
    n, p = 37, 0.1
    x = ref.fixed_input(n, cin, 5).double()
    res = ref.fixed_input(n, 128, 6).double()
    drop = nn.Dropout(p)
    torch.manual_seed(11)
    keep_hidden = drop(torch.ones(n, 512, dtype=torch.float64)) != 0
    keep_out = drop(torch.ones(n, 128, dtype=torch.float64)) != 0
    assert 0 < int((~keep_hidden).sum()) < n * 512 and 0 < int((~keep_out).sum()) < n * 128
    torch.manual_seed(11)
    with torch.no_grad():
        want = m(x)
        got = tr.ffn_train_ref(x, sd, None, keep_hidden, 1 / (1 - p), keep_out, 1 / (1 - p), norm=False)
        assert (got - want).abs().max() <= 1e-12 * want.abs().max()
        norm = nn.LayerNorm(128).double()
        norm.load_state_dict({"weight": sd["norm.weight"], "bias": sd["norm.bias"]})
        got = tr.ffn_train_ref(x, sd, res, keep_hidden.to(torch.uint8), 1 / (1 - p), keep_out.to(torch.uint8), 1 / (1 - p))
        assert (got - norm(want + res)).abs().max() <= 1e-12
        # without masks it is ffn_ref
        assert torch.equal(tr.ffn_train_ref(x, sd, res), ref.ffn_ref(x, sd, res))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_the_kink_filter_keeps_most_candidates(name, seed):
    cin, pre, ident = FAMILY_ARGS[name]
    x, keep, _ = tr.candidates(cin, pre, ident, True, seed)
    print(f"{name} seed {seed}: {int(keep.sum())} of {x.shape[0]} candidates survive")
    assert x.shape[0] == 1400 and int(keep.sum()) >= 1300


def test_masks_are_seeded_and_do_not_depend_on_n():
    kh, ko, scale = tr.masks(64, 0.1, 3)
    kh2, ko2, _ = tr.masks(32, 0.1, 3)
    assert kh.dtype == torch.uint8 and kh.shape == (64, 512) and ko.shape == (64, 128) and abs(scale - 1 / 0.9) < 1e-15
    assert torch.equal(kh[:32], kh2) and torch.equal(ko[:32], ko2) and 0 < int(kh.sum()) < kh.numel()


# ---- the entry points on host memory: refused before any HIP call ---------------------------------------------------------------

def _buf():
    buf = torch.zeros(1 << 16)
    assert buf.data_ptr() % 16 == 0
    return buf


def _table(buf, drop=(), misalign=None):
    return host_table(buf, 10, drop, misalign)


def _fwd(n=4, cin=256, f=512, e=128, drop=(), misalign=None, keep_hidden=True, scale_hidden=1.0, keep_out=True, scale_out=1.0,
         saved=0, saved_bytes=None, x=0, out=0):
    """``gf_ffn_forward_train`` through ``_lib.call``; ``saved`` / ``x`` / ``out``: a byte offset into the host buffer, ``None``: NULL."""
    buf = _buf()
    at = lambda off: None if off is None else buf.data_ptr() + off
    need = train_sizes(max(n, 0), cin if cin in (128, 256) else 256)[0]
    _lib.call("gf_ffn_forward_train", CPU, n, cin, f, e, at(x), _table(buf, drop, misalign), None, buf if keep_hidden else None, scale_hidden,
              buf if keep_out else None, scale_out, at(out), at(saved), need if saved_bytes is None else saved_bytes)


def _bwd(n=4, cin=256, f=512, e=128, drop=(), misalign=None, gdrop=(), gmisalign=None, keep_hidden=True, scale_hidden=1.0, keep_out=True,
         scale_out=1.0, saved=0, work=0, work_bytes=None, grad_out=0, grad_x=0, grad_res=None, null_grads=False):
    buf = _buf()
    at = lambda off: None if off is None else buf.data_ptr() + off
    need = train_sizes(max(n, 0), cin if cin in (128, 256) else 256)[1]
    _lib.call("gf_ffn_backward", CPU, n, cin, f, e, buf, _table(buf, drop, misalign), buf if keep_hidden else None, scale_hidden,
              buf if keep_out else None, scale_out, at(saved), at(grad_out), at(grad_x), at(grad_res),
              None if null_grads else _table(buf, gdrop, gmisalign), at(work), need if work_bytes is None else work_bytes)


@pytest.mark.parametrize("entry, run", [("gf_ffn_forward_train", _fwd), ("gf_ffn_backward", _bwd)])
def test_what_the_plain_forward_refuses(entry, run):
    fail = entry + r" failed \(code -1\): " + entry + ": "
    for kwargs, message in ((dict(e=256), r"E = 256: only embed_dims = 128"),
                            (dict(f=1024), r"F = 1024: only feedforward_channels = 512"),
                            (dict(cin=192), r"Cin = 192: only in_channels = 128 or 256"),
                            (dict(n=-1), r"n = -1 is negative"),
                            (dict(drop=(1,)), r"a half-present pair: pre_norm.bias is null and pre_norm.weight is not"),
                            (dict(drop=(8,)), r"a half-present pair: norm.weight is null and norm.bias is not"),
                            (dict(drop=(4,)), r"layers.1.weight is missing"),
                            (dict(drop=(3,)), r"layers.0.0.bias is missing"),
                            (dict(misalign=6), r"identity_fc.weight is not 16-byte aligned")):
        with pytest.raises(RuntimeError, match=fail + message):
            run(**kwargs)


def test_forward_train_refusals():
    fail = r"gf_ffn_forward_train failed \(code -1\): gf_ffn_forward_train: "
    with pytest.raises(RuntimeError, match=fail + "null params"):
        _lib.call("gf_ffn_forward_train", CPU, 4, 256, 512, 128, None, None, None, None, 1.0, None, 1.0, None, None, 0)
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match=fail + "scale_hidden = .* is not a positive finite number"):
            _fwd(scale_hidden=scale)
        with pytest.raises(RuntimeError, match=fail + "scale_out = .* is not a positive finite number"):
            _fwd(scale_out=scale)
    with pytest.raises(RuntimeError, match=fail + "x is not 16-byte aligned"):
        _fwd(x=4)
    with pytest.raises(RuntimeError, match=fail + "out is not 16-byte aligned"):
        _fwd(out=8)
    with pytest.raises(RuntimeError, match=fail + "saved is not 16-byte aligned"):
        _fwd(saved=4)
    with pytest.raises(RuntimeError, match=fail + "saved is null"):
        _fwd(saved=None)
    with pytest.raises(RuntimeError, match=fail + "null pointer"):
        _fwd(out=None)
    need = train_sizes(4, 256)[0]
    with pytest.raises(RuntimeError, match=rf"gf_ffn_forward_train failed \(code -2\): gf_ffn_forward_train: saved of {need - 1} bytes, {need} needed"):
        _fwd(saved_bytes=need - 1)
    # a scale is ignored where its mask is NULL; n == 0 is GF_OK without a launch, masks at any alignment
    _fwd(n=0, keep_hidden=False, scale_hidden=float("nan"), keep_out=False, scale_out=-1.0)
    _fwd(n=0, saved=None, drop=(0, 1, 6, 7, 8, 9))


def test_backward_refusals():
    fail = r"gf_ffn_backward failed \(code -1\): gf_ffn_backward: "
    with pytest.raises(RuntimeError, match=fail + "scale_hidden = 0 is not a positive finite number"):
        _bwd(scale_hidden=0.0)
    with pytest.raises(RuntimeError, match=fail + "scale_out = .* is not a positive finite number"):
        _bwd(scale_out=float("inf"))
    with pytest.raises(RuntimeError, match=fail + "null grad_params"):
        _bwd(null_grads=True)
    with pytest.raises(RuntimeError, match=fail + "the gradient of layers.1.bias is null"):
        _bwd(gdrop=(5,))
    with pytest.raises(RuntimeError, match=fail + "the gradient of norm.weight is null"):
        _bwd(gdrop=(8, 9))
    with pytest.raises(RuntimeError, match=fail + "the gradient of pre_norm.weight is not 16-byte aligned"):
        _bwd(gmisalign=0)
    with pytest.raises(RuntimeError, match=fail + "grad_out is not 16-byte aligned"):
        _bwd(grad_out=4)
    with pytest.raises(RuntimeError, match=fail + "grad_x is not 16-byte aligned"):
        _bwd(grad_x=4)
    with pytest.raises(RuntimeError, match=fail + "grad_residual is not 16-byte aligned"):
        _bwd(grad_res=12)
    with pytest.raises(RuntimeError, match=fail + "saved is not 16-byte aligned"):
        _bwd(saved=8)
    with pytest.raises(RuntimeError, match=fail + "workspace is not 16-byte aligned"):
        _bwd(work=4)
    with pytest.raises(RuntimeError, match=fail + "saved is null"):
        _bwd(saved=None)
    with pytest.raises(RuntimeError, match=fail + "workspace is null"):
        _bwd(work=None)
    with pytest.raises(RuntimeError, match=fail + "null pointer"):
        _bwd(grad_x=None)
    need = train_sizes(4, 256)[1]
    with pytest.raises(RuntimeError, match=rf"gf_ffn_backward failed \(code -2\): gf_ffn_backward: workspace of {need - 1} bytes, {need} needed"):
        _bwd(work_bytes=need - 1)
    # the gradient of an absent parameter may be NULL: the refusal that follows is the next one
    with pytest.raises(RuntimeError, match=fail + "workspace is null"):
        _bwd(drop=(0, 1, 6, 7), gdrop=(0, 1, 6, 7), work=None)


def test_train_sizes():
    lib = _lib.load()
    for cin in (128, 256):
        assert train_sizes(0, cin) == (0, 0)
        last = (0, 0)
        for n in sorted({1, 31, 32, 33, 128, 129, 1000, _lib.GF_FFN_WGRAD_ROWS, _lib.GF_FFN_WGRAD_ROWS + 1, _lib.GF_FFN_CHUNK_ROWS,
                         _lib.GF_FFN_CHUNK_ROWS + 1, 144000}):
            saved, work = train_sizes(n, cin)
            assert saved >= 528 * n and saved <= 640 * n + 4096, (n, saved)       # y, two (mean, rstd): no [n, 512] array
            assert saved >= last[0] and work >= last[1] and work > 0 and saved % 16 == 0 and work % 16 == 0
            last = (saved, work)
    # the per-row intermediates are one chunk's: beyond a chunk the workspace grows by the partials only
    c = _lib.GF_FFN_CHUNK_ROWS
    assert train_sizes(4 * c, 256)[1] - train_sizes(c, 256)[1] < train_sizes(c, 256)[1]
    out = ctypes.c_size_t(0)
    for args, message in (((-1, 256, ctypes.addressof(out), ctypes.addressof(out)), b"n = -1 is negative"),
                          ((4, 192, ctypes.addressof(out), ctypes.addressof(out)), b"Cin = 192"),
                          ((4, 256, None, ctypes.addressof(out)), b"null pointer")):
        assert lib.gf_ffn_train_sizes(*args) == -1 and message in lib.gf_last_error()


def test_constants_and_build_list():
    from gaussianformer_amd import build as B
    assert (_lib.GF_FFN_WGRAD_ROWS, _lib.GF_FFN_CHUNK_ROWS) == (512, 32768)
    assert _lib.GF_FFN_CHUNK_ROWS % _lib.GF_FFN_WGRAD_ROWS == 0 and _lib.GF_FFN_WGRAD_ROWS % 128 == 0
    assert "ffn_train.hip" in B.SOURCES and "ffn_train.hip" not in B.FP_ATOMICS and "gf_ffn.hpp" in B.HEADERS
    for name in ("gf_ffn_train_sizes", "gf_ffn_forward_train", "gf_ffn_backward"):
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["gf_ffn_forward_train"][1][-1] is ctypes.c_void_p and _lib.SIGNATURES["gf_ffn_backward"][1][-1] is ctypes.c_void_p
    assert not any(name.endswith("_bytes") for name in _lib.SIGNATURES if name.startswith("gf_ffn"))


# ---- the module's switch ---------------------------------------------------------------------------------------------------------

def test_native_training_is_an_attribute_off_by_default():
    m = AsymmetricFFN(**ref.FAMILIES["base"])
    assert AsymmetricFFN.native_training is False and m.native_training is False
    assert "native_training" not in inspect.signature(AsymmetricFFN.__init__).parameters
    m.native_training = True
    assert not any("native_training" in k for k in m.state_dict())
    assert AsymmetricFFN(**ref.FAMILIES["base"]).native_training is False       # set on the instance, not on the class
    assert issubclass(FFNBlockFunction, torch.autograd.Function)


def test_with_the_switch_set_cpu_tensors_and_other_configurations_take_the_torch_route(monkeypatch):
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    x = ref.fixed_input(9, 256, 3).requires_grad_(True)
    m = AsymmetricFFN(**ref.FAMILIES["base"]).train()
    m.native_training = True
    torch.manual_seed(0)
    a = m(x)
    b = m(x)
    a.sum().backward()
    assert names == [] and not torch.equal(a, b) and x.grad is not None and m.layers[1].weight.grad is not None
    for cfg in (dict(in_channels=256, embed_dims=256, feedforward_channels=1024), dict(ref.FAMILIES["base"], act_cfg=dict(type="GELU")),
                dict(ref.FAMILIES["base"], num_fcs=3), dict(ref.FAMILIES["base"], dropout_layer=dict(type="Dropout", drop_prob=0.2))):
        m = AsymmetricFFN(**cfg).train()
        m.native_training = True
        m(x).sum().backward()
    assert names == []


def test_the_functional_refuses_cpu_tensors_and_bad_arguments():
    m = AsymmetricFFN(**ref.FAMILIES["prob"])
    x = ref.fixed_input(4, 128, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ffn_block_autograd(x.requires_grad_(True), m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ffn_block_autograd(x, m, keep_hidden=torch.ones(4, 512, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"p_hidden = 1.0 is not in \[0, 1\)"):
        ffn_block_autograd(x, m, p_hidden=1.0)
    with pytest.raises(ValueError, match=r"p_out = -0.1 is not in \[0, 1\)"):
        ffn_block_autograd(x, m, p_out=-0.1)
