"""The refinement modules' native training step (gf_refine_mlp_train_sizes, gf_refine_mlp_forward_train,
gf_refine_mlp_backward, gaussianformer_amd.refine.refine_fused_autograd, the modules' ``native_training``) without a GPU: the
ABI and the build lists, the size query, what the library refuses before any HIP call, the host layer's rules, and the cap on
what the GPU tests' kink filter may reject."""
import ctypes
import os
import re

import pytest
import torch

import refine_mlp_train_ref as T
import refine_ref
from gaussianformer_amd import _lib
from gaussianformer_amd import refine as R
from refine_ref import VARIANTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = {1: R.SparseGaussian3DRefinementModule, 2: R.SparseGaussian3DRefinementModuleV2}
SIZES, FORWARD, BACKWARD = "gf_refine_mlp_train_sizes", "gf_refine_mlp_forward_train", "gf_refine_mlp_backward"


def build(name, embed_dims=128):
    cfg = refine_ref.FAMILIES[name]
    kwargs = {k: v for k, v in cfg.items() if k != "version"}
    return CLASSES[cfg["version"]](embed_dims=embed_dims, phi_activation="sigmoid", xyz_coordinate="cartesian", **kwargs)


def test_the_abi_declares_the_three_entry_points_and_the_constants():
    header = open(os.path.join(ROOT, "include", "gf_hip.h")).read()
    for name in (SIZES, FORWARD, BACKWARD):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    for name in ("GF_REFINE_MLP_WGRAD_ROWS", "GF_REFINE_MLP_CHUNK_ROWS"):
        m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", header, flags=re.M)
        assert m and int(m.group(1)) == getattr(_lib, name)
    assert _lib.GF_REFINE_MLP_CHUNK_ROWS % _lib.GF_REFINE_MLP_WGRAD_ROWS == 0 and _lib.GF_REFINE_MLP_WGRAD_ROWS % 128 == 0
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES[SIZES] == (i, [i] * 3 + [vp] * 2)
    assert _lib.SIGNATURES[FORWARD] == (i, [i] * 8 + [vp] * 14 + [vp, sz, vp])
    assert _lib.SIGNATURES[BACKWARD] == (i, [i] * 8 + [vp] * 18 + [vp, sz, vp])
    assert _lib.GF_ABI_VERSION == 10 and _lib.load().gf_abi_version() == 10
    from gaussianformer_amd import build as B
    for src in ("refine.hip", "refine_mlp.hip", "refine_mlp_train.hip"):
        assert src in B.SOURCES and src not in B.FP_ATOMICS


def test_the_size_query():
    assert R.train_sizes(0, 28, 28) == (0, 0)
    last = (0, 0)
    B, C = _lib.GF_REFINE_MLP_WGRAD_ROWS, _lib.GF_REFINE_MLP_CHUNK_ROWS
    for n in (1, 2, 127, 128, 129, B - 1, B, B + 1, 1000, C - 1, C, C + 1, C + 582, 144000):
        now = R.train_sizes(n, 28, 28)
        assert now[0] >= last[0] and now[1] >= last[1] and now[0] > 0 and now[1] > 0, (n, now, last)
        assert now[0] % 16 == 0 and now[1] % 16 == 0
        last = now
    # what is saved: four rows of 128, two (mean, rstd), 64 before Scale, D of o, as floats per row (each region rounded up)
    assert 4 * (4 * 128 + 4 + 64 + 28) * 144000 <= R.train_sizes(144000, 28, 28)[0] <= 4 * (4 * 128 + 4 + 64 + 28) * 144000 + 4 * 256
    # past one chunk the workspace grows by the partial sums only: far less than a chunk's rows
    assert R.train_sizes(2 * C, 28, 28)[1] < 1.5 * R.train_sizes(C, 28, 28)[1]
    assert R.train_sizes(1000, 43, 43)[0] > R.train_sizes(1000, 10, 10)[0]
    saved, work = ctypes.c_size_t(0), ctypes.c_size_t(0)
    fn = _lib.load().gf_refine_mlp_train_sizes
    s, w = ctypes.addressof(saved), ctypes.addressof(work)
    for args, words in (((-1, 28, 28, s, w), "n = -1"), ((5, 9, 28, s, w), "D = 9"), ((5, 44, 44, s, w), "D = 44"),
                        ((5, 28, 28, None, w), "null pointer"), ((5, 28, 28, s, None), "null pointer")):
        assert fn(*args) == -1
        assert words in _lib.load().gf_last_error().decode()
    with pytest.raises(RuntimeError, match=SIZES + r" failed \(code -1\): .*D = 44"):
        R.train_sizes(5, 44, 44)


def test_refusals_of_the_launching_entry_points_before_any_hip_call():
    cpu = torch.device("cpu")
    consts = (ctypes.c_double * 11)(-50, -50, -5, 50, 50, 3, 0.08, 0.64, 4, 4, 1)
    c = ctypes.cast(consts, ctypes.c_void_p)
    opa = _lib.GF_REFINE_OPACITY
    addr = lambda v: ctypes.c_void_p(v)
    fake = [0x1000 + 0x100 * i for i in range(15)]
    good = (ctypes.c_void_p * 15)(*fake)
    p = ctypes.cast(good, ctypes.c_void_p)
    gfake = (ctypes.c_void_p * 15)(*[0x9000 + 0x100 * i for i in range(15)])
    gp = ctypes.cast(gfake, ctypes.c_void_p)
    outs = tuple(addr(0x6000 + 0x100 * i) for i in range(8))
    big = 1 << 40

    def forward(n=64, E=128, D=28, Da=28, version=1, flags=opa, Rn=3, S=17, consts=c, feat=addr(0x3000), embed=addr(0x4000),
                anchor=addr(0x5004), params=p, outs=outs, saved=addr(0x7000), saved_bytes=big):
        _lib.call(FORWARD, cpu, n, E, D, Da, version, flags, Rn, S, consts, feat, embed, anchor, params, None, *outs, saved, saved_bytes)

    def backward(n=64, E=128, D=28, Da=28, version=1, flags=opa, Rn=3, S=17, consts=c, feat=addr(0x3000), embed=addr(0x4000),
                 anchor=addr(0x5004), params=p, saved=addr(0x7000), grads=(None,) * 8, grad_x=addr(0x8000), grad_anchor=addr(0x8804),
                 grad_mlp_out=None, grad_params=gp, work=addr(0xa000), work_bytes=big):
        _lib.call(BACKWARD, cpu, n, E, D, Da, version, flags, Rn, S, consts, feat, embed, anchor, params, saved, *grads, grad_x,
                  grad_anchor, grad_mlp_out, grad_params, work, work_bytes)

    for name, call in ((FORWARD, forward), (BACKWARD, backward)):
        # everything gf_refine_mlp_forward refuses, in its words, under the name of the entry point called
        with pytest.raises(RuntimeError, match=name + r" failed \(code -1\): " + name + ": S must be"):
            call(D=44, Da=44, S=33)
        with pytest.raises(RuntimeError, match=r"D must be 10 \+ opacity \+ S"):
            call(flags=0)
        with pytest.raises(RuntimeError, match="R must be in"):
            call(Rn=29)
        with pytest.raises(RuntimeError, match="Da is smaller"):
            call(Da=2)
        with pytest.raises(RuntimeError, match="version"):
            call(version=3)
        with pytest.raises(RuntimeError, match="version"):
            call(n=-1)
        with pytest.raises(RuntimeError, match="flags"):
            call(flags=opa | 32)
        with pytest.raises(RuntimeError, match="null consts"):
            call(consts=None)
        for E in (64, 256):
            with pytest.raises(RuntimeError, match=rf"E = {E}: only embed_dims = 128"):
                call(E=E)
        with pytest.raises(RuntimeError, match="null params"):
            call(params=None)
        for i, key in enumerate(R.MLP_KEYS):
            bad = list(fake)
            bad[i] = None
            keep = (ctypes.c_void_p * 15)(*bad)
            with pytest.raises(RuntimeError, match=rf"params\[{i}\] \({re.escape(key)}\) is null"):
                call(params=ctypes.cast(keep, ctypes.c_void_p))
            bad[i] = fake[i] + 8
            keep = (ctypes.c_void_p * 15)(*bad)
            with pytest.raises(RuntimeError, match=rf"params\[{i}\] \({re.escape(key)}\) = 0x{fake[i] + 8:x} is not 16-byte aligned"):
                call(params=ctypes.cast(keep, ctypes.c_void_p))
        with pytest.raises(RuntimeError, match="null instance_feature"):
            call(feat=None)
        with pytest.raises(RuntimeError, match="null anchor_embed"):
            call(embed=None)
        with pytest.raises(RuntimeError, match="null anchor"):
            call(anchor=None)
        with pytest.raises(RuntimeError, match="instance_feature = 0x3004 is not 16-byte aligned"):
            call(feat=addr(0x3004))
        with pytest.raises(RuntimeError, match="anchor_embed = 0x4008 is not 16-byte aligned"):
            call(embed=addr(0x4008))
        # the saved region
        with pytest.raises(RuntimeError, match="saved is null"):
            call(saved=None)
        with pytest.raises(RuntimeError, match="saved = 0x7008 is not 16-byte aligned"):
            call(saved=addr(0x7008))

    # the forward's own
    with pytest.raises(RuntimeError, match="null pointer"):
        forward(outs=(None,) * 8)
    with pytest.raises(RuntimeError, match="null pointer"):
        forward(version=2, Rn=0, outs=outs[:6] + (None, None))
    need = R.train_sizes(64, 28, 28)
    with pytest.raises(RuntimeError, match=FORWARD + rf" failed \(code -2\): .*saved of {need[0] - 1} bytes, {need[0]} needed"):
        forward(saved_bytes=need[0] - 1)
    forward(n=0, params=None, feat=None, embed=None, anchor=None, outs=(None,) * 8, saved=None, saved_bytes=0)

    # the backward's own
    with pytest.raises(RuntimeError, match="null grad_params"):
        backward(grad_params=None)
    for i, key in enumerate(R.MLP_KEYS):
        bad = [0x9000 + 0x100 * k for k in range(15)]
        bad[i] = None
        keep = (ctypes.c_void_p * 15)(*bad)
        with pytest.raises(RuntimeError, match=rf"grad_params\[{i}\] \(the gradient of {re.escape(key)}\) is null"):
            backward(grad_params=ctypes.cast(keep, ctypes.c_void_p))
        with pytest.raises(RuntimeError, match=rf"grad_params\[{i}\]"):       # also when there is nothing else to do
            backward(n=0, grad_params=ctypes.cast(keep, ctypes.c_void_p))
    with pytest.raises(RuntimeError, match="workspace is null"):
        backward(work=None)
    with pytest.raises(RuntimeError, match="workspace = 0xa004 is not 16-byte aligned"):
        backward(work=addr(0xa004))
    with pytest.raises(RuntimeError, match="grad_x is null"):
        backward(grad_x=None)
    with pytest.raises(RuntimeError, match="grad_x = 0x8008 is not 16-byte aligned"):
        backward(grad_x=addr(0x8008))
    with pytest.raises(RuntimeError, match="grad_anchor is null"):
        backward(grad_anchor=None)
    with pytest.raises(RuntimeError, match=BACKWARD + rf" failed \(code -2\): .*workspace of {need[1] - 1} bytes, {need[1]} needed"):
        backward(work_bytes=need[1] - 1)


@pytest.mark.parametrize("name", list(refine_ref.FAMILIES))
def test_the_attribute_is_off_and_outside_the_state_dict(name):
    module = build(name, embed_dims=32)
    assert module.native_training is False and type(module).native_training is False
    keys = list(module.state_dict())
    module.native_training = True
    assert list(module.state_dict()) == keys == list(R.MLP_KEYS)
    for table in (keys, dict(module.named_buffers()), dict(module.named_parameters())):
        assert "native_training" not in table
    fresh = build(name, embed_dims=32)
    fresh.load_state_dict(module.state_dict(), strict=True)
    assert fresh.native_training is False
    # not a constructor key: it falls into **kwargs, as any other unknown key does
    m = CLASSES[1](embed_dims=32, pc_range=[-1.0] * 3 + [1.0] * 3, scale_range=[0.1, 0.2], refine_manual=[], native_training=True)
    assert m.native_training is False and m.fused_mlp is False


@pytest.mark.parametrize("name", list(refine_ref.FAMILIES))
def test_no_cpu_fallback(name):
    z = torch.zeros
    module = build(name)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.refine_fused_autograd(z(5, 128), z(5, 28), z(5, 128), module, module._cfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.refine_fused_autograd(z(5, 128).requires_grad_(True), z(5, 28), z(5, 128), module.state_dict(), module._cfg)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        R.refine_fused_autograd(z(5, 128), z(5, 28), z(5, 128), module, module._cfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.RefineFusedFunction.apply(z(5, 128), z(5, 28), z(5, 128), module._cfg, *[module.state_dict()[k] for k in R.MLP_KEYS])
    for E in (32, 128):      # the modules: CPU tensors take the default route, which refuses them
        module = build(name, embed_dims=E)
        module.native_training = True
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            module(z(2, 5, E), z(2, 5, 28), z(2, 5, E))
    # refine_fused keeps refusing gradients, in its words
    with pytest.raises(RuntimeError, match="refine_fused computes no gradients"):
        R.refine_fused(z(5, 128), z(5, 28), z(5, 128), build(name), module._cfg)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_kink_filter_keeps_at_least_1300_of_1400(variant):
    """A condition that keeps the filter from hiding a failure, not a tolerance.  Measured with exactly these weights and
    inputs: 1 355 - 1 374 of the 1 400 candidates survive (1.9 - 3.2 % rejected)."""
    keep = T.candidates(variant)[4]
    print(f"{variant}: {int(keep.sum())} of {keep.numel()} candidates survive ({100 * (1 - float(keep.float().mean())):.1f} % rejected)")
    assert keep.numel() == T.CANDIDATES == 1400 and int(keep.sum()) >= 1300


def test_kinds():
    assert [T.kind(k) for k in R.MLP_KEYS] == ["square weight", "Linear bias"] * 2 + ["LN weight", "LN bias"] + \
        ["square weight", "Linear bias"] * 2 + ["LN weight", "LN bias"] + ["last weight", "Linear bias", "scale"]
