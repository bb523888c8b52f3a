"""The fused refinement step (gf_refine_mlp_forward, gaussianformer_amd.refine.refine_fused, the modules' ``fused_mlp``) without
a GPU: the ABI and the build lists, what the library refuses before any HIP call, and the host layer's rules."""
import ctypes
import os
import re

import pytest
import torch

import refine_ref
from gaussianformer_amd import _lib
from gaussianformer_amd import refine as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = {1: R.SparseGaussian3DRefinementModule, 2: R.SparseGaussian3DRefinementModuleV2}
NAME = "gf_refine_mlp_forward"


def build(name, embed_dims=128):
    cfg = refine_ref.FAMILIES[name]
    kwargs = {k: v for k, v in cfg.items() if k != "version"}
    return CLASSES[cfg["version"]](embed_dims=embed_dims, phi_activation="sigmoid", xyz_coordinate="cartesian", **kwargs)


def test_abi_is_10_and_declares_the_entry_point():
    header = open(os.path.join(ROOT, "include", "gf_hip.h")).read()
    assert re.search(r"^#define\s+GF_ABI_VERSION\s+10\b", header, flags=re.M)
    assert _lib.GF_ABI_VERSION == 10 and _lib.load().gf_abi_version() == 10
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", header) and NAME in _lib.SIGNATURES
    assert re.search(r"^#define\s+GF_REFINE_MLP_PARAMS\s+15\b", header, flags=re.M) and _lib.GF_REFINE_MLP_PARAMS == 15
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_int] * 8 + [ctypes.c_void_p] * 15
    assert hasattr(_lib.load(), NAME)
    from gaussianformer_amd import build as B
    assert "refine_mlp.hip" in B.SOURCES and "refine_mlp.hip" not in B.FP_ATOMICS and "gf_refine.hpp" in B.HEADERS
    assert len(R.MLP_KEYS) == 15 and list(R.MLP_KEYS) == [k for k in build("solid").state_dict()]


def test_refusals_of_the_library_before_any_hip_call():
    cpu = torch.device("cpu")
    consts = (ctypes.c_double * 11)(-50, -50, -5, 50, 50, 3, 0.08, 0.64, 4, 4, 1)
    c = ctypes.cast(consts, ctypes.c_void_p)
    opa, softmax = _lib.GF_REFINE_OPACITY, _lib.GF_REFINE_SEM_SOFTMAX

    def call(n, E, D, Da, version, flags, Rn, S, consts=c, feat=None, embed=None, anchor=None, params=None, outs=(None,) * 8):
        _lib.call(NAME, cpu, n, E, D, Da, version, flags, Rn, S, consts, feat, embed, anchor, params, None, *outs)

    # what gf_refine_forward refuses, in its words
    with pytest.raises(RuntimeError, match=NAME + r" failed \(code -1\): .*S must be"):
        call(64, 128, 10 + 1 + 33, 44, 1, opa, 3, 33)
    with pytest.raises(RuntimeError, match=r"D must be 10 \+ opacity \+ S"):
        call(64, 128, 28, 28, 1, 0, 3, 17)
    with pytest.raises(RuntimeError, match="R must be in"):
        call(64, 128, 28, 28, 1, opa, 29, 17)
    with pytest.raises(RuntimeError, match="Da is smaller"):
        call(64, 128, 28, 2, 1, opa, 3, 17)
    with pytest.raises(RuntimeError, match="Da is smaller"):
        call(64, 128, 28, 2, 2, opa, 0, 17)
    with pytest.raises(RuntimeError, match="version"):
        call(64, 128, 28, 28, 3, opa, 3, 17)
    with pytest.raises(RuntimeError, match="version"):
        call(-1, 128, 28, 28, 1, opa, 3, 17)
    with pytest.raises(RuntimeError, match="flags"):
        call(64, 128, 28, 28, 1, opa | softmax | _lib.GF_REFINE_SEM_SOFTPLUS, 3, 17)
    with pytest.raises(RuntimeError, match="flags"):
        call(64, 128, 28, 28, 1, opa | 32, 3, 17)
    with pytest.raises(RuntimeError, match="null consts"):
        call(64, 128, 28, 28, 1, opa, 3, 17, consts=None)
    # its own
    for E in (64, 256, 0):
        with pytest.raises(RuntimeError, match=rf"E = {E}: only embed_dims = 128"):
            call(64, E, 28, 28, 1, opa, 3, 17)
    with pytest.raises(RuntimeError, match="null params"):
        call(64, 128, 28, 28, 1, opa, 3, 17)
    # a table of made-up addresses: refused before anything is dereferenced
    fake = [0x1000 + 0x100 * i for i in range(15)]
    for i, key in enumerate(R.MLP_KEYS):
        bad = list(fake)
        bad[i] = None
        keep = (ctypes.c_void_p * 15)(*bad)
        with pytest.raises(RuntimeError, match=rf"params\[{i}\] \({re.escape(key)}\) is null"):
            call(64, 128, 28, 28, 1, opa, 3, 17, params=ctypes.cast(keep, ctypes.c_void_p))
        bad[i] = fake[i] + 8
        keep = (ctypes.c_void_p * 15)(*bad)
        with pytest.raises(RuntimeError, match=rf"params\[{i}\] \({re.escape(key)}\) = 0x{fake[i] + 8:x} is not 16-byte aligned"):
            call(64, 128, 28, 28, 1, opa, 3, 17, params=ctypes.cast(keep, ctypes.c_void_p))
    good = (ctypes.c_void_p * 15)(*fake)
    p = ctypes.cast(good, ctypes.c_void_p)
    addr = lambda v: ctypes.c_void_p(v)
    with pytest.raises(RuntimeError, match="null instance_feature"):
        call(64, 128, 28, 28, 1, opa, 3, 17, params=p, embed=addr(0x4000), anchor=addr(0x5000))
    with pytest.raises(RuntimeError, match="null anchor_embed"):
        call(64, 128, 28, 28, 1, opa, 3, 17, params=p, feat=addr(0x3000), anchor=addr(0x5000))
    with pytest.raises(RuntimeError, match="null anchor"):
        call(64, 128, 28, 28, 1, opa, 3, 17, params=p, feat=addr(0x3000), embed=addr(0x4000))
    with pytest.raises(RuntimeError, match="null anchor"):          # also where the tail reads no anchor column (R = 0)
        call(64, 128, 28, 28, 1, opa, 0, 17, params=p, feat=addr(0x3000), embed=addr(0x4000))
    with pytest.raises(RuntimeError, match="instance_feature = 0x3004 is not 16-byte aligned"):
        call(64, 128, 28, 28, 1, opa, 3, 17, params=p, feat=addr(0x3004), embed=addr(0x4000), anchor=addr(0x5004))
    with pytest.raises(RuntimeError, match="anchor_embed = 0x4008 is not 16-byte aligned"):
        call(64, 128, 28, 28, 1, opa, 3, 17, params=p, feat=addr(0x3000), embed=addr(0x4008), anchor=addr(0x5004))
    with pytest.raises(RuntimeError, match="null pointer"):         # the outputs, as gf_refine_forward
        call(64, 128, 28, 28, 1, opa, 3, 17, params=p, feat=addr(0x3000), embed=addr(0x4000), anchor=addr(0x5004))
    outs6 = tuple(addr(0x6000 + 0x100 * i) for i in range(6)) + (None, None)
    with pytest.raises(RuntimeError, match="null pointer"):         # version 2 writes original_means and delta_means too
        call(64, 128, 28, 28, 2, opa, 0, 17, params=p, feat=addr(0x3000), embed=addr(0x4000), anchor=addr(0x5004), outs=outs6)
    # nothing to do: no pointer is looked at
    call(0, 128, 28, 28, 1, opa, 3, 17)
    call(0, 128, 28, 28, 2, opa, 0, 17)


@pytest.mark.parametrize("name", list(refine_ref.FAMILIES))
def test_the_attribute_is_off_and_outside_the_state_dict(name):
    module = build(name, embed_dims=32)
    assert module.fused_mlp is False and type(module).fused_mlp is False
    keys = list(module.state_dict())
    module.fused_mlp = True
    assert list(module.state_dict()) == keys == list(R.MLP_KEYS)
    assert "fused_mlp" not in keys and "fused_mlp" not in dict(module.named_buffers()) and "fused_mlp" not in dict(module.named_parameters())
    fresh = build(name, embed_dims=32)
    fresh.load_state_dict(module.state_dict(), strict=True)
    assert fresh.fused_mlp is False
    # not a constructor key: it falls into **kwargs, as any other unknown key does
    m = CLASSES[1](embed_dims=32, pc_range=[-1.0] * 3 + [1.0] * 3, scale_range=[0.1, 0.2], refine_manual=[], fused_mlp=True)
    assert m.fused_mlp is False


@pytest.mark.parametrize("name", list(refine_ref.FAMILIES))
def test_a_fused_module_has_no_cpu_fallback(name):
    z = torch.zeros
    for E in (32, 128):
        module = build(name, embed_dims=E)
        module.fused_mlp = True
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            module(z(2, 5, E), z(2, 5, 28), z(2, 5, E))
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            module(z(2, 5, E), z(2, 5, 28), z(2, 5, E))


def test_refine_fused_is_forward_only():
    module = build("solid")
    z = torch.zeros
    with pytest.raises(RuntimeError, match="refine_fused computes no gradients"):
        R.refine_fused(z(5, 128), z(5, 28), z(5, 128), module, module._cfg)                       # the module's parameters require grad
    state = module.state_dict()
    for k in range(3):
        args = [z(5, 128), z(5, 28), z(5, 128)]
        args[k].requires_grad_(True)
        with pytest.raises(RuntimeError, match="refine_fused computes no gradients"):
            R.refine_fused(args[0], args[1], args[2], state, module._cfg)
    # where nothing would be recorded the call goes on, to the refusal of CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.refine_fused(z(5, 128), z(5, 28), z(5, 128), state, module._cfg)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        R.refine_fused(z(5, 128).requires_grad_(True), z(5, 28), z(5, 128), module, module._cfg)
