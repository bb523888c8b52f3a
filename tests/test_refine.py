"""The refinement step without a GPU: the torch restatement (tests/refine_ref.py) against the reference's own recorded
results (tests/golden/refine.npz, tools/make_golden_refine.py), the drop-in modules' parameters against the reference's,
what the host layer and the library refuse, and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import refine_ref
from gaussianformer_amd import _lib
from gaussianformer_amd import refine as R
from row_judge import bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = {1: R.SparseGaussian3DRefinementModule, 2: R.SparseGaussian3DRefinementModuleV2}


def fixture(name):
    with np.load(os.path.join(ROOT, "tests", "golden", "refine.npz")) as z:
        return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + ".")}


def build(name, embed_dims=32):
    cfg = refine_ref.FAMILIES[name]
    kwargs = {k: v for k, v in cfg.items() if k != "version"}
    return CLASSES[cfg["version"]](embed_dims=embed_dims, phi_activation="sigmoid", xyz_coordinate="cartesian", **kwargs)


@pytest.mark.parametrize("name", list(refine_ref.FAMILIES))
def test_restatement_reproduces_the_reference(name):
    """refine_ref in float32 on the CPU against every recorded output and gradient of the reference's module.  Bound: 4 eps32
    at the tensor's largest magnitude -- the restatement performs the reference's operations in its order, so only the order
    in which autograd adds a tensor's several gradients could differ.  Measured: every output and gradient of the three
    families is bit-equal (distance 0.0) on the torch build the fixture was recorded with."""
    fx = fixture(name)
    cfg = refine_ref.FAMILIES[name]
    state = {k[6:]: torch.from_numpy(v).requires_grad_(v.dtype == np.float32) for k, v in fx.items() if k.startswith("state.")}
    feat, anchor, embed = (torch.from_numpy(fx[k]).requires_grad_(True) for k in ("instance_feature", "anchor", "anchor_embed"))
    outs = refine_ref.refine_module(state, feat, anchor, embed, cfg)
    assert sorted(outs) == sorted(k[4:] for k in fx if k.startswith("out."))
    refine_ref.weighted_sum(outs, refine_ref.fixed_weights(outs)).backward()
    got = {"out." + k: v.detach() for k, v in outs.items()}
    got.update({"grad.instance_feature": feat.grad, "grad.anchor": anchor.grad})
    got.update({"grad.param." + k: v.grad for k, v in state.items()})
    assert torch.equal(embed.grad, feat.grad)
    checked = 0
    for k, v in got.items():
        want = torch.from_numpy(fx[k])
        assert v.shape == want.shape, k
        if want.numel() == 0:
            continue
        dist, limit = float((v - want).abs().max()), bound(0.0, want)      # 4 eps32 max|want|: the same formula, no yardstick
        print(f"{name} {k}: distance {dist:.3g} bound {limit:.3g}")
        assert dist <= limit, (k, dist, limit)
        checked += 1
    assert checked == len([k for k in fx if k.startswith(("out.", "grad.")) and fx[k].size])


@pytest.mark.parametrize("name", list(refine_ref.FAMILIES))
def test_state_dict_parity(name):
    fx = fixture(name)
    module = build(name)
    keys = [str(k) for k in fx["keys"]]
    sd = module.state_dict()
    assert list(sd.keys()) == keys
    assert [k for k, _ in module.named_parameters()] == keys       # no buffer is persistent, as in the reference
    for k in keys:
        assert tuple(sd[k].shape) == fx["state." + k].shape, k
    assert sd["layers.11.scale"].shape == (module.output_dim,)
    module.load_state_dict({k: torch.from_numpy(fx["state." + k]) for k in keys}, strict=True)
    if refine_ref.FAMILIES[name]["version"] == 2:
        assert "unit_xyz" in dict(module.named_buffers()) and module.unit_xyz.dtype == torch.float32


def test_refusals_of_the_host_layer():
    base = dict(embed_dims=16, pc_range=[-50.0, -50.0, -5.0, 50.0, 50.0, 3.0], scale_range=[0.08, 0.64])
    with pytest.raises(NotImplementedError, match=r"refine_module\.py:106-108"):
        R.SparseGaussian3DRefinementModule(refine_manual=[0, 1, 2], scale_activation="identity", **base)
    with pytest.raises(NotImplementedError, match=r"refine_module_v2\.py:88-90"):
        R.SparseGaussian3DRefinementModuleV2(unit_xyz=[4.0, 4.0, 1.0], scale_activation="identity", **base)
    with pytest.raises(ValueError, match="prefix"):
        R.SparseGaussian3DRefinementModule(refine_manual=[0, 2], **base)
    with pytest.raises(ValueError, match="prefix"):
        R.refine_config(1, base["pc_range"], base["scale_range"], refine_manual=[1])
    module = build("solid")
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        module(z(2, 5, 32), z(2, 5, 28), z(2, 5, 32))
    cfg = R.refine_config(2, base["pc_range"], base["scale_range"], [4.0, 4.0, 1.0], semantic_dim=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.RefineFunction.apply(z(5, 11), z(5, 11), cfg)


def test_refusals_of_the_library_before_any_hip_call():
    cpu = torch.device("cpu")
    consts = (ctypes.c_double * 11)(-50, -50, -5, 50, 50, 3, 0.08, 0.64, 4, 4, 1)
    c = ctypes.cast(consts, ctypes.c_void_p)
    opa, softmax = _lib.GF_REFINE_OPACITY, _lib.GF_REFINE_SEM_SOFTMAX
    fwd = lambda *head: _lib.call("gf_refine_forward", cpu, *head, c, *([None] * 10))
    bwd = lambda *head: _lib.call("gf_refine_backward", cpu, *head, c, *([None] * 12))
    for call in (fwd, bwd):
        name = "gf_refine_forward" if call is fwd else "gf_refine_backward"
        with pytest.raises(RuntimeError, match=name + r" failed \(code -1\): .*S must be"):
            call(64, 10 + 1 + 33, 44, 1, opa, 3, 33)
        with pytest.raises(RuntimeError, match=r"D must be 10 \+ opacity \+ S"):
            call(64, 28, 28, 1, 0, 3, 17)                    # no opacity column: D would be 27
        with pytest.raises(RuntimeError, match="Da is smaller"):
            call(64, 28, 2, 1, opa, 3, 17)
        with pytest.raises(RuntimeError, match="Da is smaller"):
            call(64, 28, 2, 2, opa, 0, 17)                   # version 2 reads three anchor columns
        with pytest.raises(RuntimeError, match="version"):
            call(64, 28, 28, 3, opa, 3, 17)
        with pytest.raises(RuntimeError, match="flags"):
            call(64, 28, 28, 1, opa | softmax | _lib.GF_REFINE_SEM_SOFTPLUS, 3, 17)
        with pytest.raises(RuntimeError, match="null pointer"):
            call(64, 28, 28, 1, opa, 3, 17)
        call(0, 28, 28, 1, opa, 3, 17)                       # nothing to do: no pointer is looked at


def test_abi_is_10_and_declares_the_entry_points():
    header = open(os.path.join(ROOT, "include", "gf_hip.h")).read()
    assert re.search(r"^#define\s+GF_ABI_VERSION\s+10\b", header, flags=re.M)
    assert _lib.GF_ABI_VERSION == 10 and _lib.load().gf_abi_version() == 10
    for name in ("gf_refine_forward", "gf_refine_backward"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and name in _lib.SIGNATURES
    from gaussianformer_amd import build as B
    assert "refine.hip" in B.SOURCES and "refine.hip" not in B.FP_ATOMICS
