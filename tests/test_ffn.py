"""The feed-forward block without a GPU: the restatement against the reference's recorded outputs, the drop-in module's
structure and CPU route, and the entry point's refusals (which come before any HIP call)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import ffn_ref as ref
from gaussianformer_amd import _lib
from gaussianformer_amd.ffn import AsymmetricFFN, ffn_block
from row_judge import bound, held, host_table, max_error

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ffn.npz")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def weights_of(golden, name, dtype=torch.float32):
    shapes = ref.family_shapes(name)
    cin = shapes["layers.0.0.weight"][1]
    return ref.fixed_weights(cin, "pre_norm.weight" in shapes, "identity_fc.weight" in shapes, seed=int(golden[name + ".seed"]), dtype=dtype)


def module_of(golden, name):
    m = AsymmetricFFN(**ref.FAMILIES[name])
    m.load_state_dict(ref.module_state(weights_of(golden, name)), strict=True)
    return m


@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_restatement_equals_the_reference_in_float64(golden, name):
    sd = weights_of(golden, name, torch.float64)
    x = torch.from_numpy(golden[name + ".input"]).double()
    res = x if ref.FOLLOWED_BY_ADD[name] else None
    for key, got in (("ffn64", ref.ffn_ref(x, sd, norm=False)), ("block64", ref.ffn_ref(x, sd, residual=res))):
        want = golden[f"{name}.{key}"]
        assert np.abs(got.numpy() - want).max() <= 1e-10 * np.abs(want).max(), (name, key)


@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_state_dict_is_the_reference_s(golden, name):
    m = module_of(golden, name)     # (strict=True)
    sd = m.state_dict()
    assert list(sd.keys()) == list(golden[name + ".keys"])
    assert [list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()] == golden[name + ".shapes"].tolist()
    assert m.layers[0][1] is m.activate and isinstance(m.activate, nn.ReLU)
    assert [type(x).__name__ for x in m.layers] == ["Sequential", "Linear", "Dropout"] and m.layers[2].p == 0.1


def test_identity_fc_quirk(golden):
    base, prob = module_of(golden, "base"), module_of(golden, "prob")
    assert isinstance(base.identity_fc, nn.Linear) and (base.identity_fc.in_features, base.identity_fc.out_features) == (256, 128)
    assert not prob.add_identity and not hasattr(prob, "identity_fc")
    same = AsymmetricFFN(in_channels=64, embed_dims=32, feedforward_channels=32)
    assert isinstance(same.identity_fc, nn.Identity)            # F == E: Identity, whatever in_channels is
    assert same.in_channels == 64 and same.pre_norm is None and isinstance(same.dropout_layer, nn.Identity)
    wide = AsymmetricFFN(in_channels=128, embed_dims=128, feedforward_channels=512)
    assert isinstance(wide.identity_fc, nn.Linear)              # in_channels == E, F != E: still a Linear
    with pytest.raises(TypeError):                              # ... of self.in_channels, which may be None, as in the reference
        AsymmetricFFN(embed_dims=128, feedforward_channels=512)


@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_cpu_route_meets_the_recorded_truth(golden, name):
    m = module_of(golden, name).eval()
    x = torch.from_numpy(golden[name + ".input"])
    with torch.no_grad():
        out = m(x)
    truth = golden[name + ".ffn64"]
    held(f"{name} cpu route", out.numpy(), truth, bound(max_error(golden[name + ".ffn32"], truth), truth))


def test_training_with_dropout_takes_the_torch_route_and_is_stochastic(golden, monkeypatch):
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    m = module_of(golden, "base").train()
    x = torch.from_numpy(golden["base.input"])
    torch.manual_seed(0)
    a = m(x)
    b = m(x)
    assert names == [] and a.requires_grad and not torch.equal(a, b)
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x), m(x)) and names == []


def test_constructor_refusals():
    with pytest.raises(NotImplementedError, match="BN"):
        AsymmetricFFN(in_channels=256, pre_norm=dict(type="BN"), embed_dims=128, feedforward_channels=512)
    with pytest.raises(NotImplementedError, match="Swish"):
        AsymmetricFFN(embed_dims=128, feedforward_channels=512, act_cfg=dict(type="Swish"))
    with pytest.raises(NotImplementedError, match="DropPath"):
        AsymmetricFFN(embed_dims=128, feedforward_channels=512, dropout_layer=dict(type="DropPath", drop_prob=0.1))
    with pytest.raises(AssertionError, match="num_fcs"):
        AsymmetricFFN(embed_dims=128, feedforward_channels=512, num_fcs=1)
    m = AsymmetricFFN(in_channels=128, embed_dims=128, feedforward_channels=512, act_cfg=dict(type="GELU"), dropout_layer=dict(type="Dropout", drop_prob=0.2), num_fcs=3)
    assert isinstance(m.activate, nn.GELU) and isinstance(m.dropout_layer, nn.Dropout) and m.dropout_layer.p == 0.2 and len(m.layers) == 4


def test_ffn_block_refuses_cpu_tensors_and_autograd(golden):
    m = module_of(golden, "prob").eval()
    x = torch.from_numpy(golden["prob.input"])
    with pytest.raises(RuntimeError, match="without a native backward"):
        ffn_block(x, m)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        ffn_block(x, m)


def _raw(n=4, cin=256, f=512, e=128, drop=(), misalign=None, half=None):
    """``gf_ffn_forward`` through ``_lib.call`` on host memory: it must refuse before it touches a device."""
    buf = torch.zeros(64)
    assert buf.data_ptr() % 16 == 0
    _lib.call("gf_ffn_forward", CPU, n, cin, f, e, buf, host_table(buf, 10, drop, misalign), None, buf)


def test_entry_point_refusals():
    fail = r"gf_ffn_forward failed \(code -1\): gf_ffn_forward: "
    with pytest.raises(RuntimeError, match=fail + r"E = 256: only embed_dims = 128"):
        _raw(e=256)
    with pytest.raises(RuntimeError, match=fail + r"F = 1024: only feedforward_channels = 512"):
        _raw(f=1024)
    with pytest.raises(RuntimeError, match=fail + r"Cin = 192: only in_channels = 128 or 256"):
        _raw(cin=192)
    with pytest.raises(RuntimeError, match=fail + r"n = -1 is negative"):
        _raw(n=-1)
    with pytest.raises(RuntimeError, match=fail + r"a half-present pair: pre_norm.bias is null and pre_norm.weight is not"):
        _raw(drop=(1,))
    with pytest.raises(RuntimeError, match=fail + r"a half-present pair: norm.weight is null and norm.bias is not"):
        _raw(drop=(8,))
    with pytest.raises(RuntimeError, match=fail + r"layers.1.weight is missing"):
        _raw(drop=(4,))
    with pytest.raises(RuntimeError, match=fail + r"layers.0.0.bias is missing"):
        _raw(drop=(3,))
    with pytest.raises(RuntimeError, match=fail + r"identity_fc.weight is not 16-byte aligned"):
        _raw(misalign=6)
    with pytest.raises(RuntimeError, match=fail + r"null params"):
        _lib.call("gf_ffn_forward", CPU, 4, 256, 512, 128, None, None, None, None)
    _raw(n=0)                                   # GF_OK, no launch
    _raw(n=0, drop=(0, 1, 6, 7, 8, 9))          # every optional part absent


def test_constants_and_build_list():
    from gaussianformer_amd import build as B
    assert (_lib.GF_FFN_PARAMS, _lib.GF_FFN_EMBED_DIMS, _lib.GF_FFN_HIDDEN) == (10, 128, 512)
    assert "ffn.hip" in B.SOURCES and "ffn.hip" not in B.FP_ATOMICS and "gf_rows.hpp" in B.HEADERS
