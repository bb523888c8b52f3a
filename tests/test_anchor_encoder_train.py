"""The anchor encoder's training step without a GPU: the kink filter the GPU tests draw their rows from (its conditions are
asserted here, on the CPU), the float64 walk it is built on, the header's prototypes, the sizes query and the module's switch and routing
under a monkeypatched ``_lib.call``."""
import ctypes
import os
import re

import pytest
import torch

import anchor_embed_ref as ref
import anchor_embed_train_ref as tr
import row_ref
from gaussianformer_amd import _lib, anchor_encoder
from gaussianformer_amd.anchor_encoder import SparseGaussian3DEncoder, anchor_embed, anchor_embed_autograd, train_sizes
from row_judge import ptr_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference walk and the kink filter -------------------------------------------------------------------------------------

def test_walk_is_the_restatement():
    x, _, sd = tr.candidates("opa_s17")
    sd64 = ref.cast(sd, torch.float64)
    with torch.no_grad():
        out, stages = tr.walk(x[:64].double(), sd64)
        assert torch.equal(out, ref.anchor_embed_ref(x[:64].double(), sd64))
    assert [name for name, _, _ in stages] == [f"{st}.{lin}" for st in ref.STAGES for lin in (0, 3)]
    assert all(z.shape == (64, 128) and bool((scale >= z.abs() * (1 - 1e-12)).all()) for _, z, scale in stages)


@pytest.mark.parametrize("name", list(tr.FAMILIES))
def test_kink_filter_keeps_enough(name):
    """Measured for the eight families at seeds 0 and 1: 4.0-9.1 % rejected, at least 1 273 survivors, 4-6 plants."""
    x, keep, _ = tr.candidates(name)
    rejected, plants = 1.0 - keep.float().mean().item(), int(keep[:tr.PLANTS].sum())
    print(f"{name}: rejected {100 * rejected:.1f} %, survivors {int(keep.sum())}, plants kept {plants}")
    assert rejected <= 0.15
    assert plants >= 4
    assert int(keep.sum()) >= 1000


def test_kink_filter_rejects_a_kink():
    """A row whose first pre-activation is moved onto 0 (through the bias) is rejected; the untouched weights keep it."""
    x, keep, sd = tr.candidates("opa_s0")
    row = int(torch.nonzero(keep)[10])
    assert bool(row_ref.kink_free(tr.relu_stages(x[row:row + 1], sd)))
    z0 = torch.nn.functional.linear(x[row, 0:3].double(), sd["xyz_fc.0.weight"].double(), sd["xyz_fc.0.bias"].double())
    sd2 = dict(sd)
    sd2["xyz_fc.0.bias"] = sd["xyz_fc.0.bias"].clone()
    sd2["xyz_fc.0.bias"][5] -= z0[5].float()
    assert not bool(row_ref.kink_free(tr.relu_stages(x[row:row + 1], sd2)))


def test_kinds():
    kinds = {k: tr.kind(k) for k in ref.shapes(True, 17)}
    assert kinds["xyz_fc.0.weight"] == "thin weight" and kinds["output_fc.0.weight"] == "square weight"
    assert kinds["rot_fc.3.weight"] == "square weight" and kinds["opacity_fc.3.bias"] == "Linear bias"
    assert kinds["scale_fc.2.weight"] == "LN weight" and kinds["output_fc.5.bias"] == "LN bias"
    assert sorted(set(kinds.values())) == ["LN bias", "LN weight", "Linear bias", "square weight", "thin weight"]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------

def test_header_declares_the_training_step():
    text = open(os.path.join(ROOT, "include", "gf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(gf_anchor_embed_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))
    assert sorted(protos) == ["gf_anchor_embed_backward", "gf_anchor_embed_forward", "gf_anchor_embed_forward_train",
                              "gf_anchor_embed_train_sizes"]
    assert re.search(r"size_t\s*\*\s*saved_bytes,\s*size_t\s*\*\s*workspace_bytes\s*$", protos["gf_anchor_embed_train_sizes"])
    assert re.search(r"void\s*\*\s*saved,\s*size_t\s+saved_bytes,\s*void\s*\*\s*stream\s*$", protos["gf_anchor_embed_forward_train"])
    assert re.search(r"grad_out,\s*float\s*\*\s*grad_anchor,\s*void\s*\*\s*const\s*\*\s*grad_params,\s*void\s*\*\s*workspace,\s*"
                     r"size_t\s+workspace_bytes,\s*void\s*\*\s*stream\s*$", protos["gf_anchor_embed_backward"])
    for name in protos:
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert not any(n.endswith("_bytes") for n in protos)


def test_sizes():
    assert train_sizes(0, 1, 17) == (0, 0)
    prev = (0, 0)
    for n in (1, 31, 128, 129, 511, 512, 513, 1000, 25600, 144000):
        now = train_sizes(n, 1, 17)
        assert now[0] > prev[0] and now[1] > prev[1] and now[0] % 256 == 0 and now[1] % 256 == 0
        prev = now
    # the saved region: twelve stages' rows and statistics and the sum, about 6.8 KB per anchor at (opa, 17)
    assert 6700 * 144000 < train_sizes(144000, 1, 17)[0] < 6800 * 144000
    # fewer branches, smaller regions; S only says whether the semantic branch exists
    assert train_sizes(1000, 0, 0) < train_sizes(1000, 1, 0) < train_sizes(1000, 1, 1) == train_sizes(1000, 1, 32)
    # one more block of the weight-gradient kernel, one more partial of every weight
    B = _lib.GF_ANCHOR_EMBED_WGRAD_ROWS
    step = train_sizes(B + 1, 1, 17)[1] - train_sizes(B, 1, 17)[1]
    assert step >= 7 * 128 * 128 * 4


def test_sizes_refuses():
    lib = _lib.load()
    a, b = ctypes.c_size_t(7), ctypes.c_size_t(7)
    pa, pb = ctypes.addressof(a), ctypes.addressof(b)
    assert lib.gf_anchor_embed_train_sizes(-1, 1, 17, pa, pb) == -1 and b"negative n" in lib.gf_last_error()
    assert lib.gf_anchor_embed_train_sizes(10, 1, 33, pa, pb) == -1 and b"S must be" in lib.gf_last_error()
    assert lib.gf_anchor_embed_train_sizes(10, 1, -1, pa, pb) == -1
    assert lib.gf_anchor_embed_train_sizes(10, 1, 17, None, pb) == -1 and b"null" in lib.gf_last_error()
    assert (a.value, b.value) == (7, 7)
    with pytest.raises(RuntimeError, match=r"gf_anchor_embed_train_sizes failed \(code -1\)"):
        train_sizes(-5, 1, 17)


def test_entry_points_check_arguments_before_the_device():
    lib = _lib.load()
    pt = ptr_table([], 48)
    assert lib.gf_anchor_embed_forward_train(8, 28, 256, 1, 17, None, pt, None, None, 0, None) == -1
    assert b"gf_anchor_embed_forward_train" in lib.gf_last_error() and b"128" in lib.gf_last_error()
    assert lib.gf_anchor_embed_backward(8, 28, 128, 1, 33, None, pt, None, None, None, pt, None, 0, None) == -1
    assert b"gf_anchor_embed_backward" in lib.gf_last_error() and b"S must be" in lib.gf_last_error()
    assert lib.gf_anchor_embed_backward(8, 27, 128, 1, 17, None, pt, None, None, None, pt, None, 0, None) == -1
    assert b"Da" in lib.gf_last_error()
    assert lib.gf_anchor_embed_backward(8, 28, 128, 1, 17, None, pt, None, None, None, pt, None, 0, None) == -1
    assert b"null parameter" in lib.gf_last_error()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------

def test_module_switch():
    """``native_training`` is an attribute, off by default; the constructor stays the reference's and takes no such key."""
    import inspect
    assert "native_training" not in inspect.signature(SparseGaussian3DEncoder.__init__).parameters
    with pytest.raises(TypeError):
        SparseGaussian3DEncoder(embed_dims=128, native_training=True)
    assert SparseGaussian3DEncoder.native_training is False
    plain = SparseGaussian3DEncoder(embed_dims=128, semantics=True, semantic_dim=17)
    native = SparseGaussian3DEncoder(embed_dims=128, semantics=True, semantic_dim=17)
    native.native_training = True
    assert plain.native_training is False and native.native_training is True and SparseGaussian3DEncoder.native_training is False
    assert list(plain.state_dict()) == list(native.state_dict()) == list(ref.shapes(True, 17))
    native.load_state_dict(plain.state_dict(), strict=True)


@pytest.fixture
def routes(monkeypatch):
    """What the module decides for a tensor that claims to be an fp32 GPU tensor: ``_launch`` and ``AnchorEmbedFunction.apply``
    are replaced by recorders, and ``_lib.call`` fails the test (nothing may reach the library from here)."""
    seen = []
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("the library was called"))
    monkeypatch.setattr(anchor_encoder, "_launch", lambda anchor, params: seen.append("forward") or torch.zeros(anchor.shape[0], 128))

    class Fn:
        @staticmethod
        def apply(anchor, *params):
            assert len(params) == 48
            seen.append("train")
            return torch.zeros(anchor.shape[0], 128)
    monkeypatch.setattr(anchor_encoder, "AnchorEmbedFunction", Fn)
    return seen


class _OnGpu(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True: the module's routing reads nothing else of the device."""
    is_cuda = True


def _claimed(t):
    return t.as_subclass(_OnGpu)


def _module(native_training, E=128, S=17):
    m = SparseGaussian3DEncoder(embed_dims=E, semantics=S > 0, semantic_dim=S or None)
    m.native_training = native_training
    return m


def test_routing(routes, monkeypatch):
    monkeypatch.setattr(SparseGaussian3DEncoder, "forward_torch", lambda self, x: routes.append("torch") or torch.zeros(x.shape[0], self.embed_dims))
    x = _claimed(torch.zeros(5, 28))
    xg = _claimed(torch.zeros(5, 28)).requires_grad_(True)
    for native in (False, True):
        m = _module(native)
        params = [_claimed(p) for p in m.parameters()]
        monkeypatch.setattr(anchor_encoder, "_param_list", lambda mod, params=params: (params * 48)[:48])
        del routes[:]
        with torch.no_grad():
            m(x)
        m(xg)                                              # needs autograd: the switch decides
        m(_claimed(torch.zeros(5, 28, dtype=torch.float64)))   # another dtype: torch, whatever the switch
        m(torch.zeros(5, 28))                              # a CPU tensor: torch
        assert routes == ["forward", "train" if native else "torch", "torch", "torch"]
    del routes[:]
    _module(True, E=256)(xg)                               # another width: torch
    _module(True, S=33)(_claimed(torch.zeros(5, 44)).requires_grad_(True))   # a semantic width beyond the native op's
    assert routes == ["torch", "torch"]


def test_functionals_on_cpu_tensors():
    sd = ref.fixed_weights(True, 17)
    x = torch.zeros(4, 28, requires_grad=True)
    with pytest.raises(RuntimeError, match="without a native backward.*anchor_embed_autograd"):
        anchor_embed(x, sd)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        anchor_embed_autograd(x, sd)
    with pytest.raises(RuntimeError, match="no CPU fallback"), torch.no_grad():
        anchor_embed_autograd(x, sd)
