"""The deformable block without a GPU: the restatement against what the reference's own module computed
(tests/golden/caller_dfa.npz), the drop-in module's structure, and the two entry points' refusals (which come before any HIP
call)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import deform_block_ref as ref
from gaussianformer_amd import _lib
from gaussianformer_amd.deformable_block import DeformableFeatureAggregation, deformable_logits, deformable_output
from gaussianformer_amd.key_points import SparseGaussian3DKeyPointsGenerator
from row_judge import host_table

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caller_dfa.npz")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def config():
    cfg = dict(ref.FIXTURE_CONFIG)
    cfg["kps_generator"] = dict(cfg["kps_generator"])
    return cfg


def relative(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-6)


def test_restatement_reproduces_the_reference_module(golden):
    """The float64 restatement on the fixture's parameters and inputs against the output the reference's module produced
    (float32, CPU oracle kernels), with the bound of tests/test_ref_callers.py::test_dfa_call_replayed_on_the_dropin."""
    d = golden
    t = lambda k: torch.from_numpy(d[k]).double()
    sd = {k[len("param_"):]: t(k) for k in d.files if k.startswith("param_")}
    maps = [t(f"feature_map{i}") for i in range(len(d["levels"]))]
    out = ref.module_ref(sd, config(), t("instance_feature"), t("anchor"), t("anchor_embed"), maps, t("projection_mat"), t("image_wh"))
    err = relative(out.numpy(), d["output"])
    print(f"float64 restatement against the recorded output: {err:.3e}")
    assert err <= 1e-4
    # the right half of a "cat" row is the instance feature itself
    assert np.array_equal(out[..., 32:].numpy(), d["instance_feature"].astype(np.float64))


def test_state_dict_is_the_reference_s(golden):
    m = DeformableFeatureAggregation(**config())
    want = {k[len("param_"):]: golden[k].shape for k in golden.files if k.startswith("param_")}
    sd = m.state_dict()
    assert set(sd) == set(want) and {k: tuple(v.shape) for k, v in sd.items()} == want
    assert list(sd) == list(ref.shapes(config()))       # the restatement's shape map is the module's, in its order
    m.load_state_dict({k: torch.from_numpy(golden["param_" + k]) for k in want}, strict=True)
    assert "native_dense" not in sd and DeformableFeatureAggregation.native_dense is True
    assert isinstance(m.kps_generator, SparseGaussian3DKeyPointsGenerator) and m.kps_generator.embed_dims == 32
    assert (m.num_pts, m.group_dims, m.num_levels, m.num_groups, m.num_cams, m.attn_drop, m.residual_mode) == (9, 8, 3, 4, 3, 0.0, "cat")
    assert [type(x).__name__ for x in m.camera_encoder] == ["Linear", "ReLU", "LayerNorm", "Linear", "ReLU", "LayerNorm"]
    assert m.camera_encoder[0].in_features == 12 and isinstance(m.proj_drop, nn.Dropout) and m.proj_drop.p == 0.0


def test_constructor_without_the_camera_embedding_and_defaults():
    kps = dict(type="SparseGaussian3DKeyPointsGenerator", num_learnable_pts=6, fix_scale=ref.FIX7, pc_range=[-50, -50, -5, 50, 50, 3],
               scale_range=[0.08, 0.64])
    m = DeformableFeatureAggregation(embed_dims=128, num_groups=4, kps_generator=kps, use_deformable_func=True, proj_drop=0.1, attn_drop=0.15)
    assert m.camera_encoder is None and m.weights_fc.out_features == 4 * 6 * 4 * 13 and m.residual_mode == "add"
    assert kps["embed_dims"] == 128 and m.kps_generator.learnable_fc.out_features == 18     # (embed_dims forced, :124)
    assert list(m.state_dict()) == ["kps_generator.learnable_fc.weight", "kps_generator.learnable_fc.bias", "output_proj.weight",
                                    "output_proj.bias", "weights_fc.weight", "weights_fc.bias"]
    with pytest.raises(ValueError, match="divisible"):
        DeformableFeatureAggregation(embed_dims=130, num_groups=4, kps_generator=dict(kps), use_deformable_func=True)
    with pytest.raises(AssertionError):
        DeformableFeatureAggregation(embed_dims=128, kps_generator=dict(kps))          # use_deformable_func=False, as the reference


def test_init_weight():
    m = DeformableFeatureAggregation(**config())
    torch.manual_seed(3)
    m.init_weight()
    assert not m.weights_fc.weight.any() and not m.weights_fc.bias.any() and not m.output_proj.bias.any()
    w = m.output_proj.weight.detach()
    limit = float(np.sqrt(6.0 / (32 + 32)))         # xavier-uniform, gain 1
    assert float(w.abs().max()) <= limit and float(w.abs().max()) > 0.8 * limit and abs(float(w.mean())) < 0.05
    torch.manual_seed(3)
    again = torch.empty(32, 32)
    nn.init.xavier_uniform_(again)
    assert torch.equal(w, again)


def test_functions_refuse_cpu_tensors_and_autograd():
    f, e = torch.zeros(2, 5, 128), torch.zeros(2, 5, 128)
    wfc, lfc, proj = nn.Linear(128, 144), nn.Linear(128, 6), nn.Linear(128, 128)
    with pytest.raises(RuntimeError, match="without a native backward.*deformable_fused"):
        deformable_logits(f, e, wfc, lfc)
    with pytest.raises(RuntimeError, match="without a native backward.*deformable_fused"):
        deformable_output(f, proj, e)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            deformable_logits(f, e, wfc, lfc)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            deformable_logits(f, None, (wfc.weight, wfc.bias))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            deformable_output(f, proj, e, "cat")
        with pytest.raises(ValueError, match="residual_mode"):
            deformable_output(f, proj, e, "mul")
        with pytest.raises(ValueError, match="needs instance_feature"):
            deformable_output(f, proj, None, "add")


def test_module_refuses_cpu_tensors(golden):
    """No quiet CPU route: the module's middle is the native op on every route."""
    m = DeformableFeatureAggregation(**config()).eval()
    t = lambda k: torch.from_numpy(golden[k])
    maps = [t(f"feature_map{i}") for i in range(3)]
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(t("instance_feature"), t("anchor"), t("anchor_embed"), maps, dict(projection_mat=t("projection_mat"), image_wh=t("image_wh")))


BUF = torch.zeros(4096)


def _table(count, drop=(), misalign=None):
    return host_table(BUF, count, drop, misalign)


def _logits(n=4, e=128, k3=6, nw=144, feature=BUF, embed=BUF, learned=None, raw=None, table=None, **kw):
    """``gf_deform_logits_forward`` through ``_lib.call`` on host memory: it must refuse before it touches a device."""
    out = torch.zeros(8192)
    learned = out[:1024] if learned is None else learned
    raw = out[1024:] if raw is None else raw
    _lib.call("gf_deform_logits_forward", CPU, n, e, k3, nw, feature, embed, _table(4, **kw) if table is None else table, learned, raw)


def _output(n=4, e=128, mode=1, features=BUF, inst=BUF, residual=None, out=None, table=None, drop=(2, 3), **kw):
    out = torch.zeros(4096) if out is None else out
    _lib.call("gf_deform_output_forward", CPU, n, e, mode, features, inst, _table(4, drop=drop, **kw) if table is None else table, residual, out)


def test_logits_entry_point_refusals():
    assert BUF.data_ptr() % 16 == 0
    fail = r"gf_deform_logits_forward failed \(code -1\): gf_deform_logits_forward: "
    for kw, msg in ((dict(e=256), r"E = 256: only embed_dims = 128"), (dict(k3=33), r"K3 = 33"), (dict(k3=-3), r"K3 = -3"),
                    (dict(nw=0), r"Nw = 0"), (dict(nw=146), r"Nw = 146"), (dict(nw=-4), r"Nw = -4"), (dict(n=-1), r"n = -1 is negative"),
                    (dict(drop=(2,)), r"weights_fc.weight is missing"), (dict(drop=(3,)), r"weights_fc.bias is missing"),
                    (dict(drop=(0,)), r"kps_generator.learnable_fc.weight is missing"),
                    (dict(drop=(1,)), r"kps_generator.learnable_fc.bias is missing"),
                    (dict(misalign=2), r"weights_fc.weight is not 16-byte aligned"),
                    (dict(misalign=1), r"kps_generator.learnable_fc.bias is not 16-byte aligned"),
                    (dict(feature=BUF[1:]), r"instance_feature is not 16-byte aligned"),
                    (dict(embed=BUF[1:]), r"anchor_embed is not 16-byte aligned"),
                    (dict(raw=torch.zeros(2048)[1:]), r"raw is not 16-byte aligned"),
                    (dict(learned=torch.zeros(2048)[3:]), r"learned is not 16-byte aligned"),
                    (dict(feature=None), r"null pointer"), (dict(raw=BUF[256:]), r"raw aliases an input"),
                    (dict(learned=BUF[508:]), r"learned aliases an input")):
        with pytest.raises(RuntimeError, match=fail + msg):
            _logits(**kw)
    both = torch.zeros(4096)
    with pytest.raises(RuntimeError, match=fail + r"learned aliases raw"):
        _logits(learned=both[:64], raw=both[20:])
    with pytest.raises(RuntimeError, match=fail + r"null params"):
        _lib.call("gf_deform_logits_forward", CPU, 4, 128, 6, 144, BUF, BUF, None, BUF, BUF)
    _logits(n=0)                                              # GF_OK, no launch
    _logits(n=0, k3=0, drop=(0, 1), embed=None, nw=1 << 20)   # no learnable_fc, no embedding, any width


def test_output_entry_point_refusals():
    fail = r"gf_deform_output_forward failed \(code -1\): gf_deform_output_forward: "
    for kw, msg in ((dict(e=32), r"E = 32: only embed_dims = 128"), (dict(mode=3), r"mode = 3"), (dict(n=-2), r"n = -2 is negative"),
                    (dict(drop=(0, 2, 3)), r"output_proj.weight is missing"), (dict(drop=(1, 2, 3)), r"output_proj.bias is missing"),
                    (dict(drop=(2,)), r"a half-present pair: norm.weight is null and norm.bias is not"),
                    (dict(drop=(3,)), r"a half-present pair: norm.bias is null and norm.weight is not"),
                    (dict(mode=2, drop=()), r"a post norm with mode = 2"), (dict(mode=2, residual=BUF), r"a residual with mode = 2"),
                    (dict(misalign=0), r"output_proj.weight is not 16-byte aligned"), (dict(drop=(), misalign=3), r"norm.bias is not 16-byte aligned"),
                    (dict(features=BUF[1:]), r"features is not 16-byte aligned"), (dict(inst=BUF[2:]), r"instance_feature is not 16-byte aligned"),
                    (dict(residual=BUF[3:]), r"residual is not 16-byte aligned"), (dict(out=torch.zeros(4096)[1:]), r"out is not 16-byte aligned"),
                    (dict(features=None), r"null pointer"), (dict(inst=None), r"null pointer"),
                    (dict(out=BUF[256:]), r"out aliases an input"), (dict(mode=2, out=BUF[508:]), r"out aliases an input")):
        with pytest.raises(RuntimeError, match=fail + msg):
            _output(**kw)
    side = torch.zeros(4096)
    with pytest.raises(RuntimeError, match=fail + r"out aliases an input"):
        _output(mode=0, inst=None, residual=side, out=side[128:])
    with pytest.raises(RuntimeError, match=fail + r"null params"):
        _lib.call("gf_deform_output_forward", CPU, 4, 128, 1, BUF, BUF, None, None, BUF)
    _output(n=0)
    _output(n=0, mode=0, inst=None, drop=())


def test_constants_and_build_list():
    from gaussianformer_amd import build as B
    assert (_lib.GF_DEFORM_EMBED_DIMS, _lib.GF_DEFORM_MAX_LEARNED, _lib.GF_DEFORM_LOGITS_PARAMS, _lib.GF_DEFORM_OUTPUT_PARAMS) == (128, 32, 4, 4)
    assert (_lib.GF_DEFORM_NONE, _lib.GF_DEFORM_ADD, _lib.GF_DEFORM_CAT) == (0, 1, 2)
    assert "deform_dense.hip" in B.SOURCES and "deform_dense.hip" not in B.FP_ATOMICS and "gf_rows.hpp" in B.HEADERS
    assert _lib.GF_ABI_VERSION == 10 and _lib.load().gf_abi_version() == 10
