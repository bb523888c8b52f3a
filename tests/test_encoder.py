"""The drop-in ``GaussianOccEncoder`` without a GPU: the plan of every shipped ``operation_order``, construction from the
recorded settings of every config family (tests/golden/encoder_orders.json, tools/make_golden_encoder.py), the ``state_dict``
layout, ``init_weights`` and ``set_native``."""
import json
import os

import pytest
import torch
import torch.nn as nn

from gaussianformer_amd import GaussianOccEncoder
from gaussianformer_amd.encoder import Step, build_module, plan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_orders.json")
FAMILIES = ["nuscenes_gs144000", "nuscenes_gs25600_solid", "prob/nuscenes_gs6400", "prob/nuscenes_gs12800", "prob/nuscenes_gs25600"]

# the shipped orders, written out (their source: the golden file, compared below)
FIRST = ["deformable", "ffn", "norm", "refine"]
LATER = ["spconv", "norm", "deformable", "ffn", "norm", "refine"]
SOLID_ORDER = FIRST + LATER * 3
PROB_BLOCK = ["identity", "deformable", "add", "norm", "identity", "ffn", "add", "norm", "identity", "spconv", "add", "norm",
              "identity", "ffn", "add", "norm", "refine"]
PROB_ORDER = PROB_BLOCK * 4
ORDERS = {"nuscenes_gs144000": SOLID_ORDER, "nuscenes_gs25600_solid": SOLID_ORDER, "prob/nuscenes_gs6400": PROB_ORDER,
          "prob/nuscenes_gs12800": PROB_ORDER, "prob/nuscenes_gs25600": PROB_ORDER}
DEFAULT_BLOCK = ["spconv", "norm", "deformable", "norm", "ffn", "norm", "refine"]


def solid_plan():
    """"cat" absorbs nothing; "ffn", "norm" and "spconv", "norm" are one step each."""
    steps = [Step("deformable", 0, False, None), Step("ffn", 1, False, 2), Step("refine", 3, False, None)]
    for b in range(3):
        o = 4 + 6 * b
        steps += [Step("spconv", o, False, o + 1), Step("deformable", o + 2, False, None), Step("ffn", o + 3, False, o + 4),
                  Step("refine", o + 5, False, None)]
    return steps


def prob_plan():
    """Every "identity", X, "add", "norm" is the identity and one step."""
    steps = []
    for b in range(4):
        o = 17 * b
        for j, op in enumerate(("deformable", "ffn", "spconv", "ffn")):
            steps += [Step("identity", o + 4 * j, False, None), Step(op, o + 4 * j + 1, True, o + 4 * j + 3)]
        steps.append(Step("refine", o + 16, False, None))
    return steps


def default_plan(num_decoder):
    steps = []
    for b in range(num_decoder):
        o = 7 * b
        steps += [Step("spconv", o, False, o + 1), Step("deformable", o + 2, False, o + 3), Step("ffn", o + 4, False, o + 5),
                  Step("refine", o + 6, False, None)]
    return steps


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


class _Mode:
    def __init__(self, mode):
        self.residual_mode = mode


def _layers(order, mode):
    return [_Mode(mode) if op == "deformable" else None for op in order]


@pytest.mark.parametrize("family", FAMILIES)
def test_plan_of_the_shipped_orders(recorded, family):
    order = recorded[family]["operation_order"]
    assert order == ORDERS[family]
    mode = recorded[family]["deformable_model"]["residual_mode"]
    assert mode == ("none" if family.startswith("prob/") else "cat")
    want = prob_plan() if family.startswith("prob/") else solid_plan()
    assert plan(order, _layers(order, mode)) == want
    covered = sorted(i for s in want for i in (s.index, *([s.index + 1] if s.add else []), *([] if s.norm is None else [s.norm])))
    assert covered == list(range(len(order)))          # every op of the order belongs to exactly one step


def test_plan_of_the_default_order():
    order = DEFAULT_BLOCK * 2
    assert plan(order, _layers(order, "add")) == default_plan(2)
    assert plan(order) == default_plan(2)              # (without layers every block absorbs)


def test_plan_cat_absorbs_nothing():
    order = ["identity", "deformable", "add", "norm"]
    assert plan(order, _layers(order, "cat")) == [Step(op, i, False, None) for i, op in enumerate(order)]
    assert plan(order, _layers(order, "none")) == [Step("identity", 0, False, None), Step("deformable", 1, True, 3)]


def test_plan_add_without_identity_is_not_absorbed():
    assert plan(["ffn", "add", "norm"]) == [Step("ffn", 0, False, None), Step("add", 1, False, None), Step("norm", 2, False, None)]
    # an identity anywhere earlier in the order serves (the reference's variable stays assigned)
    assert plan(["identity", "norm", "ffn", "add"]) == [Step("identity", 0, False, None), Step("norm", 1, False, None), Step("ffn", 2, True, None)]
    # only an IMMEDIATELY following add / norm
    assert plan(["identity", "ffn", "norm", "add"]) == [Step("identity", 0, False, None), Step("ffn", 1, False, 2), Step("add", 3, False, None)]


def test_plan_unknown_op_raises_the_references_message():
    with pytest.raises(NotImplementedError, match="^temporal is not supported.$"):
        plan(["ffn", "temporal", "norm"])
    plan(["mid_refine", "refine"])                     # ("refine" in op)


def _encoder(settings, num_blocks=1, **over):
    cfg = {k: v for k, v in settings.items() if k != "operation_order"}
    block = 17 if "identity" in settings["operation_order"] else None
    order = settings["operation_order"][:17 * num_blocks] if block else settings["operation_order"][:4 + 6 * num_blocks]
    cfg.update(operation_order=order, **over)
    return GaussianOccEncoder(**cfg)


@pytest.mark.parametrize("family", FAMILIES)
def test_construction_and_state_dict_keys(recorded, family):
    enc = _encoder(recorded[family])
    order = enc.operation_order
    assert len(enc.layers) == len(order)
    want = ["anchor_encoder." + k for k in enc.anchor_encoder.state_dict()]
    for i, op in enumerate(order):
        if op in ("identity", "add"):
            assert enc.layers[i] is None
        else:
            assert enc.layers[i] is not None
            want += [f"layers.{i}.{k}" for k in enc.layers[i].state_dict()]
    assert list(enc.state_dict()) == want
    kinds = {"norm": "LayerNorm", "ffn": "AsymmetricFFN", "deformable": "DeformableFeatureAggregation", "spconv": "SparseConv3D",
             "refine": recorded[family]["refine_layer"]["type"]}
    assert [type(m).__name__ for m, op in zip(enc.layers, order) if m is not None] == [kinds[op] for op in order if op in kinds]
    # one module per occurrence, none shared
    mods = [m for m in enc.layers if m is not None]
    assert len({id(m) for m in mods}) == len(mods)
    assert enc.steps == plan(order, enc.layers)
    multi = recorded[family]["spconv_layer"].get("use_multi_layer", False)
    sp = [m for m, op in zip(enc.layers, order) if op == "spconv"][0]
    assert isinstance(sp.layer, nn.ModuleList) == multi and type(sp).native_tail is True and "native_tail" not in sp.state_dict()


def test_default_order_and_module_instances(recorded):
    s = recorded["nuscenes_gs25600_solid"]
    ffn = build_module(s["ffn"])
    enc = GaussianOccEncoder(s["anchor_encoder"], s["norm_layer"], ffn, s["deformable_model"], s["refine_layer"],
                             spconv_layer=s["spconv_layer"], num_decoder=2)
    assert enc.operation_order == DEFAULT_BLOCK * 2
    a, b = enc.layers[4], enc.layers[11]
    assert a is not ffn and b is not ffn and a is not b          # a module given directly: one deep copy per occurrence
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), ffn.parameters()))
    assert GaussianOccEncoder.fold is True and "fold" not in enc.state_dict()


def test_unknown_type_raises(recorded):
    s = dict(recorded["nuscenes_gs25600_solid"])
    s["ffn"] = dict(s["ffn"], type="MixtureFFN")
    with pytest.raises(ValueError, match="MixtureFFN"):
        _encoder(s)


def test_init_weights(recorded):
    torch.manual_seed(0)
    enc = _encoder(recorded["prob/nuscenes_gs6400"])
    refine = [m for m, op in zip(enc.layers, enc.operation_order) if op == "refine"]
    before = [p.detach().clone() for m in refine for p in m.parameters()]
    marks = []
    for m, op in zip(enc.layers, enc.operation_order):
        if op == "ffn":
            marks.append((m.layers[1].weight, m.layers[1].weight.detach().clone()))
    enc.init_weights()
    for m, op in zip(enc.layers, enc.operation_order):
        if op == "deformable":
            assert not m.weights_fc.weight.any() and not m.weights_fc.bias.any() and not m.output_proj.bias.any()
            assert m.output_proj.weight.abs().max() > 0
    assert all(torch.equal(p, q) for p, q in zip([p for m in refine for p in m.parameters()], before))
    assert all(not torch.equal(p, q) for p, q in marks)          # the xavier pass reached the other layers' matrices


def test_set_native(recorded):
    enc = _encoder(recorded["prob/nuscenes_gs6400"])
    having = lambda name: [m for m in enc.modules() if hasattr(m, name)]
    assert having("native_training") and having("fused_mlp")
    before = {id(m): dict(vars(m)) for m in enc.modules()}
    assert enc.set_native() is enc
    assert all(dict(vars(m)) == before[id(m)] for m in enc.modules())           # nothing asked, nothing set
    assert enc.set_native(training=True, fused_mlp=True) is enc
    assert all(m.native_training is True for m in having("native_training"))
    assert all(m.fused_mlp is True for m in having("fused_mlp"))
    for m in enc.modules():                                                     # ... and only those
        extra = {k: v for k, v in vars(m).items() if k not in before[id(m)] or before[id(m)][k] is not v}
        assert set(extra) <= {"native_training", "fused_mlp"}
    enc.set_native(training=False)
    assert all(m.native_training is False for m in having("native_training"))
    assert all(m.fused_mlp is True for m in having("fused_mlp"))
    # the classes' defaults are untouched
    from gaussianformer_amd.ffn import AsymmetricFFN
    from gaussianformer_amd.refine import SparseGaussian3DRefinementModuleV2
    assert AsymmetricFFN.native_training is False and SparseGaussian3DRefinementModuleV2.fused_mlp is False
