"""TEST INFRASTRUCTURE for the anchor encoder's training step: the float64 walk of ``anchor_embed_ref`` that also returns every
stage's pre-activations, the kink filter's candidates built on it, and the kinds of its leaves.

The kink filter is tests/row_ref.py's, on every Linear of the twelve stages (each stands in front of a ReLU).  Never imported by
the product."""
import functools

import torch
import torch.nn.functional as F

import anchor_embed_ref as ref
import row_ref
from anchor_embed_ref import LAYOUTS as FAMILIES, make_input
from row_ref import CANDIDATES

PLANTS, INPUT_SEED = 6, 7


def walk(anchor, sd):
    """``anchor_embed_ref`` stage by stage in ``anchor``'s dtype: ``(out, [(name, z, scale)])`` with ``z`` every Linear's
    pre-activation and ``scale = sum_k |W_ok x_k| + |b_o|``, the size of the terms z is the sum of."""
    stages = []

    def stage(x, name):
        E = sd[name + ".0.bias"].shape[0]
        for lin, ln in ((0, 2), (3, 5)):
            W, b = sd[f"{name}.{lin}.weight"], sd[f"{name}.{lin}.bias"]
            z, scale = row_ref.linear_stage(x, W, b)
            stages.append((f"{name}.{lin}", z, scale))
            x = F.layer_norm(F.relu(z), (E,), sd[f"{name}.{ln}.weight"], sd[f"{name}.{ln}.bias"], 1e-5)
        return x

    opa = 1 if "opacity_fc.0.weight" in sd else 0
    out = stage(anchor[..., 0:3], "xyz_fc") + stage(anchor[..., 3:6], "scale_fc") + stage(anchor[..., 6:10], "rot_fc")
    if opa:
        out = out + stage(anchor[..., 10:11], "opacity_fc")
    if "semantics_fc.0.weight" in sd:
        S = sd["semantics_fc.0.weight"].shape[1]
        out = out + stage(anchor[..., 10 + opa:10 + opa + S], "semantics_fc")
    return stage(out, "output_fc"), stages


def relu_stages(anchor, sd):
    """The ``(z, scale)`` the kink filter judges the rows of ``anchor`` (float32 values) by: in float64, on the CPU."""
    with torch.no_grad():
        _, stages = walk(anchor.double().cpu(), ref.cast(sd, torch.float64, "cpu"))
    return [(z, scale) for _, z, scale in stages]


@functools.lru_cache(maxsize=None)
def candidates(name, seed=0, dead_branch=None):
    """``(x [1400, Da] float32, keep bool [1400], sd)`` of a family: the candidate rows (the six planted rows first), which
    of them the filter keeps, and the weights ``fixed_weights(seed)`` (with ``dead_branch``'s first bias at -1e6)."""
    opa, S, Da = FAMILIES[name]
    sd = ref.fixed_weights(bool(opa), S, seed=seed)
    if dead_branch:
        sd[dead_branch + ".0.bias"] = torch.full_like(sd[dead_branch + ".0.bias"], -1e6)
    x = make_input(CANDIDATES, opa, S, Da, INPUT_SEED + seed)
    return x, row_ref.kink_free(relu_stages(x, sd)), sd


def survivors(name, seed=0, dead_branch=None):
    """``(rows [m, Da] float32 on the CPU, sd)``: the candidates the filter keeps, in their order."""
    x, keep, sd = candidates(name, seed, dead_branch)
    return x[keep].contiguous(), sd


def kind(key):
    """The kind of a state_dict leaf, for the parameter gradients' yardsticks."""
    stage, slot = key.split(".", 1)
    if slot in ("0.weight", "3.weight"):
        return "square weight" if slot == "3.weight" or stage == "output_fc" else "thin weight"
    return {"0.bias": "Linear bias", "3.bias": "Linear bias", "2.weight": "LN weight", "5.weight": "LN weight",
            "2.bias": "LN bias", "5.bias": "LN bias"}[slot]
