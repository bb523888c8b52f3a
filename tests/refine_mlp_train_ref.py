"""TEST INFRASTRUCTURE for the refinement modules' native training step: the float64 walk of ``refine_ref.mlp`` that also
returns every stage's pre-activation, the kink filter's candidates built on it, and the kinds of its leaves.

The kink filter is tests/row_ref.py's, on the four Linears in front of a ReLU (the last Linear's pre-activation is walked too,
but no ReLU follows it).  Never imported by the product."""
import functools

import torch
import torch.nn.functional as F

import row_ref
from gaussianformer_amd.refine import MLP_KEYS
from refine_ref import VARIANTS, make_inputs, make_module
from row_ref import CANDIDATES

RELU_STAGES = (0, 2, 5, 7)


def walk(state, x):
    """``refine_ref.mlp`` stage by stage in ``x``'s dtype: ``(out, [(key, z, scale)])`` with ``z`` every Linear's
    pre-activation (the four in front of a ReLU and the last one) and ``scale = sum_k |W_ok x_k| + |b_o|``, the size of the
    terms z is the sum of."""
    stages = []
    for first in (0, 5):
        for k in (first, first + 2):
            W, b = state[f"layers.{k}.weight"], state[f"layers.{k}.bias"]
            z, scale = row_ref.linear_stage(x, W, b)
            stages.append((f"layers.{k}", z, scale))
            x = F.relu(z)
        ln = first + 4
        x = F.layer_norm(x, x.shape[-1:], state[f"layers.{ln}.weight"], state[f"layers.{ln}.bias"])
    z, scale = row_ref.linear_stage(x, state["layers.10.weight"], state["layers.10.bias"])
    stages.append(("layers.10", z, scale))
    return z * state["layers.11.scale"], stages


def relu_stages(state, x):
    """The ``(z, scale)`` the kink filter judges the rows of ``x`` by: the four ReLU stages, in float64, on the CPU."""
    with torch.no_grad():
        _, stages = walk({k: v.detach().double().cpu() for k, v in state.items()}, x.double().cpu())
    return [(z, scale) for key, z, scale in stages if int(key.split(".")[1]) in RELU_STAGES]


@functools.lru_cache(maxsize=None)
def candidates(variant):
    """``(module, feat, anchor, embed, keep)`` of a variant, on the CPU: the module and the 1 400 candidate rows drawn exactly
    as tests/test_refine_mlp_gpu.py draws them, and which rows the filter keeps (judged on ``feat + embed`` in float64)."""
    cfg, extra = VARIANTS[variant]
    seed = 200 + list(VARIANTS).index(variant)
    module = make_module(cfg, seed)
    feat, anchor, embed = make_inputs(module.output_dim, extra, CANDIDATES, seed + 1000)
    keep = row_ref.kink_free(relu_stages(module.state_dict(), feat.double() + embed.double()))
    return module, feat, anchor, embed, keep


def survivors(variant):
    """``(module, feat, anchor, embed)``: the candidate rows the filter keeps, in their order (float32, CPU)."""
    module, feat, anchor, embed, keep = candidates(variant)
    return module, feat[keep].contiguous(), anchor[keep].contiguous(), embed[keep].contiguous()


def kind(key):
    """The kind of a state_dict leaf, for the parameter gradients' yardsticks."""
    layer, slot = key.split(".")[1:]
    if slot == "scale":
        return "scale"
    if layer in ("4", "9"):
        return "LN " + slot
    if slot == "bias":
        return "Linear bias"
    return "last weight" if layer == "10" else "square weight"


KINDS = ("square weight", "last weight", "Linear bias", "LN weight", "LN bias", "scale")
assert sorted({kind(k) for k in MLP_KEYS}) == sorted(KINDS)
