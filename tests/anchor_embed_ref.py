"""TEST INFRASTRUCTURE: a dtype-generic restatement of ``SparseGaussian3DEncoder.forward``
(model/encoder/gaussian_encoder/anchor_encoder_module.py:38-53 with ``linear_relu_ln``, utils.py:49-59) on a plain mapping of
its state_dict.  In float64 it is the truth the tests hold every path to; in float32 it is what a user of the reference runs
today.  ``fixed_weights`` gives the reproducible parameter sets, so no weights are committed.  Never imported by the product."""
import torch
import torch.nn.functional as F

import row_ref
from row_ref import cast, fixed_input, output_weights  # noqa: F401  (re-exported: the tests reach them as ``ref.``)

STAGES = ("xyz_fc", "scale_fc", "rot_fc", "opacity_fc", "semantics_fc", "output_fc")
# the fixture's families (tools/make_golden_anchor_embed.py): constructor keys of the module, embed_dims = 128
FAMILIES = {
    "opa_s17": dict(include_opa=True, semantics=True, semantic_dim=17),
    "gs144000": dict(include_opa=False, semantics=True, semantic_dim=18),
    "opa_nosem": dict(include_opa=True, semantics=False, semantic_dim=None),
}
GOLDEN_ROWS = 96
# the GPU tests' layouts, name: (include_opa, S, Da)
LAYOUTS = {
    "opa_s17": (1, 17, 28), "gs144000": (0, 18, 28), "opa_s0": (1, 0, 11), "noopa_s0": (0, 0, 10),
    "opa_s1": (1, 1, 12), "opa_s5": (1, 5, 16), "opa_s32": (1, 32, 43), "opa_s17_da40": (1, 17, 40),
}


def shapes(include_opa, S, E=128):
    """``{state_dict key: shape}`` in the module's own order."""
    k_in = {"xyz_fc": 3, "scale_fc": 3, "rot_fc": 4, "opacity_fc": 1 if include_opa else 0, "semantics_fc": S, "output_fc": E}
    order = ["xyz_fc", "scale_fc", "rot_fc"] + (["opacity_fc"] if include_opa else []) + (["semantics_fc"] if S else []) + ["output_fc"]
    out = {}
    for st in order:
        for key, shape in (("0.weight", (E, k_in[st])), ("0.bias", (E,)), ("2.weight", (E,)), ("2.bias", (E,)),
                           ("3.weight", (E, E)), ("3.bias", (E,)), ("5.weight", (E,)), ("5.bias", (E,))):
            out[f"{st}.{key}"] = shape
    return out


def fixed_weights(include_opa=True, S=17, E=128, seed=0, dtype=torch.float32):
    """``row_ref.fixed_weights`` of the module's state_dict (stream offset 0)."""
    return row_ref.fixed_weights(shapes(include_opa, S, E), 0, seed, dtype)


def make_input(n, opa, S, Da, seed):
    """N(0, 1) logits with the planted rows (as many of them as n admits)."""
    x = fixed_input(n, Da, seed)
    ss = 10 + opa
    plant = [lambda r: r.zero_(), lambda r: r.fill_(1e-30),
             lambda r: r[ss:ss + S].fill_(80.0), lambda r: r[ss:ss + S].fill_(-80.0),
             lambda r: r[0:3].fill_(1e4), lambda r: r[0:3].fill_(-1e4)]
    for i, f in enumerate(plant):
        if i < n:
            f(x[i])
    return x


def _stage(x, sd, name):
    E = sd[name + ".0.bias"].shape[0]
    for lin, ln in ((0, 2), (3, 5)):
        x = F.relu(F.linear(x, sd[f"{name}.{lin}.weight"], sd[f"{name}.{lin}.bias"]))
        x = F.layer_norm(x, (E,), sd[f"{name}.{ln}.weight"], sd[f"{name}.{ln}.bias"], 1e-5)
    return x


def anchor_embed_ref(anchor, sd):
    """The forward in ``anchor``'s dtype, on the state_dict ``sd`` of the same dtype and device."""
    opa = 1 if "opacity_fc.0.weight" in sd else 0
    out = _stage(anchor[..., 0:3], sd, "xyz_fc") + _stage(anchor[..., 3:6], sd, "scale_fc") + _stage(anchor[..., 6:10], sd, "rot_fc")
    if opa:
        out = out + _stage(anchor[..., 10:11], sd, "opacity_fc")
    if "semantics_fc.0.weight" in sd:
        S = sd["semantics_fc.0.weight"].shape[1]
        out = out + _stage(anchor[..., 10 + opa:10 + opa + S], sd, "semantics_fc")
    return _stage(out, sd, "output_fc")
