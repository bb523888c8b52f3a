"""TEST INFRASTRUCTURE: a dtype-generic restatement of ``SparseGaussian3DEncoder.forward``
(model/encoder/gaussian_encoder/anchor_encoder_module.py:38-53 with ``linear_relu_ln``, utils.py:49-59) on a plain mapping of
its state_dict.  In float64 it is the truth the tests hold every path to; in float32 it is what a user of the reference runs
today.  ``fixed_weights`` gives the reproducible parameter sets, so no weights are committed.  Never imported by the product."""
import numpy as np
import torch
import torch.nn.functional as F

STAGES = ("xyz_fc", "scale_fc", "rot_fc", "opacity_fc", "semantics_fc", "output_fc")
# the fixture's families (tools/make_golden_anchor_embed.py): constructor keys of the module, embed_dims = 128
FAMILIES = {
    "opa_s17": dict(include_opa=True, semantics=True, semantic_dim=17),
    "gs144000": dict(include_opa=False, semantics=True, semantic_dim=18),
    "opa_nosem": dict(include_opa=True, semantics=False, semantic_dim=None),
}
GOLDEN_ROWS = 96


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


def _uniform(count, stream):
    """``count`` values in [-1, 1) from an integer hash of (index, stream): exactly reproducible, no generator state."""
    m = np.uint64(0xFFFFFFFF)
    x = (np.arange(count, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(stream) * np.uint64(40503) + np.uint64(12345)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(3266489917)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.float64) / 2.0 ** 31 - 1.0


def fixed_weights(include_opa=True, S=17, E=128, seed=0, dtype=torch.float32):
    """A seeded state_dict away from the initial state: Linear weights uniform with variance 1 / fan_in, biases of +-0.3,
    LayerNorm weights in [0.7, 1.3] and biases of +-0.3 (computed in float64, rounded once to float32, then cast)."""
    sd = {}
    for i, (key, shape) in enumerate(shapes(include_opa, S, E).items()):
        u = _uniform(int(np.prod(shape)), 1000 * seed + i).reshape(shape)
        if len(shape) == 2:
            v = u * np.sqrt(3.0 / shape[1])
        elif key.endswith("weight"):
            v = 1.0 + 0.3 * u
        else:
            v = 0.3 * u
        sd[key] = torch.from_numpy(v.astype(np.float32)).to(dtype)
    return sd


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


def cast(sd, dtype=None, device=None):
    return {k: v.to(dtype=dtype, device=device) for k, v in sd.items()}


def fixed_input(n, Da, seed):
    """N(0, 1) rows [n, Da], float32."""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, Da)).astype(np.float32))


def output_weights(shape, dtype=torch.float64):
    """The fixed weights of the scalar that gradients come from: cos(0.37 i) over the output's elements."""
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.37).reshape(shape).to(dtype)
