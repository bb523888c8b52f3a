"""TEST INFRASTRUCTURE: a dtype-generic restatement of the encoder's feed-forward block -- ``AsymmetricFFN.forward``
(model/encoder/gaussian_encoder/ffn_module.py:66-75) in eval mode, then the ``"add"`` and ``"norm"`` that follow it in the
encoder's ``operation_order`` -- on a plain mapping of the module's state_dict.  In float64 it is the truth the tests hold
every path to; in float32 it is what a user of the reference runs today.  ``fixed_weights`` gives the reproducible parameter
sets, so no weights are committed.  Never imported by the product."""
import numpy as np
import torch
import torch.nn.functional as F

from anchor_embed_ref import _uniform, cast  # noqa: F401  (the same reproducible hash; cast is re-exported)

E, HIDDEN = 128, 512
# the fixture's families (tools/make_golden_ffn.py): the constructor arguments of the two shipped config families
# (base: _base_/model.py:62-71 merged into nuscenes_gs25600_solid.py:116-121; prob: prob/nuscenes_gs*.py:161-169), and what
# follows the ffn in their operation_order
FAMILIES = {
    "base": dict(in_channels=256, pre_norm=dict(type="LN"), embed_dims=128, feedforward_channels=512, num_fcs=2,
                 act_cfg=dict(type="ReLU", inplace=True), ffn_drop=0.1),
    "prob": dict(embed_dims=128, feedforward_channels=512, ffn_drop=0.1, add_identity=False),
}
FOLLOWED_BY_ADD = {"base": False, "prob": True}
GOLDEN_ROWS = 64
NORM_KEYS = ("norm.weight", "norm.bias")   # the post norm's place in a weight mapping (not part of the module's state_dict)


def shapes(cin=256, pre_norm=True, identity=True, norm=True, e=E, f=HIDDEN):
    """``{key: shape}``: the module's state_dict in its own order, then the post norm's pair."""
    out = {}
    if pre_norm:
        out["pre_norm.weight"] = (cin,)
        out["pre_norm.bias"] = (cin,)
    out["layers.0.0.weight"] = (f, cin)
    out["layers.0.0.bias"] = (f,)
    out["layers.1.weight"] = (e, f)
    out["layers.1.bias"] = (e,)
    if identity:
        out["identity_fc.weight"] = (e, cin)
        out["identity_fc.bias"] = (e,)
    if norm:
        out["norm.weight"] = (e,)
        out["norm.bias"] = (e,)
    return out


def family_shapes(name):
    return shapes(256, True, True) if name == "base" else shapes(128, False, False)


def fixed_weights(cin=256, pre_norm=True, identity=True, norm=True, e=E, f=HIDDEN, seed=0, dtype=torch.float32):
    """A seeded weight mapping away from the initial state: Linear weights uniform with variance 1 / fan_in, biases of +-0.3,
    LayerNorm weights in [0.7, 1.3] and biases of +-0.3 (computed in float64, rounded once to float32, then cast)."""
    sd = {}
    for i, (key, shape) in enumerate(shapes(cin, pre_norm, identity, norm, e, f).items()):
        u = _uniform(int(np.prod(shape)), 1000 * seed + 500 + i).reshape(shape)
        if len(shape) == 2:
            v = u * np.sqrt(3.0 / shape[1])
        elif key.endswith("weight") and ("norm" in key):
            v = 1.0 + 0.3 * u
        else:
            v = 0.3 * u
        sd[key] = torch.from_numpy(v.astype(np.float32)).to(dtype)
    return sd


def module_state(sd):
    """The module's part of a weight mapping (without the post norm's pair): what ``load_state_dict`` takes."""
    return {k: v for k, v in sd.items() if k not in NORM_KEYS}


def ffn_ref(x, sd, residual=None, norm=True, act=F.relu):
    """The block in ``x``'s dtype on the mapping ``sd`` of the same dtype and device: the FFN, ``+ residual`` where given, the
    post norm where ``norm`` and the mapping has one."""
    u = x
    if "pre_norm.weight" in sd:
        u = F.layer_norm(x, (x.shape[-1],), sd["pre_norm.weight"], sd["pre_norm.bias"], 1e-5)
    y = F.linear(act(F.linear(u, sd["layers.0.0.weight"], sd["layers.0.0.bias"])), sd["layers.1.weight"], sd["layers.1.bias"])
    if "identity_fc.weight" in sd:
        y = F.linear(u, sd["identity_fc.weight"], sd["identity_fc.bias"]) + y
    if residual is not None:
        y = y + residual
    if norm and "norm.weight" in sd:
        y = F.layer_norm(y, (y.shape[-1],), sd["norm.weight"], sd["norm.bias"], 1e-5)
    return y


def fixed_input(n, cin, seed):
    """N(0, 1) rows [n, cin], float32."""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, cin)).astype(np.float32))


def planted(x):
    """Rows that a random draw does not reach (as many as ``x`` has room for): zeros, tiny, +-1e4 in a few columns."""
    x = x.clone()
    plant = [lambda r: r.zero_(), lambda r: r.fill_(1e-30), lambda r: r[3:6].fill_(1e4), lambda r: r[40:43].fill_(-1e4)]
    for i, f in enumerate(plant):
        if i < x.shape[0]:
            f(x[i])
    return x
