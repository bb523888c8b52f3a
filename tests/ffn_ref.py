"""TEST INFRASTRUCTURE: a dtype-generic restatement of the encoder's feed-forward block -- ``AsymmetricFFN.forward``
(model/encoder/gaussian_encoder/ffn_module.py:66-75) in eval mode, then the ``"add"`` and ``"norm"`` that follow it in the
encoder's ``operation_order`` -- on a plain mapping of the module's state_dict.  In float64 it is the truth the tests hold
every path to; in float32 it is what a user of the reference runs today.  ``fixed_weights`` gives the reproducible parameter
sets, so no weights are committed.  Never imported by the product."""
import torch
import torch.nn.functional as F

import row_ref
from row_ref import NORM_KEYS, cast, fixed_input, module_state, planted  # noqa: F401  (re-exported: the tests reach them as ``ref.``)

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
# the GPU tests' variants, name: (Cin, pre_norm, identity_fc, residual, post norm)
VARIANTS = {
    "base_norm": (256, True, True, False, True),
    "base": (256, True, True, False, False),
    "prob_add_norm": (128, False, False, True, True),
    "prob": (128, False, False, False, False),
    "c256_nopre_id": (256, False, True, False, True),
    "c128_pre": (128, True, False, False, True),
}


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
    """``row_ref.fixed_weights`` of the block's weight mapping (stream offset 500)."""
    return row_ref.fixed_weights(shapes(cin, pre_norm, identity, norm, e, f), 500, seed, dtype)


def parts(sd):
    """A weight mapping as ``ffn_block`` takes it: the module's part, and the post norm's pair or ``None``."""
    return module_state(sd), ((sd["norm.weight"], sd["norm.bias"]) if "norm.weight" in sd else None)


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
