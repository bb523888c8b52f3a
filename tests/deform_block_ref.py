"""TEST INFRASTRUCTURE: a dtype-generic restatement of the deformable block's dense ends and of the whole module body --
``DeformableFeatureAggregation.forward`` (model/encoder/gaussian_encoder/deformable_module.py:146-262) in eval mode, then the
``"add"`` and ``"norm"`` that may follow it in the encoder's ``operation_order`` -- on a plain mapping of the module's
state_dict.  The middle (key points, projection, masked softmax, bilinear sampling, the sum over the key points) is
oracle/daf_prepare_ref.py's and tests/daf_fused_ref.py's.  In float64 it is the truth the tests hold every path to; in float32
it is what a user of the reference runs today.  ``fixed_weights`` gives the reproducible parameter sets, so no weights are
committed.  Never imported by the product."""
import torch
import torch.nn.functional as F

import daf_fused_ref
import row_ref
from oracle import daf_prepare_ref
from row_ref import NORM_KEYS, cast, fixed_input, module_state, planted  # noqa: F401  (re-exported: the tests reach them as ``ref.``)

E = 128
FIX7 = [[0, 0, 0], [0.45, 0, 0], [-0.45, 0, 0], [0, 0.45, 0], [0, -0.45, 0], [0, 0, 0.45], [0, 0, -0.45]]
# the configuration tests/golden/caller_dfa.npz was recorded with (tools/make_golden_callers.py; tests/test_ref_callers.py:231-258)
FIXTURE_CONFIG = dict(embed_dims=32, num_groups=4, num_levels=3, num_cams=3, use_deformable_func=True, use_camera_embed=True,
                      residual_mode="cat",
                      kps_generator=dict(type="SparseGaussian3DKeyPointsGenerator", num_learnable_pts=2, fix_scale=FIX7,
                                         pc_range=[-20.0, -20.0, -2.0, 20.0, 20.0, 4.0], scale_range=[0.08, 0.64]))


def logits_ref(f, e, ww, bw, wl=None, bl=None):
    """The front: ``(raw [..., Nw], learned [..., 3K] | None)``; ``e`` may be ``None`` (:59-63, :250-262)."""
    raw = F.linear(f if e is None else f + e, ww, bw)
    return raw, None if wl is None else F.linear(f, wl, bl)


def output_ref(x, wo, bo, f=None, mode="add", residual=None, norm=None):
    """The back: ``output_proj``, the block's residual mode, then ``+ residual`` and the post norm ``(weight, bias)`` where
    given (:243-248)."""
    y = F.linear(x, wo, bo)
    if mode == "add":
        y = y + f
    elif mode == "cat":
        y = torch.cat([y, f], dim=-1)
    if residual is not None:
        y = y + residual
    if norm is not None:
        y = F.layer_norm(y, (y.shape[-1],), norm[0], norm[1], 1e-5)
    return y


def shapes(cfg, norm=False):
    """``{key: shape}``: the module's state_dict in its own order for the constructor arguments ``cfg``, then the post norm's pair."""
    e, k = cfg["embed_dims"], cfg["kps_generator"].get("num_learnable_pts", 0)
    pts = len(cfg["kps_generator"].get("fix_scale") or [[0, 0, 0]]) + k
    out = {}
    if k:
        out["kps_generator.learnable_fc.weight"] = (3 * k, e)
        out["kps_generator.learnable_fc.bias"] = (3 * k,)
    out["output_proj.weight"] = (e, e)
    out["output_proj.bias"] = (e,)
    nw = cfg["num_groups"] * cfg["num_levels"] * pts
    if cfg.get("use_camera_embed"):
        for i, shape in ((0, (e, 12)), (2, (e,)), (3, (e, e)), (5, (e,))):
            out[f"camera_encoder.{i}.weight"] = shape
            out[f"camera_encoder.{i}.bias"] = (e,)
    else:
        nw *= cfg["num_cams"]
    out["weights_fc.weight"] = (nw, e)
    out["weights_fc.bias"] = (nw,)
    if norm:
        out["norm.weight"] = (e,)
        out["norm.bias"] = (e,)
    return out


def fixed_weights(shape_map, seed=0, dtype=torch.float32):
    """``row_ref.fixed_weights`` of ``{key: shape}`` (stream offset 700; the LayerNorms: camera_encoder.2 / .5, norm)."""
    return row_ref.fixed_weights(shape_map, 700, seed, dtype)


def dense_shapes(k3, nw, norm=False):
    """The two kernels' parameters alone, under the module's keys."""
    out = {}
    if k3:
        out["kps_generator.learnable_fc.weight"] = (k3, E)
        out["kps_generator.learnable_fc.bias"] = (k3,)
    out.update({"output_proj.weight": (E, E), "output_proj.bias": (E,), "weights_fc.weight": (nw, E), "weights_fc.bias": (nw,)})
    if norm:
        out.update({"norm.weight": (E,), "norm.bias": (E,)})
    return out


def camera_embed(sd, pm, cams):
    """``camera_encoder`` (linear_relu_ln(E, 1, 2, 12)) on the projection matrices' first three rows (:254-258)."""
    x = pm[:, :, :3].reshape(pm.shape[0], cams, -1)
    for i in (0, 3):
        x = F.relu(F.linear(x, sd[f"camera_encoder.{i}.weight"], sd[f"camera_encoder.{i}.bias"]))
        x = F.layer_norm(x, (x.shape[-1],), sd[f"camera_encoder.{i + 2}.weight"], sd[f"camera_encoder.{i + 2}.bias"], 1e-5)
    return x


def module_ref(sd, cfg, inst, anchor, emb, maps, pm, wh, residual=None, middle=None):
    """The module's forward in ``inst``'s dtype on the mapping ``sd``: ``maps`` the pyramid levels ``[bs, cams, C, h, w]``;
    ``middle(key_points, raw [bs, A, cams, L, pts, G]) -> features [bs, A, C]`` replaces the sampling middle (default: the
    restatement of tests/daf_fused_ref.py in the same dtype).  The post norm is applied where ``sd`` has one."""
    gen = cfg["kps_generator"]
    bs, A = inst.shape[:2]
    cams, L, G = cfg["num_cams"], cfg["num_levels"], cfg["num_groups"]
    kp = daf_prepare_ref.key_points(anchor, inst, gen.get("fix_scale") or [[0.0, 0.0, 0.0]], sd.get("kps_generator.learnable_fc.weight"),
                                    sd.get("kps_generator.learnable_fc.bias"), gen["pc_range"], gen["scale_range"],
                                    gen.get("learnable_fixed_scale", 1))
    pts = kp.shape[2]
    feature = inst + emb
    if cfg.get("use_camera_embed"):
        feature = feature[:, :, None] + camera_embed(sd, pm, cams)[:, None]
        raw = F.linear(feature, sd["weights_fc.weight"], sd["weights_fc.bias"]).reshape(bs, A, cams, L, pts, G)
    else:
        raw = F.linear(feature, sd["weights_fc.weight"], sd["weights_fc.bias"]).reshape(bs, A, cams, L, pts, G)
    feats = middle(kp, raw) if middle is not None else daf_fused_ref.block(kp, pm, wh, maps, raw)
    norm = (sd["norm.weight"], sd["norm.bias"]) if "norm.weight" in sd else None
    return output_ref(feats, sd["output_proj.weight"], sd["output_proj.bias"], inst, cfg.get("residual_mode", "add"), residual, norm)
