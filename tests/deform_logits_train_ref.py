"""TEST INFRASTRUCTURE for the training step of the deformable block's dense front (``gf_deform_logits_forward`` /
``gf_deform_logits_backward``): ``deform_block_ref.logits_ref`` in a generic dtype on a weight mapping, the
gradients of the fixed scalar ``sum(raw * output_weights) + sum(learned * output_weights)`` through
``row_ref.scalar_gradients``, and seeded weights from ``deform_block_ref``.

The op is linear: there is no kink, no filter, and no row is exempt -- every row of every tensor is judged.  Never imported by
the product."""
import torch

import deform_block_ref as ref
import row_ref
from row_ref import cast, fixed_input, output_weights, planted  # noqa: F401  (re-exported: the tests reach them as ``tr.``)

E = ref.E
# name: (3K, Nw, with anchor_embed) -- tests/test_deform_block_gpu.py's FRONT: the shipped widths (solid; base and prob; the two
# without the camera embedding), both widths on a non-multiple of 32 with a single partial chunk, Nw just past a chunk edge
FRONT = {"solid": (6, 144, True), "base": (18, 208, True), "nocam_solid": (0, 864, True), "nocam_base": (18, 1248, True),
         "narrow": (30, 16, False), "edge": (3, 132, True)}
WL, BL, WW, BW = KEYS = ("kps_generator.learnable_fc.weight", "kps_generator.learnable_fc.bias", "weights_fc.weight",
                         "weights_fc.bias")     # the library's table order
PER_ROW = ("out", "instance_feature", "anchor_embed")


def weights(k3, nw, seed=0, dtype=torch.float32):
    """``{learnable_fc.weight, .bias (with k3), weights_fc.weight, .bias}``: ``deform_block_ref.fixed_weights`` of the dense
    shapes, the front's keys alone."""
    sd = ref.fixed_weights(ref.dense_shapes(k3, nw), seed, dtype)
    return {k: v for k, v in sd.items() if k in KEYS}


def pairs(sd):
    """``(weights_fc, learnable_fc | None)`` as the functions take them."""
    return (sd[WW], sd[BW]), ((sd[WL], sd[BL]) if WL in sd else None)


def logits_train_ref(f, e, sd):
    """The op in ``f``'s dtype on the mapping ``sd``: ``[raw | learned]`` side by side, ``[n, Nw + 3K]`` (``e`` may be ``None``)."""
    raw, learned = ref.logits_ref(f, e, sd[WW], sd[BW], sd.get(WL), sd.get(BL))
    return raw if learned is None else torch.cat([raw, learned], dim=-1)


def cotangent(n, k3, nw, dtype=torch.float64):
    """``output_weights`` on ``raw`` and on ``learned``, side by side as ``logits_train_ref`` lays them."""
    parts = [output_weights((n, nw), dtype)] + ([output_weights((n, k3), dtype)] if k3 else [])
    return torch.cat(parts, dim=-1)


def gradients(forward, f, e, sd):
    """``{"out": [raw | learned], "instance_feature", "anchor_embed" (where given), key: d/d sd[key]}`` of the fixed scalar;
    ``forward(f, e, leaves) -> [raw | learned]`` is the restatement or the native functional."""
    k3, nw = (sd[WL].shape[0] if WL in sd else 0), sd[WW].shape[0]
    cot = cotangent(f.shape[0], k3, nw, f.dtype).to(f.device)
    return row_ref.scalar_gradients(forward, {"instance_feature": f, "anchor_embed": e}, sd, cotangent=cot, with_out=True)


def kind(key):
    """The kind of a leaf, by how its gradient is formed: a weight is a contraction over the rows on the matrix cores, a bias a
    plain sum over the rows of the cotangent."""
    return "weight" if key.endswith("weight") else "bias"
