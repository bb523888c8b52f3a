"""TEST INFRASTRUCTURE for the training step of the deformable block's dense back (``gf_deform_output_forward_train`` /
``gf_deform_output_backward``): ``deform_block_ref.output_ref`` in a generic dtype on a weight mapping, the
gradients of the fixed scalar ``sum(out * output_weights)`` through ``row_ref.scalar_gradients``, seeded weights from
``row_ref``, and the sparse block's restatement (``subm_stage_ref.block``) under the names the tests judge it by.

The op has no ReLU: there is no kink, no filter, and no row is exempt -- every row of every tensor is judged.  Never imported
by the product."""
import torch

import deform_block_ref as ref
import row_ref
import subm_stage_ref
from row_ref import cast, fixed_input, output_weights, planted  # noqa: F401  (re-exported: the tests reach them as ``tr.``)

E = ref.E
# name: (residual_mode, residual, post norm) -- the five variants of the output launch
VARIANTS = {"none": ("none", False, False), "add": ("add", False, False), "cat": ("cat", False, False),
            "none_res_norm": ("none", True, True), "add_norm": ("add", False, True)}
PER_ROW = ("out", "features", "instance_feature", "residual")
KEYS = ("output_proj.weight", "output_proj.bias", "norm.weight", "norm.bias")     # the library's table order


def weights(norm, seed=0, dtype=torch.float32):
    """``{output_proj.weight, .bias[, norm.weight, .bias]}``: seeded, away from the initial state (``row_ref.fixed_weights``)."""
    shapes = {"output_proj.weight": (E, E), "output_proj.bias": (E,)}
    if norm:
        shapes.update({"norm.weight": (E,), "norm.bias": (E,)})
    return row_ref.fixed_weights(shapes, 900, seed, dtype)


def norm_of(sd):
    return (sd["norm.weight"], sd["norm.bias"]) if "norm.weight" in sd else None


def output_train_ref(features, instance_feature, residual, sd, mode):
    """The op in ``features``' dtype on the mapping ``sd`` (``instance_feature`` is ``None`` with ``"none"``)."""
    return ref.output_ref(features, sd["output_proj.weight"], sd["output_proj.bias"], instance_feature, mode, residual, norm_of(sd))


def gradients(forward, features, instance_feature, residual, sd):
    """``{"out", "features", "instance_feature", "residual" (where given), key: d/d sd[key]}`` of ``sum(forward(features,
    instance_feature, residual, leaves) * output_weights)``; ``forward`` is the restatement or the native functional."""
    inputs = {"features": features, "instance_feature": instance_feature, "residual": residual}
    return row_ref.scalar_gradients(forward, inputs, sd, with_out=True)


def kind(key):
    """The kind of a leaf, by how its gradient is formed: ``output_proj.weight`` is a contraction over the rows on the matrix
    cores, the three vectors are plain sums over the rows of a per-row quantity."""
    return "matrix" if key == "output_proj.weight" else "vector"


def sparse_block_gradients(x, residual, leaves, idx, batch, shape, K, masks, rep=None, dtype=torch.float64):
    """``subm_stage_ref.block_gradients``: the float64 truth of a sparse block whose tail -- ``output_proj`` (``proj.*``), the
    residual and the post norm (``norm.*``) -- is the op above; ``masks``: the native stages' ReLU masks (``None`` for a
    single-layer block)."""
    return subm_stage_ref.block_gradients(x, residual, leaves, idx, batch, shape, K, masks, rep, dtype)
