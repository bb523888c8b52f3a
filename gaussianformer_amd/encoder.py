"""The encoder: drop-in for ``GaussianOccEncoder`` (model/encoder/gaussian_encoder/gaussian_encoder.py:10-123), the module that
walks a config's ``operation_order`` over the anchor encoder, the deformable block, the feed-forward block, the sparse
convolution block, the refinement step and the LayerNorms between them.  Every one of those has a one-launch inference form
that takes the ``"add"`` / ``"norm"`` behind it (``ffn_block``, ``DeformableFeatureAggregation.forward(residual=, norm=)``,
``SparseConv3D.forward(residual=, norm=)``); :func:`plan` turns the runs ``"identity", X, "add", "norm"`` and ``X, "norm"`` of an
order into those calls.  Training folds the same steps with the opt-in ``fold_training``, where a step's
layer has a native training route that takes the add and the norm; without it training, and every call the
fused forms do not cover, walks the order op by op as the reference does."""
import copy
from collections import namedtuple

import torch
import torch.nn as nn

from . import _lib
from .anchor_encoder import SparseGaussian3DEncoder
from .deformable_aggregation import DeformableAggregationFunction as DAF
from .deformable_block import DeformableFeatureAggregation
from .ffn import AsymmetricFFN, ffn_block, ffn_block_autograd
from .refine import SparseGaussian3DRefinementModule, SparseGaussian3DRefinementModuleV2
from .sparse_conv import SparseConv3D, SubMConv3d

# the drop-ins a config dict's ``type`` may name
MODULES = {cls.__name__: cls for cls in (SparseGaussian3DEncoder, AsymmetricFFN, DeformableFeatureAggregation,
                                         SparseGaussian3DRefinementModule, SparseGaussian3DRefinementModuleV2, SparseConv3D)}
ABSORBING = ("deformable", "ffn", "spconv")

# One step of a plan.  ``op``: the name in the order, ``index``: its position there (``layers[index]`` is its module), ``add``:
# the ``"add"`` at ``index + 1`` is part of the step (its residual is the running ``identity``), ``norm``: the position of the
# ``"norm"`` that is part of the step, or ``None``.  A step that absorbed nothing has ``add = False, norm = None``.
Step = namedtuple("Step", "op index add norm")


def _known(op):
    return op in ("spconv", "norm", "ffn", "identity", "add", "deformable") or "refine" in op


def plan(operation_order, layers=None):
    """The steps of ``operation_order``, a pure function of the order and of each deformable block's ``residual_mode``
    (``layers[i]``; without ``layers`` every block is taken to absorb).  After an op ``X`` of ``"deformable"``, ``"ffn"`` or
    ``"spconv"`` the step takes an immediately following ``"add"`` if an ``"identity"`` comes earlier in the order, then an
    immediately following ``"norm"``; a deformable block with ``residual_mode == "cat"`` takes nothing (its output is 256 wide
    and the library's output launch has no add or norm behind a cat).  Every other op is a step of its own.  An op the
    reference's loop does not know raises its ``NotImplementedError`` here, when the plan is made."""
    order = list(operation_order)
    for op in order:
        if not _known(op):
            raise NotImplementedError(f"{op} is not supported.")
    steps, i, seen_identity = [], 0, False
    while i < len(order):
        op = order[i]
        add, norm, nxt = False, None, i + 1
        cat = op == "deformable" and layers is not None and getattr(layers[i], "residual_mode", None) == "cat"
        if op in ABSORBING and not cat:
            if nxt < len(order) and order[nxt] == "add" and seen_identity:
                add, nxt = True, nxt + 1
            if nxt < len(order) and order[nxt] == "norm":
                norm, nxt = nxt, nxt + 1
        if op == "identity":
            seen_identity = True
        steps.append(Step(op, i, add, norm))
        i = nxt
    return steps


def build_module(cfg, default_type=None):
    """A module from a config dict whose ``type`` names one of this package's drop-ins (``MODULES``) or, for a norm layer,
    ``"LN"``; a module instance is deep-copied; ``None`` stays ``None``."""
    if cfg is None:
        return None
    if isinstance(cfg, nn.Module):
        return copy.deepcopy(cfg)
    cfg = copy.deepcopy(dict(cfg))     # (the constructors may write into their config: kps_generator["embed_dims"])
    kind = cfg.pop("type", default_type)
    if kind == "LN":
        cfg.pop("requires_grad", None)
        return nn.LayerNorm(**cfg)
    if kind not in MODULES:
        raise ValueError(f"GaussianOccEncoder: no drop-in for a module of type {kind!r} (known: {sorted(MODULES)} and 'LN')")
    return MODULES[kind](**cfg)


def _formatted(feature_maps):
    return isinstance(feature_maps, (tuple, list)) and len(feature_maps) == 3 and feature_maps[1].dim() == 2


class GaussianOccEncoder(nn.Module):
    """Same constructor keys and defaults, ``operation_order`` default, ``layers`` (an ``nn.ModuleList`` in the order's order,
    ``None`` for ``"identity"`` and ``"add"``), ``state_dict`` keys (``anchor_encoder.*``, ``layers.{i}.*``), ``init_weights()``
    and ``forward(representation, rep_features, ms_img_feats, metas) -> {"representation": [{"gaussian": ...}, ...]}`` as the
    reference class (gaussian_encoder.py:10-123); built without mmengine: each module argument is a config dict whose ``type``
    names a drop-in of this package (built once per occurrence in the order, as there), or a module (deep-copied per
    occurrence).

    ``ms_img_feats``: a tensor, the list of pyramid levels, or an already formatted ``(table, spatial_shape,
    scale_start_index)`` triple; a list is formatted once per call and handed to every deformable block.

    ``fold`` is a class attribute, not a constructor key and not part of the ``state_dict``.  With it, in eval mode, on fp32 GPU
    inputs and with nothing that needs autograd, the call runs the steps of :func:`plan`: one fused call per step.  Every
    other call, training included, walks the order op by op on each module's own route.

    ``fold_training`` is likewise a class attribute, off by default (``set_native(fold_training=True)`` sets it on the instance).
    With it a call in train mode or one that needs autograd, on fp32 GPU inputs, runs the steps of :func:`plan` too: a step that
    absorbed an ``"add"`` or a ``"norm"`` is one call where its layer's own native training route takes them -- a deformable
    block with ``native_training`` or a sparse block with ``native_training`` and ``native_tail_training`` (``residual=`` /
    ``norm=``), an ``AsymmetricFFN`` with ``native_training``
    and no active ``dropout_layer`` (``ffn_block_autograd`` with the module's dropout probabilities) -- and the same ops one by
    one otherwise.  The random draws come in the unfolded route's order."""

    fold = True
    fold_training = False

    def __init__(self, anchor_encoder, norm_layer, ffn, deformable_model, refine_layer, mid_refine_layer=None, spconv_layer=None,
                 num_decoder=6, operation_order=None, init_cfg=None, **kwargs):
        super().__init__()
        self.init_cfg = init_cfg
        self.num_decoder = num_decoder
        if operation_order is None:
            operation_order = ["spconv", "norm", "deformable", "norm", "ffn", "norm", "refine"] * num_decoder
        self.operation_order = list(operation_order)
        self.anchor_encoder = anchor_encoder if isinstance(anchor_encoder, nn.Module) else build_module(anchor_encoder)
        self.op_config_map = {"norm": norm_layer, "ffn": ffn, "deformable": (deformable_model, "DeformableFeatureAggregation"),
                              "refine": refine_layer, "mid_refine": mid_refine_layer, "spconv": spconv_layer}
        layers = []
        for op in self.operation_order:
            cfg = self.op_config_map.get(op)
            cfg, default = cfg if isinstance(cfg, tuple) else (cfg, None)
            layers.append(build_module(cfg, default))
        self.layers = nn.ModuleList(layers)
        self.steps = plan(self.operation_order, self.layers)

    def init_weights(self):
        for i, op in enumerate(self.operation_order):
            if self.layers[i] is None:
                continue
            elif op != "refine":
                for p in self.layers[i].parameters():
                    if p.dim() > 1:
                        nn.init.xavier_uniform_(p)
        for m in self.modules():
            if hasattr(m, "init_weight"):
                m.init_weight()

    def set_native(self, training=None, fused_mlp=None, fold_training=None, front_training=None):
        """Sets ``native_training`` / ``fused_mlp`` on every submodule that has the attribute (``None``: left alone); returns
        ``self``.  Their defaults do not change.  ``native_training`` is an attribute of the anchor encoder, the feed-forward
        block, the refinement modules, the deformable block (its back end) and the sparse convolution block
        (``SparseConv3D``: its LayerNorm stages).  ``fold_training`` sets this encoder's attribute of that name
        and ``native_tail_training`` on every submodule that has it (``SparseConv3D``: the tail that takes the block's add and
        norm in training); ``training=`` touches neither.  ``front_training`` sets ``native_front_training`` on
        every submodule that has it (the deformable block's dense front) and nothing else; ``training=`` and
        ``fold_training=`` do not touch it."""
        if fold_training is not None:
            self.fold_training = bool(fold_training)
        for m in self.modules():
            if fold_training is not None and hasattr(m, "native_tail_training"):
                m.native_tail_training = bool(fold_training)
            if training is not None and hasattr(m, "native_training"):
                m.native_training = bool(training)
            if front_training is not None and hasattr(m, "native_front_training"):
                m.native_front_training = bool(front_training)
            if fused_mlp is not None and hasattr(m, "fused_mlp"):
                m.fused_mlp = bool(fused_mlp)
        return self

    @staticmethod
    def _fold_inputs(anchor, instance_feature, feature_maps):
        """The inputs both folds look at -- the two tensors and the feature maps (a formatted triple's table) -- or ``None``
        unless every one of them is an fp32 GPU tensor."""
        maps = [] if feature_maps is None else [feature_maps[0]] if _formatted(feature_maps) else list(feature_maps)
        tensors = [anchor, instance_feature, *maps]
        if not all(isinstance(t, torch.Tensor) for t in tensors) or not _lib.native_tensors(tensors):
            return None
        return tensors

    def _folds(self, anchor, instance_feature, feature_maps):
        if not self.fold or self.training:
            return False
        tensors = self._fold_inputs(anchor, instance_feature, feature_maps)
        return tensors is not None and not _lib.needs_grad([*tensors, *self.parameters()])

    def _folds_training(self, anchor, instance_feature, feature_maps):
        if not self.fold_training:
            return False
        tensors = self._fold_inputs(anchor, instance_feature, feature_maps)
        return tensors is not None and (self.training or _lib.needs_grad([*tensors, *self.parameters()]))

    def forward(self, representation, rep_features, ms_img_feats=None, metas=None, **kwargs):
        feature_maps = ms_img_feats
        if isinstance(feature_maps, torch.Tensor):
            feature_maps = [feature_maps]
        instance_feature = rep_features
        anchor = representation
        fold = self._folds(anchor, instance_feature, feature_maps)
        fold_training = not fold and self._folds_training(anchor, instance_feature, feature_maps)
        if feature_maps is not None and not _formatted(feature_maps) and "deformable" in self.operation_order:
            feature_maps = DAF.feature_maps_format(list(feature_maps))    # once, not in every block
        anchor_embed = self.anchor_encoder(anchor)
        identity = None
        prediction = []
        last = len(self.operation_order) - 1
        steps = self.steps if fold or fold_training else [Step(op, i, False, None) for i, op in enumerate(self.operation_order)]
        for step in steps:
            op, i = step.op, step.index
            layer = self.layers[i]
            norm = None if step.norm is None else self.layers[step.norm]
            residual = identity if step.add else None
            fused = step.add or norm is not None
            folds = self._step_folds_training if fold_training else self._step_folds
            if fused and not folds(op, layer, instance_feature, anchor, anchor_embed, feature_maps, residual, norm):
                # the fused call would refuse this configuration: the same ops one by one
                instance_feature = self._one(op, layer, instance_feature, anchor, anchor_embed, feature_maps, metas)
                if step.add:
                    instance_feature = instance_feature + identity
                if norm is not None:
                    instance_feature = norm(instance_feature)
            elif fused and op == "ffn" and fold_training:
                p_hidden, p_out = (layer.layers[0][2].p, layer.layers[2].p) if layer.training else (0.0, 0.0)
                instance_feature = ffn_block_autograd(instance_feature, layer, norm, residual, p_hidden, p_out)
            elif fused and op == "ffn":
                instance_feature = ffn_block(instance_feature, layer, norm, residual)
            elif fused and op == "deformable":
                instance_feature = layer(instance_feature, anchor, anchor_embed, feature_maps, metas, residual=residual, norm=norm)
            elif fused:
                instance_feature = layer(instance_feature, anchor, residual=residual, norm=norm)
            elif op == "identity":
                identity = instance_feature
            elif op == "add":
                instance_feature = instance_feature + identity
            elif "refine" in op:
                anchor, gaussian = layer(instance_feature, anchor, anchor_embed)
                prediction.append({"gaussian": gaussian})
                if i != last:
                    anchor_embed = self.anchor_encoder(anchor)
            else:
                instance_feature = self._one(op, layer, instance_feature, anchor, anchor_embed, feature_maps, metas)
        return {"representation": prediction}

    @staticmethod
    def _one(op, layer, instance_feature, anchor, anchor_embed, feature_maps, metas):
        """One of the reference loop's module calls (:92-109)."""
        if op == "spconv":
            return layer(instance_feature, anchor)
        if op == "deformable":
            return layer(instance_feature, anchor, anchor_embed, feature_maps, metas)
        return layer(instance_feature)     # "norm", "ffn"

    @staticmethod
    def _step_folds(op, layer, instance_feature, anchor, anchor_embed, feature_maps, residual, norm):
        """Whether the step's fused call takes this configuration: the checks the callee makes, asked instead of caught.  The
        deformable block and the sparse block ask them themselves -- a call of theirs with ``residual=`` / ``norm=`` that their
        native route does not cover runs their torch layers with the add and the norm behind them, the same ops in the same
        order -- so only their type is looked at here; ``ffn_block`` has no such route and is asked in full."""
        if op == "deformable":
            return isinstance(layer, DeformableFeatureAggregation) and feature_maps is not None
        if op == "spconv":
            return isinstance(layer, SparseConv3D)
        if not _lib.norm_native(norm) or not isinstance(layer, AsymmetricFFN) or not layer._native(instance_feature, None):
            return False
        if layer.add_identity and isinstance(layer.identity_fc, nn.Identity):
            return False
        return layer.pre_norm is None or isinstance(layer.pre_norm, nn.LayerNorm)

    @classmethod
    def _step_folds_training(cls, op, layer, instance_feature, anchor, anchor_embed, feature_maps, residual, norm):
        """``_step_folds`` for a training call: whether the layer's own native training route takes the step's add and norm.
        The deformable block and the sparse block are asked what their ``forward`` asks (a call that needs no autograd
        after all is their inference route's); the feed-forward block must have ``native_training``, no active
        ``dropout_layer`` and dropout probabilities below 1, as its own ``forward`` requires."""
        if not getattr(layer, "native_training", False):
            return False
        if op == "deformable":
            if not isinstance(layer, DeformableFeatureAggregation) or feature_maps is None:
                return False
            args = (instance_feature, anchor, anchor_embed, feature_maps[0], residual, norm)
            return layer._native_training(*args) or layer._native(*args)
        if op == "spconv":
            if not isinstance(layer, SparseConv3D):
                return False
            args = (instance_feature, anchor, residual, norm)
            if layer._native_tail(*args):
                return True
            return layer._native_training(*args) and (layer._tail_training(norm) or isinstance(layer.layer, SubMConv3d))
        if not cls._step_folds(op, layer, instance_feature, anchor, anchor_embed, feature_maps, residual, norm):
            return False
        if not isinstance(norm, (nn.LayerNorm, type(None))):
            return False
        if layer.training and isinstance(layer.dropout_layer, nn.Dropout) and layer.dropout_layer.p > 0:
            return False
        return not layer.training or (layer.layers[0][2].p < 1.0 and layer.layers[2].p < 1.0)
