"""The deformable block: drop-in for ``DeformableFeatureAggregation`` (model/encoder/gaussian_encoder/deformable_module.py:
93-262) and the native form of its dense ends.  The middle of the block was native already (``key_points``,
``deformable_fused_forward`` / ``deformable_fused``); its ends ran as torch layers wherever the block was assembled:
``kps_generator.learnable_fc`` and ``weights_fc`` on ``instance_feature + anchor_embed`` before the sampling, ``output_proj``
with the add or the cat behind it.  ``gf_deform_logits_forward`` and ``gf_deform_output_forward`` (include/gf_hip.h, DESIGN.md
§3.13e) are one launch each: an inference block is four launches and the ``[A, 128]`` sum never reaches memory.  The back end has
a native training step as well (``deformable_output_autograd``: ``gf_deform_output_forward_train`` / ``gf_deform_output_backward``,
DESIGN.md §3.13f), which the module takes with the opt-in ``native_training``, and so has the front end
(``deformable_logits_autograd``: ``gf_deform_logits_forward`` / ``gf_deform_logits_backward``) with the opt-in
``native_front_training``; without them training, dropout and everything the native ops do not cover run the module's own
torch layers around ``deformable_fused``."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .deformable_aggregation import DeformableAggregationFunction as DAF
from .deformable_prepare import deformable_fused, deformable_fused_forward
from .key_points import SparseGaussian3DKeyPointsGenerator, key_points

f32 = torch.float32
E_NATIVE, MAX_LEARNED = _lib.GF_DEFORM_EMBED_DIMS, _lib.GF_DEFORM_MAX_LEARNED
MODES = {"none": _lib.GF_DEFORM_NONE, "add": _lib.GF_DEFORM_ADD, "cat": _lib.GF_DEFORM_CAT}


def _pair(layer, what):
    """``(weight, bias)`` of an ``nn.Linear`` or of a pair; ``(None, None)`` for ``None``."""
    if layer is None:
        return None, None
    if isinstance(layer, nn.Module):
        if not isinstance(layer, nn.Linear) or layer.weight is None or layer.bias is None:
            raise ValueError(f"{what} is a {type(layer).__name__} without weight and bias, not an Linear with both")
        return layer.weight, layer.bias
    weight, bias = layer
    return weight, bias


def _refuse_autograd(name, tensors):
    _lib.refuse_autograd(name, tensors, "(the DeformableFeatureAggregation module routes training to its torch layers around "
                         "deformable_fused)")


def _logits_args(weights_fc, learnable_fc):
    """``(ww, bw, wl, bl)`` of a logits call, the pairs checked (``wl``, ``bl``: ``None`` without ``learnable_fc``)."""
    ww, bw = _pair(weights_fc, "weights_fc")
    wl, bl = _pair(learnable_fc, "learnable_fc")
    return ww, bw, wl, bl


def _logits_shapes(name, instance_feature, anchor_embed, ww, bw, wl, bl):
    """``(f [n, E], e [n, E] | None, leading shape, E, K3, Nw)`` as the library reads them, the shapes checked."""
    _lib.require_gpu(instance_feature, anchor_embed, ww, bw, wl, bl)
    E = instance_feature.shape[-1]
    Nw, K3 = ww.shape[0], 0 if wl is None else wl.shape[0]
    if ww.shape != (Nw, E) or bw.shape != (Nw,) or (wl is not None and (wl.shape != (K3, E) or bl.shape != (K3,) or K3 % 3)):
        raise ValueError(f"{name}: instance_feature [..., {E}] against weights_fc {tuple(ww.shape)}, {tuple(bw.shape)}"
                         + ("" if wl is None else f" and learnable_fc {tuple(wl.shape)}, {tuple(bl.shape)}"))
    if anchor_embed is not None and anchor_embed.shape != instance_feature.shape:
        raise ValueError(f"{name}: anchor_embed {tuple(anchor_embed.shape)} is not {tuple(instance_feature.shape)}")
    f, e = _lib.aligned(instance_feature).reshape(-1, E), None if anchor_embed is None else _lib.aligned(anchor_embed).reshape(-1, E)
    return f, e, instance_feature.shape[:-1], E, K3, Nw


def _logits_launch(f, e, E, K3, Nw, table):
    """``(raw [n, Nw], learned [n, K3] | None)`` of ``gf_deform_logits_forward``."""
    n = f.shape[0]
    raw = torch.empty(n, Nw, dtype=f32, device=f.device)
    learned = torch.empty(n, K3, dtype=f32, device=f.device) if K3 else None
    _lib.call("gf_deform_logits_forward", f.device, n, E, K3, Nw, f, e, table, learned, raw)
    return raw, learned


def _logits_views(raw, learned, lead):
    return raw.view(*lead, raw.shape[-1]), None if learned is None else learned.view(*lead, learned.shape[-1] // 3, 3)


def deformable_logits(instance_feature, anchor_embed, weights_fc, learnable_fc=None):
    """``(raw [..., Nw], learned [..., K, 3] | None)`` in one launch, on any leading shape: ``raw = weights_fc(instance_feature +
    anchor_embed)`` (deformable_module.py:250-262; ``anchor_embed`` may be ``None``) and ``learned = learnable_fc(
    instance_feature)`` (:59-63) as ``key_points`` takes it.  ``weights_fc`` / ``learnable_fc``: an ``nn.Linear`` or a ``(weight,
    bias)`` pair, read in place at every call.  Forward only: inputs that need autograd are refused
    (``deformable_logits_autograd`` takes them)."""
    ww, bw, wl, bl = _logits_args(weights_fc, learnable_fc)
    _refuse_autograd("deformable_logits", [instance_feature, anchor_embed, ww, bw, wl, bl])
    return _logits_inference("deformable_logits", instance_feature, anchor_embed, ww, bw, wl, bl)


def _logits_inference(name, instance_feature, anchor_embed, ww, bw, wl, bl):
    """The inference launch; the callers have settled autograd."""
    f, e, lead, E, K3, Nw = _logits_shapes(name, instance_feature, anchor_embed, ww, bw, wl, bl)
    table, held = _lib.param_table([wl, bl, ww, bw], _lib.GF_DEFORM_LOGITS_PARAMS)
    return _logits_views(*_logits_launch(f, e, E, K3, Nw, table), lead)


def logits_train_sizes(n, K3, Nw, E=E_NATIVE):
    """``(saved_bytes, workspace_bytes)`` of the front's training step on ``n`` rows (``gf_deform_logits_train_sizes``);
    ``saved_bytes`` is 0: the op is linear."""
    return _lib.train_sizes("gf_deform_logits_train_sizes", n, E, K3, Nw)


class DeformLogitsFunction(torch.autograd.Function):
    """``raw, learned = DeformLogitsFunction.apply(instance_feature, anchor_embed, ww, bw, wl, bl)`` (``None`` for an absent
    tensor; ``learned`` is ``None`` without ``wl``): the forward is ``gf_deform_logits_forward`` -- the op is linear, nothing is
    saved but the inputs themselves -- and ``gf_deform_logits_backward`` returns the gradients of ``instance_feature``,
    ``anchor_embed`` and the four parameters -- of those that require one; the others get ``None`` and the library a NULL slot.
    Once-differentiable."""

    @staticmethod
    def forward(ctx, instance_feature, anchor_embed, ww, bw, wl, bl):
        f, e, lead, E, K3, Nw = _logits_shapes("deformable_logits_autograd", instance_feature, anchor_embed, ww, bw, wl, bl)
        slots, table, held = _lib.ParamSlots.pack([wl, bl, ww, bw], _lib.GF_DEFORM_LOGITS_PARAMS)
        raw, learned = _logits_launch(f, e, E, K3, Nw, table)
        ctx.save_for_backward(f, e, *held)
        ctx.shape = (lead, E, K3, Nw, instance_feature.dtype, None if anchor_embed is None else anchor_embed.dtype, slots)
        ctx.set_materialize_grads(False)     # an output nobody used: a NULL cotangent, not a tensor of zeros
        return _logits_views(raw, learned, lead)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_raw, grad_learned):
        f, e, *held = ctx.saved_tensors
        lead, E, K3, Nw, f_dtype, e_dtype, slots = ctx.shape
        n, need = f.shape[0], ctx.needs_input_grad
        wanted = need[4:6] + need[2:4]      # the table's order (wl, bl, ww, bw) from apply()'s (..., ww, bw, wl, bl)
        params, table = slots.unpack(held)
        grads, gtable = slots.grad_buffers(params, wanted)     # only those that require one: the others a NULL slot
        _, work_bytes = logits_train_sizes(n, K3, Nw, E)
        work = torch.empty(work_bytes, dtype=torch.uint8, device=f.device) if any(g is not None for g in grads) else None
        new = lambda: torch.empty(n, E, dtype=f32, device=f.device)
        grad_f = new() if need[0] else None
        grad_e = new() if e is not None and need[1] else None
        gr = None if grad_raw is None else _lib.aligned(grad_raw).reshape(n, Nw)
        gl = None if grad_learned is None or K3 == 0 else _lib.as_arg(grad_learned).reshape(n, K3)
        _lib.call("gf_deform_logits_backward", f.device, n, E, K3, Nw, f, e, table, gl, gr, grad_f, grad_e, gtable,
                  work, work_bytes if work is not None else 0)
        wl_g, bl_g, ww_g, bw_g = slots.returned(grads, wanted)
        return (None if grad_f is None else grad_f.view(*lead, E).to(f_dtype),
                None if grad_e is None else grad_e.view(*lead, E).to(e_dtype), ww_g, bw_g, wl_g, bl_g)


def deformable_logits_autograd(instance_feature, anchor_embed, weights_fc, learnable_fc=None):
    """``deformable_logits`` with a native backward: the same arguments and checks, the same bits, and ``raw``
    and ``learned`` carry the graph of ``DeformLogitsFunction``, so ``instance_feature``, ``anchor_embed`` and each of the four
    parameters that requires grad receives its gradient (the others ``None``).  With nothing that needs autograd (or under
    ``torch.no_grad()``) it is ``deformable_logits``."""
    ww, bw, wl, bl = _logits_args(weights_fc, learnable_fc)
    if not _lib.needs_grad([instance_feature, anchor_embed, ww, bw, wl, bl]):
        return _logits_inference("deformable_logits_autograd", instance_feature, anchor_embed, ww, bw, wl, bl)
    return DeformLogitsFunction.apply(instance_feature, anchor_embed, ww, bw, wl, bl)


def _output_args(name, features, output_proj, instance_feature, residual_mode, residual, norm):
    """``(wo, bo, g, b, inst)`` of an output call, its mode and pairs checked; ``inst`` is ``None`` with ``"none"``."""
    if residual_mode not in MODES:
        raise ValueError(f"{name}: residual_mode {residual_mode!r} is not one of {sorted(MODES)}")
    wo, bo = _pair(output_proj, "output_proj")
    g, b = _lib.norm_pair(norm, name)
    inst = instance_feature if residual_mode != "none" else None
    if residual_mode != "none" and inst is None:
        raise ValueError(f"{name}: residual_mode {residual_mode!r} needs instance_feature")
    return wo, bo, g, b, inst


def _output_shapes(name, features, inst, residual, wo, bo, g, b):
    """``(x [n, E], inst [n, E] | None, residual [n, E] | None, leading shape, E)`` as the library reads them, the shapes checked."""
    _lib.require_gpu(features, inst, residual, wo, bo, g, b)
    E = features.shape[-1]
    if wo.shape != (E, E) or bo.shape != (E,) or (g is not None and (g.shape != (E,) or b.shape != (E,))):
        raise ValueError(f"{name}: features [..., {E}] against output_proj {tuple(wo.shape)}, {tuple(bo.shape)}")
    for what, t in (("instance_feature", inst), ("residual", residual)):
        if t is not None and t.shape != features.shape:
            raise ValueError(f"{name}: {what} {tuple(t.shape)} is not {tuple(features.shape)}")
    x = _lib.aligned(features).reshape(-1, E)
    fi, res = (None if t is None else _lib.aligned(t).reshape(-1, E) for t in (inst, residual))
    return x, fi, res, features.shape[:-1], E


def deformable_output(features, output_proj, instance_feature=None, residual_mode="add", residual=None, norm=None):
    """``out`` of the block in one launch, on any leading shape: ``y = output_proj(features)``, then ``y`` (``residual_mode``
    ``"none"``), ``y + instance_feature`` (``"add"``) or ``cat([y, instance_feature])`` (``"cat"``; deformable_module.py:243-248),
    then -- not with ``"cat"`` -- ``+ residual [..., 128]`` and the ``nn.LayerNorm(128)`` ``norm`` where given: the encoder's
    ``"add", "norm"`` behind the block.  ``output_proj`` / ``norm``: a module or a ``(weight, bias)`` pair.  ``proj_drop`` is
    not applied (eval semantics).  Forward only: inputs that need autograd are refused."""
    wo, bo, g, b, inst = _output_args("deformable_output", features, output_proj, instance_feature, residual_mode, residual, norm)
    _refuse_autograd("deformable_output", [features, inst, residual, wo, bo, g, b])
    return _output_launch("deformable_output", features, inst, residual_mode, residual, wo, bo, g, b)


def _output_launch(name, features, inst, residual_mode, residual, wo, bo, g, b):
    """The inference launch; the callers have settled autograd."""
    x, fi, res, lead, E = _output_shapes(name, features, inst, residual, wo, bo, g, b)
    table, held = _lib.param_table([wo, bo, g, b], _lib.GF_DEFORM_OUTPUT_PARAMS)
    width = 2 * E if residual_mode == "cat" else E
    out = torch.empty(x.shape[0], width, dtype=f32, device=x.device)
    _lib.call("gf_deform_output_forward", x.device, x.shape[0], E, MODES[residual_mode], x, fi, table, res, out)
    return out.view(*lead, width)


def output_train_sizes(n, residual_mode="add", with_norm=False, E=E_NATIVE):
    """``(saved_bytes, workspace_bytes)`` of the output's training step on ``n`` rows (``gf_deform_output_train_sizes``)."""
    return _lib.train_sizes("gf_deform_output_train_sizes", n, E, MODES[residual_mode], int(bool(with_norm)))


class DeformOutputFunction(torch.autograd.Function):
    """``out = DeformOutputFunction.apply(residual_mode, features, instance_feature, residual, wo, bo, g, b)`` (``None`` for an
    absent tensor): ``gf_deform_output_forward_train`` keeps the row before the post norm and its statistics (nothing without a
    norm), ``gf_deform_output_backward`` returns the gradients of ``features``, ``instance_feature``, the residual and the four
    parameters -- of those that require one; the others get ``None`` and the library a NULL slot.  Once-differentiable."""

    @staticmethod
    def forward(ctx, residual_mode, features, instance_feature, residual, wo, bo, g, b):
        x, fi, res, lead, E = _output_shapes("deformable_output_autograd", features, instance_feature, residual, wo, bo, g, b)
        slots, table, held = _lib.ParamSlots.pack([wo, bo, g, b], _lib.GF_DEFORM_OUTPUT_PARAMS)
        n, mode = x.shape[0], MODES[residual_mode]
        saved_bytes, _ = output_train_sizes(n, residual_mode, g is not None, E)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=x.device) if saved_bytes else None
        width = 2 * E if residual_mode == "cat" else E
        out = torch.empty(n, width, dtype=f32, device=x.device)
        _lib.call("gf_deform_output_forward_train", x.device, n, E, mode, x, fi, table, res, out, saved, saved_bytes)
        ctx.save_for_backward(x, saved, *held)
        ctx.shape = (lead, E, residual_mode, features.dtype, None if instance_feature is None else instance_feature.dtype,
                     None if residual is None else residual.dtype, slots)
        return out.view(*lead, width)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, saved, *held = ctx.saved_tensors
        lead, E, residual_mode, x_dtype, inst_dtype, res_dtype, slots = ctx.shape
        n, mode, need = x.shape[0], MODES[residual_mode], ctx.needs_input_grad
        params, table = slots.unpack(held)
        grads, gtable = slots.grad_buffers(params, need[4:])     # only those that require one: the others a NULL slot
        _, work_bytes = output_train_sizes(n, residual_mode, params[2] is not None, E)
        work = torch.empty(work_bytes, dtype=torch.uint8, device=x.device)
        new = lambda: torch.empty(n, E, dtype=f32, device=x.device)
        grad_x = new()     # (the library writes it in full whoever asks)
        grad_inst = new() if inst_dtype is not None and need[2] else None
        grad_res = new() if res_dtype is not None and need[3] else None
        width = 2 * E if residual_mode == "cat" else E
        go = _lib.aligned(grad_out).reshape(n, width)
        _lib.call("gf_deform_output_backward", x.device, n, E, mode, x, table, saved, go, grad_x, grad_inst, grad_res, gtable,
                  work, work_bytes)
        return (None, grad_x.view(*lead, E).to(x_dtype) if need[1] else None,
                None if grad_inst is None else grad_inst.view(*lead, E).to(inst_dtype),
                None if grad_res is None else grad_res.view(*lead, E).to(res_dtype),
                *slots.returned(grads, need[4:]))


def deformable_output_autograd(features, output_proj, instance_feature=None, residual_mode="add", residual=None, norm=None):
    """``deformable_output`` with a native backward: the same arguments and checks, and ``out`` carries the graph of
    ``DeformOutputFunction``, so ``features``, ``instance_feature``, the residual and each of the four parameters that requires
    grad receives its gradient (the others ``None``).  ``proj_drop`` is not part of the op.  With nothing that needs autograd
    (or under ``torch.no_grad()``) it is ``deformable_output``."""
    name = "deformable_output_autograd"
    wo, bo, g, b, inst = _output_args(name, features, output_proj, instance_feature, residual_mode, residual, norm)
    if not _lib.needs_grad([features, inst, residual, wo, bo, g, b]):
        return _output_launch(name, features, inst, residual_mode, residual, wo, bo, g, b)
    return DeformOutputFunction.apply(residual_mode, features, inst, residual, wo, bo, g, b)


class DeformableFeatureAggregation(nn.Module):
    """Same constructor keys and defaults, attributes, submodule names, ``state_dict`` keys and ``forward(instance_feature, anchor,
    anchor_embed, feature_maps, metas, **kwargs)`` as the reference class (deformable_module.py:93-262), so its checkpoints load
    with ``strict=True``; built without mmengine (``kps_generator`` is the dict of this package's
    ``SparseGaussian3DKeyPointsGenerator``, its ``type`` ignored).  ``feature_maps``: the list of pyramid levels, formatted per
    call as the reference does, or an already formatted ``(table, spatial_shape, scale_start_index)`` triple, used as it is.

    The native route -- ``deformable_logits``, ``key_points``, ``deformable_fused_forward``, ``deformable_output``: four launches
    and, with ``use_camera_embed``, the camera encoder and its ``cams`` rows of ``weights_fc`` in torch (``weights_fc`` is linear:
    the ``[A cams, 128]`` broadcast sum of :253-262 is never formed) -- runs on fp32 GPU tensors with ``embed_dims == 128``, at
    most 32 learned columns, a ``residual_mode`` of ``"add"``, ``"cat"`` or ``"none"``, nothing that needs autograd, and in eval
    mode or with ``proj_drop.p == 0``.  Everything else runs ``forward_torch``: the module's torch layers around
    ``deformable_fused``, with the attention-dropout keep mask drawn as the reference draws it.

    ``native_dense`` is a class attribute, not a constructor key and not part of the ``state_dict``: ``False`` forces
    ``forward_torch``.  The keyword arguments ``residual=`` and ``norm=`` of ``forward`` fold the encoder's following ``"add",
    "norm"`` into the output launch (``out = norm(out + residual)``; not with ``"cat"``); without them the call is the
    reference's.

    ``native_training`` is likewise a class attribute, off by default and not part of the ``state_dict``: with it a call that
    needs autograd runs ``forward_torch`` as it is up to ``features`` and then ``deformable_output_autograd`` -- ``output_proj``,
    the add or the cat, ``residual=`` and ``norm=`` in one saving launch with a native backward -- under
    the conditions of the native route that concern the back end: ``embed_dims == 128``, fp32 GPU tensors, a known
    ``residual_mode``, eval mode or ``proj_drop.p == 0``, an affine ``LayerNorm`` with ``eps = 1e-5``.  The front end
    (``weights_fc``, ``learnable_fc``) stays on torch there.

    ``native_front_training`` is a switch of its own for that front end, again a class attribute, off by default and not part
    of the ``state_dict``: with it a call that needs autograd, with ``embed_dims == 128``, fp32 GPU tensors and at most 32
    learned columns -- in train or eval mode, with any ``attn_drop``: the mask is drawn behind the front as before -- takes
    ``raw`` and ``learned`` from ``deformable_logits_autograd`` (one launch forward, a native backward) and the
    key points from the functional ``key_points``; ``weights_fc`` and ``learnable_fc`` do not run as modules.  The camera encoder
    and its rows of ``weights_fc`` stay on torch (``weights_fc.weight`` then has two producers; autograd adds them).  The two
    switches are independent; together they leave only the camera encoder on torch."""

    native_dense = True
    native_training = False
    native_front_training = False

    def __init__(self, embed_dims=256, num_groups=8, num_levels=4, num_cams=6, proj_drop=0.0, attn_drop=0.0, kps_generator=None,
                 use_deformable_func=False, use_camera_embed=False, residual_mode="add"):
        super().__init__()
        if embed_dims % num_groups != 0:
            raise ValueError(f"embed_dims must be divisible by num_groups, but got {embed_dims} and {num_groups}")
        self.group_dims = int(embed_dims / num_groups)
        self.embed_dims = embed_dims
        self.num_levels = num_levels
        self.num_groups = num_groups
        self.num_cams = num_cams
        self.use_deformable_func = use_deformable_func
        assert self.use_deformable_func       # (the reference's :119-120: only the op's route exists)
        self.attn_drop = attn_drop
        self.residual_mode = residual_mode
        self.proj_drop = nn.Dropout(proj_drop)
        kps_generator["embed_dims"] = embed_dims
        self.kps_generator = SparseGaussian3DKeyPointsGenerator(**{k: v for k, v in kps_generator.items() if k != "type"})
        self.num_pts = self.kps_generator.num_pts
        self.output_proj = nn.Linear(embed_dims, embed_dims)
        if use_camera_embed:
            # (the reference's linear_relu_ln(embed_dims, 1, 2, 12): keys camera_encoder.0 / .2 / .3 / .5)
            self.camera_encoder = nn.Sequential(nn.Linear(12, embed_dims), nn.ReLU(inplace=True), nn.LayerNorm(embed_dims),
                                                nn.Linear(embed_dims, embed_dims), nn.ReLU(inplace=True), nn.LayerNorm(embed_dims))
            self.weights_fc = nn.Linear(embed_dims, num_groups * num_levels * self.num_pts)
        else:
            self.camera_encoder = None
            self.weights_fc = nn.Linear(embed_dims, num_groups * num_cams * num_levels * self.num_pts)

    def init_weight(self):
        nn.init.constant_(self.weights_fc.weight, 0.0)
        nn.init.constant_(self.weights_fc.bias, 0.0)
        nn.init.xavier_uniform_(self.output_proj.weight)
        nn.init.constant_(self.output_proj.bias, 0.0)

    def _output_native(self, instance_feature, anchor, anchor_embed, table, residual, norm):
        """The tensors of a call whose back end has a native form, else ``None``: the conditions the inference route and
        the training step share."""
        if self.embed_dims != E_NATIVE or self.residual_mode not in MODES:
            return None
        if self.training and self.proj_drop.p > 0:
            return None
        if self.residual_mode == "cat" and (residual is not None or norm is not None):
            return None
        if isinstance(norm, nn.LayerNorm) and not _lib.norm_native(norm):
            return None
        tensors = [instance_feature, anchor, anchor_embed, table, residual, *self.parameters(), *_lib.norm_tensors(norm)]
        return tensors if _lib.native_tensors(tensors) else None

    def _native(self, instance_feature, anchor, anchor_embed, table, residual, norm):
        if not self.native_dense or 3 * self.kps_generator.num_learnable_pts > MAX_LEARNED:
            return False
        tensors = self._output_native(instance_feature, anchor, anchor_embed, table, residual, norm)
        return tensors is not None and not _lib.needs_grad(tensors)

    def _native_training(self, instance_feature, anchor, anchor_embed, table, residual, norm):
        """Whether this call's back end runs its native training step (``native_training``)."""
        if not self.native_training or (isinstance(norm, nn.Module) and not isinstance(norm, nn.LayerNorm)):
            return False
        tensors = self._output_native(instance_feature, anchor, anchor_embed, table, residual, norm)
        return tensors is not None and _lib.needs_grad(tensors)

    def _native_front_training(self, instance_feature, anchor, anchor_embed, table):
        """Whether this call's front end runs its native training step (``native_front_training``)."""
        if not self.native_front_training or self.embed_dims != E_NATIVE or 3 * self.kps_generator.num_learnable_pts > MAX_LEARNED:
            return False
        tensors = [instance_feature, anchor, anchor_embed, table, *self.parameters()]
        return _lib.native_tensors(tensors) and _lib.needs_grad(tensors)

    def forward(self, instance_feature, anchor, anchor_embed, feature_maps, metas, **kwargs):
        residual, norm = kwargs.get("residual"), kwargs.get("norm")
        if not (isinstance(feature_maps, (tuple, list)) and len(feature_maps) == 3 and feature_maps[1].dim() == 2):
            feature_maps = DAF.feature_maps_format(feature_maps)
        if not self._native(instance_feature, anchor, anchor_embed, feature_maps[0], residual, norm):
            native_output = self._native_training(instance_feature, anchor, anchor_embed, feature_maps[0], residual, norm)
            native_front = self._native_front_training(instance_feature, anchor, anchor_embed, feature_maps[0])
            return self.forward_torch(instance_feature, anchor, anchor_embed, feature_maps, metas, residual=residual, norm=norm,
                                      native_output=native_output, native_front=native_front)
        bs, A = instance_feature.shape[:2]
        gen = self.kps_generator
        raw, learned = deformable_logits(instance_feature, anchor_embed, self.weights_fc,
                                         gen.learnable_fc if gen.num_learnable_pts > 0 else None)
        kp = key_points(anchor, learned, gen._fix, gen.pc_range, gen.scale_range, gen.learnable_fixed_scale, gen.xyz_act, gen.scale_act)
        pm, wh = metas["projection_mat"], metas.get("image_wh")
        L, G = self.num_levels, self.num_groups
        if self.camera_encoder is not None:
            raw_cam = F.linear(self.camera_encoder(pm[:, :, :3].reshape(bs, self.num_cams, -1)), self.weights_fc.weight)
            features = deformable_fused_forward(kp, pm, wh, *feature_maps, raw_anchor=raw.view(bs, A, L, self.num_pts, G),
                                                raw_cam=raw_cam.view(bs, self.num_cams, L, self.num_pts, G))
        else:
            features = deformable_fused_forward(kp, pm, wh, *feature_maps, raw_weights=raw.view(bs, A, self.num_cams, L, self.num_pts, G))
        return deformable_output(features, self.output_proj, instance_feature, self.residual_mode, residual, norm)

    def forward_torch(self, instance_feature, anchor, anchor_embed, feature_maps, metas, residual=None, norm=None, native_output=False,
                      native_front=False):
        """The reference's composition (:146-262) on the module's torch layers around ``deformable_fused``; ``feature_maps`` is
        the formatted triple.  ``native_output``: everything behind ``features`` is ``deformable_output_autograd`` (the caller
        has asked ``_native_training``).  ``native_front``: ``weights_fc`` on the sum and ``learnable_fc`` are
        ``deformable_logits_autograd`` and the key points the functional ``key_points`` (the caller has asked
        ``_native_front_training``)."""
        bs, A = instance_feature.shape[:2]
        pm, wh = metas["projection_mat"], metas.get("image_wh")
        L, G, cams = self.num_levels, self.num_groups, self.num_cams
        if native_front:
            gen = self.kps_generator
            per_anchor, learned = deformable_logits_autograd(instance_feature, anchor_embed, self.weights_fc,
                                                             gen.learnable_fc if gen.num_learnable_pts > 0 else None)
            kp = key_points(anchor, learned, gen._fix, gen.pc_range, gen.scale_range, gen.learnable_fixed_scale, gen.xyz_act, gen.scale_act)
        else:
            kp = self.kps_generator(anchor, instance_feature)
            per_anchor = self.weights_fc(instance_feature + anchor_embed)
        if self.camera_encoder is not None:
            raw_cam = F.linear(self.camera_encoder(pm[:, :, :3].reshape(bs, cams, -1)), self.weights_fc.weight)
            logits = dict(raw_anchor=per_anchor.reshape(bs, A, L, self.num_pts, G), raw_cam=raw_cam.reshape(bs, cams, L, self.num_pts, G))
        else:
            logits = dict(raw_weights=per_anchor.reshape(bs, A, cams, L, self.num_pts, G))
        weight_mask = None
        if self.training and self.attn_drop > 0:     # (:273-282)
            weight_mask = torch.rand(bs, A, cams, L, self.num_pts, G, dtype=per_anchor.dtype, device=per_anchor.device) > self.attn_drop
        if weight_mask is None and not _lib.needs_grad([kp, feature_maps[0], per_anchor]):
            features = deformable_fused_forward(kp, pm, wh, *feature_maps, **logits)     # the same block, the inference launch
        else:
            features = deformable_fused(kp, pm, wh, *feature_maps, weight_mask=weight_mask, **logits)
        if native_output:
            return deformable_output_autograd(features, self.output_proj, instance_feature, self.residual_mode, residual, norm)
        output = self.proj_drop(self.output_proj(features))
        if self.residual_mode == "add":
            output = output + instance_feature
        elif self.residual_mode == "cat":
            output = torch.cat([output, instance_feature], dim=-1)
        if residual is not None:
            output = output + residual
        if norm is not None:
            output = _lib.apply_norm(output, norm)
        return output
