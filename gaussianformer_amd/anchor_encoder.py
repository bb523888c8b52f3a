"""The anchor encoder: drop-in for ``SparseGaussian3DEncoder`` (model/encoder/gaussian_encoder/anchor_encoder_module.py:7-53,
its layers from ``linear_relu_ln``, utils.py:49-59).  Five input branches (xyz, scale, rotation, opacity, semantics), each
``Linear(k -> E), ReLU, LayerNorm, Linear(E -> E), ReLU, LayerNorm``, their sum, then ``output_fc`` with two more such stages:
about 40 torch kernels, and ``gf_anchor_embed_forward`` (include/gf_hip.h) in one launch.  Training keeps
the module's torch layers unless asked otherwise: ``anchor_embed_autograd`` and a module with ``native_training = True`` run the native training
step (``gf_anchor_embed_forward_train`` / ``gf_anchor_embed_backward``)."""
import torch
import torch.nn as nn

from . import _lib

f32 = torch.float32
E_NATIVE, MAX_S = _lib.GF_ANCHOR_EMBED_DIMS, _lib.GF_ANCHOR_EMBED_MAX_S
STAGES = ("xyz_fc", "scale_fc", "rot_fc", "opacity_fc", "semantics_fc", "output_fc")
_SLOTS = ("0.weight", "0.bias", "2.weight", "2.bias", "3.weight", "3.bias", "5.weight", "5.bias")   # state_dict order


def embedding_layer(embed_dims, input_dims):
    """``nn.Sequential(*linear_relu_ln(embed_dims, 1, 2, input_dims))``: Linear at 0 and 3, LayerNorm at 2 and 5."""
    E = embed_dims
    return nn.Sequential(nn.Linear(input_dims, E), nn.ReLU(inplace=True), nn.LayerNorm(E),
                         nn.Linear(E, E), nn.ReLU(inplace=True), nn.LayerNorm(E))


def _param_list(module_or_params):
    """The 48 parameters in the library's order (``None`` for an absent branch), from a module with the reference's submodule
    names or from a mapping with its state_dict keys."""
    if isinstance(module_or_params, nn.Module):
        def get(stage, slot):
            sub = getattr(module_or_params, stage, None)
            if sub is None:
                return None
            i, name = slot.split(".")
            return getattr(sub[int(i)], name)
    else:
        def get(stage, slot):
            return module_or_params.get(f"{stage}.{slot}")
    return [get(stage, slot) for stage in STAGES for slot in _SLOTS]


def _shape(anchor, params):
    """``(a [n, Da] as the library reads it, leading shape, E, opa, S)`` of a call on the 48-entry parameter list."""
    _lib.require_gpu(anchor, *params)
    if params[0] is None or params[40] is None:
        raise ValueError("anchor_embed needs at least xyz_fc, scale_fc, rot_fc and output_fc")
    a = _lib.as_arg(anchor)
    return a.reshape(-1, a.shape[-1]), a.shape[:-1], params[0].shape[0], 1 if params[24] is not None else 0, 0 if params[32] is None else params[32].shape[1]


def _launch(anchor, params):
    """The library call on the 48-entry parameter list; the callers have settled autograd."""
    a, lead, E, opa, S = _shape(anchor, params)
    table, held = _lib.param_table(params, _lib.GF_ANCHOR_EMBED_PARAMS)
    out = torch.empty(a.shape[0], E, dtype=f32, device=a.device)
    _lib.call("gf_anchor_embed_forward", a.device, a.shape[0], a.shape[1], E, opa, S, a, table, out)
    return out.view(*lead, E)


def train_sizes(n, include_opa, S):
    """``(saved_bytes, workspace_bytes)`` of the training step on ``n`` rows (``gf_anchor_embed_train_sizes``)."""
    return _lib.train_sizes("gf_anchor_embed_train_sizes", n, int(bool(include_opa)), S)


class AnchorEmbedFunction(torch.autograd.Function):
    """``out = AnchorEmbedFunction.apply(anchor, *params)`` on the 48-entry parameter list (``None`` for an absent branch):
    ``gf_anchor_embed_forward_train`` keeps every stage's post-ReLU row and LayerNorm statistics, ``gf_anchor_embed_backward``
    returns the gradients of the anchor and of every parameter that requires one.  Once-differentiable."""

    @staticmethod
    def forward(ctx, anchor, *params):
        a, lead, E, opa, S = _shape(anchor, params)
        slots, table, held = _lib.ParamSlots.pack(params, _lib.GF_ANCHOR_EMBED_PARAMS)
        n, Da = a.shape
        saved_bytes, _ = train_sizes(n, opa, S)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=a.device)
        out = torch.empty(n, E, dtype=f32, device=a.device)
        _lib.call("gf_anchor_embed_forward_train", a.device, n, Da, E, opa, S, a, table, out, saved, saved_bytes)
        ctx.save_for_backward(a, saved, *held)
        ctx.shape = (lead, E, opa, S, anchor.dtype, slots)
        return out.view(*lead, E)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        a, saved, *held = ctx.saved_tensors
        lead, E, opa, S, anchor_dtype, slots = ctx.shape
        n, Da = a.shape
        params, table = slots.unpack(held)
        grads, gtable = slots.grad_buffers(params, [True] * len(params))     # every present parameter
        _, work_bytes = train_sizes(n, opa, S)
        work = torch.empty(work_bytes, dtype=torch.uint8, device=a.device)
        grad_anchor = torch.empty(n, Da, dtype=f32, device=a.device)
        go = _lib.as_arg(grad_out).reshape(n, E)
        _lib.call("gf_anchor_embed_backward", a.device, n, Da, E, opa, S, a, table, saved, go, grad_anchor, gtable, work, work_bytes)
        need = ctx.needs_input_grad
        return (grad_anchor.view(*lead, Da).to(anchor_dtype) if need[0] else None, *slots.returned(grads, need[1:]))


def anchor_embed_autograd(anchor, module_or_params):
    """``anchor_embed`` with a native backward: ``out [..., 128]`` carries the graph of ``AnchorEmbedFunction``, so the anchor and
    every parameter that requires grad receive their gradients (the others ``None``).  Under ``torch.no_grad()``, or when
    nothing requires grad, it is the plain forward."""
    params = _param_list(module_or_params)
    if not _lib.needs_grad([anchor, *params]):
        return _launch(anchor, params)
    return AnchorEmbedFunction.apply(anchor, *params)


def anchor_embed(anchor, module_or_params):
    """``out [..., 128] = SparseGaussian3DEncoder.forward(anchor [..., Da])`` by the native op, on any leading batch shape.
    ``module_or_params``: a module with the reference's submodules, or a mapping with its state_dict keys
    (``xyz_fc.0.weight`` ... ``output_fc.5.bias``); which branches exist says ``include_opa`` and the semantic width.  The
    parameters are read in place at every call.  Forward only: inputs that need autograd are refused."""
    params = _param_list(module_or_params)
    _lib.refuse_autograd("anchor_embed", [anchor, *params], "(the SparseGaussian3DEncoder module routes training to its torch "
                         "layers), or call anchor_embed_autograd, which has one")
    return _launch(anchor, params)


class SparseGaussian3DEncoder(nn.Module):
    """Same constructor keys and defaults, attributes, submodule names, ``state_dict`` keys and ``forward(box_3d)`` as the
    reference class (anchor_encoder_module.py:7-53), so its checkpoints load with ``strict=True``.  The native op runs when the
    input is an fp32 GPU tensor, ``embed_dims == 128``, the semantic width is at most 32 and nothing needs autograd; everything
    else (training, CPU tensors, other widths or dtypes) runs the module's own torch layers, the reference's composition.
    ``native_training`` is an attribute, not a constructor key (the constructor stays the reference's), off by default and not
    part of the ``state_dict``: set ``module.native_training = True`` and, under the same conditions, a call that needs autograd
    runs ``AnchorEmbedFunction`` instead of the torch layers."""

    native_training = False

    def __init__(self, embed_dims=256, include_opa=True, semantics=False, semantic_dim=None):
        super().__init__()
        self.embed_dims = embed_dims
        self.include_opa = include_opa
        self.semantics = semantics
        self.xyz_fc = embedding_layer(embed_dims, 3)
        self.scale_fc = embedding_layer(embed_dims, 3)
        self.rot_fc = embedding_layer(embed_dims, 4)
        if include_opa:
            self.opacity_fc = embedding_layer(embed_dims, 1)
        if semantics:
            assert semantic_dim is not None
            self.semantics_fc = embedding_layer(embed_dims, semantic_dim)
            self.semantic_start = 10 + int(include_opa)
        else:
            semantic_dim = 0
        self.semantic_dim = semantic_dim
        self.output_fc = embedding_layer(embed_dims, embed_dims)

    def forward(self, box_3d):
        if box_3d.is_cuda and box_3d.dtype == f32 and self.embed_dims == E_NATIVE and self.semantic_dim <= MAX_S:
            params = _param_list(self)
            if params[0].is_cuda and params[0].dtype == f32:
                if not _lib.needs_grad([box_3d, *params]):
                    return _launch(box_3d, params)
                if self.native_training:
                    return AnchorEmbedFunction.apply(box_3d, *params)
        return self.forward_torch(box_3d)

    def forward_torch(self, box_3d):
        """The reference's composition (:38-53) on the module's torch layers."""
        output = self.xyz_fc(box_3d[..., :3]) + self.scale_fc(box_3d[..., 3:6]) + self.rot_fc(box_3d[..., 6:10])
        if self.include_opa:
            output = output + self.opacity_fc(box_3d[..., 10:11])
        if self.semantics:
            output = output + self.semantics_fc(box_3d[..., self.semantic_start:self.semantic_start + self.semantic_dim])
        return self.output_fc(output)
