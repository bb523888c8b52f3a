"""The encoder's Gaussian refinement step: host mirror of ``SparseGaussian3DRefinementModule``
(model/encoder/gaussian_encoder/refine_module.py:11-123) and ``SparseGaussian3DRefinementModuleV2``
(refine_module_v2.py:12-108).  By default the MLP (``layers``) stays torch; everything after it -- the 30-40 slices, stacks,
cats, clamps, sigmoids and logs of :72-123 / v2 :62-107 -- is ``gf_refine_forward`` / ``gf_refine_backward``
(include/gf_hip.h): one launch each way.  ``refine_fused`` (and the modules with ``fused_mlp = True``, inference only) runs the
MLP and the tail in one launch, ``gf_refine_mlp_forward``.  ``refine_fused_autograd`` (and the modules with
``native_training = True``) is the native training step: ``gf_refine_mlp_forward_train`` / ``gf_refine_mlp_backward``."""
import ctypes
from collections import namedtuple
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import Function, once_differentiable

from . import _lib

f32 = torch.float32
_SEMANTICS = {"softmax": _lib.GF_REFINE_SEM_SOFTMAX, "softplus": _lib.GF_REFINE_SEM_SOFTPLUS}


# the reference's result type by its field names (model/encoder/gaussian_encoder/utils.py:62-69); the last two are version 2's
GaussianPrediction = namedtuple("GaussianPrediction", "means scales rotations opacities semantics original_means delta_means",
                                defaults=(None, None))


class RefineConfig(NamedTuple):
    """What the library call needs besides the tensors: ``consts`` = pc_range (6), scale_range (2), unit (3) as doubles."""
    version: int
    flags: int
    R: int
    S: int
    consts: tuple


def refine_config(version, pc_range, scale_range, unit=None, restrict_xyz=False, refine_manual=(), semantic_dim=0,
                  include_opa=True, semantics_activation="softmax", xyz_activation="sigmoid"):
    """``unit``: version 1 = the module's ``unit_sigmoid`` (needed with ``restrict_xyz`` only), version 2 = ``unit_xyz``."""
    refine_manual = list(refine_manual)
    if refine_manual != list(range(len(refine_manual))):
        raise ValueError(f"refine_manual must be the prefix 0 .. R-1 (refine_module.py:57), got {refine_manual}")
    flags = _SEMANTICS.get(semantics_activation, 0)
    flags |= _lib.GF_REFINE_RESTRICT_XYZ if (version == 1 and restrict_xyz) else 0
    flags |= 0 if xyz_activation == "sigmoid" else _lib.GF_REFINE_XYZ_IDENTITY
    flags |= _lib.GF_REFINE_OPACITY if include_opa else 0
    unit = (0.0, 0.0, 0.0) if unit is None else unit
    consts = tuple(float(v) for v in (*pc_range, *scale_range, *unit))
    assert len(consts) == 11
    return RefineConfig(version, flags, len(refine_manual) if version == 1 else 0, int(semantic_dim), consts)


class RefineFunction(Function):
    """``anchor_out [n, D], means [n, 3], scales [n, 3], rotations [n, 4], opacities [n, 0 | 1], semantics [n, S],
    original_means [n, 3], delta_means [n, 3] = apply(output [n, D], anchor [n, Da], cfg)``; the last two are empty in
    version 1.  ``output`` is the MLP's result after ``Scale``."""

    @staticmethod
    def forward(ctx, output, anchor, cfg):
        _lib.require_gpu(output, anchor)
        ctx.set_materialize_grads(False)   # an unused output's gradient reaches the library as NULL, not as a tensor of zeros
        o, a = _lib.as_arg(output), _lib.as_arg(anchor)
        n, D = o.shape
        Da = a.shape[1]
        opa = 1 if cfg.flags & _lib.GF_REFINE_OPACITY else 0

        def new(w):
            return torch.empty(n, w, dtype=f32, device=o.device)

        three = 3 if cfg.version == 2 else 0
        outs = (new(D), new(3), new(3), new(4), new(opa), new(cfg.S), new(three), new(three))
        consts = (ctypes.c_double * 11)(*cfg.consts)
        ctx.call = (n, D, Da, cfg.version, cfg.flags, cfg.R, cfg.S, consts)
        _lib.call("gf_refine_forward", o.device, n, D, Da, cfg.version, cfg.flags, cfg.R, cfg.S,
                  ctypes.cast(consts, ctypes.c_void_p), o, a, *outs)
        ctx.save_for_backward(o, a)
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        o, a = ctx.saved_tensors
        n, D, Da, version, flags, R, S, consts = ctx.call
        g = [None if t is None or t.numel() == 0 else _lib.as_arg(t) for t in grads]   # (an empty output's carries nothing)
        go, ga = torch.empty_like(o), torch.empty_like(a)
        _lib.call("gf_refine_backward", o.device, n, D, Da, version, flags, R, S, ctypes.cast(consts, ctypes.c_void_p), o, a, *g, go, ga)
        return go, ga, None


def refine(output, anchor, cfg):
    """Functional form on any leading batch shape: ``(anchor_out [..., D], GaussianPrediction)``."""
    lead = output.shape[:-1]
    outs = RefineFunction.apply(output.reshape(-1, output.shape[-1]), anchor.reshape(-1, anchor.shape[-1]), cfg)
    return _prediction([t.view(*lead, t.shape[-1]) for t in outs], cfg)


def _prediction(outs, cfg):
    """``(anchor_out, GaussianPrediction)`` of a launch's eight outputs; version 1 has no ``original_means`` / ``delta_means``."""
    return outs[0], GaussianPrediction(*outs[1:6 if cfg.version == 1 else 8])


MLP_KEYS = ("layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias", "layers.4.weight", "layers.4.bias",
            "layers.5.weight", "layers.5.bias", "layers.7.weight", "layers.7.bias", "layers.9.weight", "layers.9.bias",
            "layers.10.weight", "layers.10.bias", "layers.11.scale")
assert len(MLP_KEYS) == _lib.GF_REFINE_MLP_PARAMS


def _mlp_table(params):
    """The library's host table of the 15 parameter pointers, the tensors as ``_lib.as_arg`` left them.  (Not
    ``_lib.param_table``: that clones a misaligned parameter, and this op's contract is that the library refuses one.)"""
    return ctypes.cast((ctypes.c_void_p * _lib.GF_REFINE_MLP_PARAMS)(*[t.data_ptr() for t in params]), ctypes.c_void_p)


def refine_fused(instance_feature, anchor, anchor_embed, module_or_state_dict, cfg, return_mlp_output=False):
    """The modules' whole forward in one launch (``gf_refine_mlp_forward``), on any leading batch shape:
    ``(anchor_out [..., D], GaussianPrediction)``, plus the MLP's result after ``Scale`` ``[..., D]`` -- the bits the tail
    consumed -- with ``return_mlp_output``.  The parameters come from a refinement module or from a state_dict with its keys
    (``MLP_KEYS``), as they are at the time of the call.  Forward only: it computes no gradients and refuses to run where
    autograd would record one."""
    state = module_or_state_dict
    if isinstance(state, nn.Module):
        state = dict(state.named_parameters())
    params = [state[k] for k in MLP_KEYS]
    if _lib.needs_grad((instance_feature, anchor, anchor_embed, *params)):
        raise RuntimeError("refine_fused computes no gradients: use the module with fused_mlp = False (the torch MLP + refine) "
                           "for training, or call it under torch.no_grad()")
    f, e, a, params, lead, call, outs, consts = _fused_args(instance_feature, anchor, anchor_embed, cfg, params)
    D = call[2]
    mlp_out = torch.empty(f.shape[0], D, dtype=f32, device=f.device) if return_mlp_output else None
    _lib.call("gf_refine_mlp_forward", f.device, *call, ctypes.cast(consts, ctypes.c_void_p), f, e, a, _mlp_table(params), mlp_out, *outs)
    anchor_out, pred = _prediction([t.view(*lead, t.shape[-1]) for t in outs], cfg)
    if return_mlp_output:
        return anchor_out, pred, mlp_out.view(*lead, D)
    return anchor_out, pred


def _fused_args(instance_feature, anchor, anchor_embed, cfg, params):
    """What the one-launch forward and its saving form share: ``(f [n, E], e [n, E], a [n, Da], params, leading shape, call,
    outs, consts)`` -- the inputs and the 15 parameters as the library reads them, their shapes checked; ``call = (n, E, D, Da,
    version, flags, R, S)``, the launch's integers; the eight outputs ``[n, ...]`` (the last two empty in version 1); the
    constants as the array the launch points at."""
    _lib.require_gpu(instance_feature, anchor, anchor_embed, *params)
    lead, E = instance_feature.shape[:-1], instance_feature.shape[-1]
    f = _lib.as_arg(instance_feature).reshape(-1, E)
    e = _lib.as_arg(anchor_embed).expand(*lead, E).reshape(-1, E).contiguous()   # (a broadcast one: its rows written out)
    a = _lib.as_arg(anchor).reshape(-1, anchor.shape[-1])
    params = [_lib.as_arg(t) for t in params]
    n, Da, D = f.shape[0], a.shape[1], params[12].shape[0]
    if a.shape[0] != n:
        raise ValueError(f"instance_feature has {n} rows, anchor {a.shape[0]}")
    shapes = [(E, E), (E,), (E, E), (E,), (E,), (E,)] * 2 + [(D, E), (D,), (D,)]
    for k, t, want in zip(MLP_KEYS, params, shapes):
        if tuple(t.shape) != want:
            raise ValueError(f"{k} has shape {tuple(t.shape)}, expected {want}")
    opa = 1 if cfg.flags & _lib.GF_REFINE_OPACITY else 0

    def new(w):
        return torch.empty(n, w, dtype=f32, device=f.device)

    three = 3 if cfg.version == 2 else 0
    outs = (new(D), new(3), new(3), new(4), new(opa), new(cfg.S), new(three), new(three))
    return f, e, a, params, lead, (n, E, D, Da, cfg.version, cfg.flags, cfg.R, cfg.S), outs, (ctypes.c_double * 11)(*cfg.consts)


def train_sizes(n, D, Da):
    """``(saved_bytes, workspace_bytes)`` of the native training step on ``n`` rows (``gf_refine_mlp_train_sizes``)."""
    return _lib.train_sizes("gf_refine_mlp_train_sizes", n, D, Da)


_train_scratch = _lib.StreamScratch()   # the backward's workspace (one chunk's dz rows, the partial sums)


class RefineFusedFunction(Function):
    """``anchor_out, means, scales, rotations, opacities, semantics, original_means, delta_means =
    apply(instance_feature [..., 128], anchor [..., Da], anchor_embed (broadcastable to instance_feature), cfg, *params)`` on
    the 15 parameters in ``MLP_KEYS`` order: ``gf_refine_mlp_forward_train`` keeps the four post-ReLU rows, the LayerNorms'
    statistics and the MLP's result, ``gf_refine_mlp_backward`` returns the gradients of the three inputs and of every
    parameter that requires one.  The outputs carry the leading shape; the last two are empty in version 1.
    Once-differentiable."""

    @staticmethod
    def forward(ctx, instance_feature, anchor, anchor_embed, cfg, *params):
        ctx.set_materialize_grads(False)   # an unused output's gradient reaches the library as NULL, not as a tensor of zeros
        f, e, a, held, lead, call, outs, consts = _fused_args(instance_feature, anchor, anchor_embed, cfg, params)
        n, E, D, Da = call[:4]
        saved_bytes, _ = train_sizes(n, D, Da)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=f.device)
        ctx.call = (*call, consts)
        _lib.call("gf_refine_mlp_forward_train", f.device, *call, ctypes.cast(consts, ctypes.c_void_p),
                  f, e, a, _mlp_table(held), None, *outs, saved, saved_bytes)
        ctx.save_for_backward(f, e, a, saved, *held)
        # (no table from the record: a misaligned parameter is the library's to refuse, so the tables stay _mlp_table's)
        ctx.shape = (lead, tuple(anchor_embed.shape), instance_feature.dtype, anchor.dtype, anchor_embed.dtype,
                     _lib.ParamSlots(params, _lib.GF_REFINE_MLP_PARAMS))
        return tuple(t.view(*lead, t.shape[-1]) for t in outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        f, e, a, saved, *held = ctx.saved_tensors
        n, E, D, Da, version, flags, R, S, consts = ctx.call
        lead, embed_shape, f_dtype, a_dtype, e_dtype, slots = ctx.shape
        g = [None if t is None or t.numel() == 0 else _lib.as_arg(t).reshape(n, t.shape[-1]) for t in grads]
        grad_x = torch.empty(n, E, dtype=f32, device=f.device)
        grad_anchor = torch.empty(n, Da, dtype=f32, device=f.device)
        grad_params = [torch.empty_like(t) for t in held]
        _, work_bytes = train_sizes(n, D, Da)
        work = _train_scratch.get(f.device, work_bytes)
        _lib.call("gf_refine_mlp_backward", f.device, n, E, D, Da, version, flags, R, S, ctypes.cast(consts, ctypes.c_void_p),
                  f, e, a, _mlp_table(held), saved, *g, grad_x, grad_anchor, None,
                  _lib.out_table(grad_params, _lib.GF_REFINE_MLP_PARAMS), work, work_bytes)
        need = ctx.needs_input_grad
        gx = grad_x.view(*lead, E)
        return (gx.to(f_dtype) if need[0] else None,
                grad_anchor.view(*lead, Da).to(a_dtype) if need[1] else None,
                gx.sum_to_size(embed_shape).to(e_dtype) if need[2] else None, None,
                *slots.returned(grad_params, need[4:]))


def refine_fused_autograd(instance_feature, anchor, anchor_embed, module_or_state_dict, cfg):
    """``refine_fused`` with a native backward (``RefineFusedFunction``), on any leading batch shape: ``(anchor_out [..., D],
    GaussianPrediction)`` carrying the graph, so the three inputs and every parameter that requires grad receive their
    gradients (the others ``None``); a broadcast ``anchor_embed`` gets its gradient summed to its shape.  With nothing that
    needs autograd (or under ``torch.no_grad()``) it is ``refine_fused``."""
    state = module_or_state_dict
    if isinstance(state, nn.Module):
        state = dict(state.named_parameters())
    params = [state[k] for k in MLP_KEYS]
    _lib.require_gpu(instance_feature, anchor, anchor_embed, *params)
    if not _lib.needs_grad((instance_feature, anchor, anchor_embed, *params)):
        return refine_fused(instance_feature, anchor, anchor_embed, state, cfg)
    return _prediction(RefineFusedFunction.apply(instance_feature, anchor, anchor_embed, cfg, *params), cfg)


class Scale(nn.Module):
    """One learnable factor per column, all ones at first: the parameter ``scale [width]`` that mmcv's ``Scale`` holds when the
    reference builds it from a list."""

    def __init__(self, width):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(width))

    def forward(self, x):
        return x * self.scale


def refinement_mlp(embed_dims, output_dim):
    """The modules' ``layers``, with the reference's state_dict keys: Linear at 0, 2, 5, 7 and 10, LayerNorm at 4 and 9, the
    ``Scale`` at 11 (ReLUs between)."""
    E = embed_dims
    return nn.Sequential(
        nn.Linear(E, E), nn.ReLU(inplace=True), nn.Linear(E, E), nn.ReLU(inplace=True), nn.LayerNorm(E),
        nn.Linear(E, E), nn.ReLU(inplace=True), nn.Linear(E, E), nn.ReLU(inplace=True), nn.LayerNorm(E),
        nn.Linear(E, output_dim), Scale(output_dim))


class _Refinement(nn.Module):
    """What the two drop-ins share: the torch MLP, then one library call.  ``fused_mlp`` (an attribute, not a constructor key and
    not in the state_dict; off by default): when set, a call that needs no gradient, at ``embed_dims`` 128 on fp32 GPU tensors,
    is one launch (``refine_fused``); every other call takes the default route.  ``native_training`` (an attribute of the same
    kind, off by default): when set, a call that needs autograd, under the same conditions, is ``refine_fused_autograd`` -- the
    saving forward and the native backward -- instead of the torch layers and ``refine``."""
    fused_mlp = False
    native_training = False

    def __init__(self, version, where, embed_dims, pc_range, scale_range, unit, restrict_xyz, refine_manual, semantics,
                 semantic_dim, include_opa, semantics_activation, xyz_activation, scale_activation):
        super().__init__()
        if scale_activation != "sigmoid":
            raise NotImplementedError(
                f"scale_activation={scale_activation!r}: the reference leaves the scale unbound for anything but 'sigmoid' "
                f"({where}) and raises; only 'sigmoid' is supported")
        if semantics and semantic_dim is None:
            raise ValueError("semantics=True needs semantic_dim")
        S = int(semantic_dim) if semantics else 0
        self.embed_dims, self.pc_range, self.scale_range = embed_dims, pc_range, scale_range
        self.output_dim = 10 + (1 if include_opa else 0) + S
        self._cfg = refine_config(version, pc_range, scale_range, unit, restrict_xyz, refine_manual, S, include_opa,
                                  semantics_activation, xyz_activation)
        self.layers = refinement_mlp(embed_dims, self.output_dim)

    def _takes_launch(self, switch, with_grad, instance_feature, anchor, anchor_embed):
        """Whether a call goes to the one-launch route behind ``switch``: ``embed_dims`` 128, fp32 GPU tensors, and a call that
        autograd would record exactly when ``with_grad``."""
        tensors = (instance_feature, anchor, anchor_embed, *self.layers.parameters())
        return switch and self.embed_dims == 128 and _lib.needs_grad(tensors) == with_grad and _lib.native_tensors(tensors)

    def _takes_fused(self, instance_feature, anchor, anchor_embed):
        return self._takes_launch(self.fused_mlp, False, instance_feature, anchor, anchor_embed)

    def _takes_native_training(self, instance_feature, anchor, anchor_embed):
        return self._takes_launch(self.native_training, True, instance_feature, anchor, anchor_embed)

    def forward(self, instance_feature, anchor, anchor_embed):
        if self._takes_fused(instance_feature, anchor, anchor_embed):
            return refine_fused(instance_feature, anchor, anchor_embed, self, self._cfg)
        if self._takes_native_training(instance_feature, anchor, anchor_embed):
            return refine_fused_autograd(instance_feature, anchor, anchor_embed, self, self._cfg)
        return refine(self.layers(instance_feature + anchor_embed), anchor, self._cfg)


class SparseGaussian3DRefinementModule(_Refinement):
    """Same constructor keys, parameters and ``forward(instance_feature, anchor, anchor_embed) -> (anchor,
    GaussianPrediction)`` as the reference class (refine_module.py:11-123); further config keys go to ``**kwargs`` as there."""

    def __init__(self, embed_dims=256, pc_range=None, scale_range=None, restrict_xyz=False, unit_xyz=None, refine_manual=None,
                 semantics=False, semantic_dim=None, include_opa=True, semantics_activation="softmax",
                 xyz_activation="sigmoid", scale_activation="sigmoid", **kwargs):
        if not isinstance(refine_manual, list):
            raise TypeError("refine_manual must be a list (refine_module.py:55)")
        unit = None
        if restrict_xyz:   # the step per axis as a share of the range; the sigmoid's slope at 0 is 1/4 (refine_module.py:48-53)
            if unit_xyz is None:
                raise ValueError("restrict_xyz=True needs unit_xyz")
            gain = 4 if xyz_activation == "sigmoid" else 1
            unit = [gain * (unit_xyz[i] / (pc_range[i + 3] - pc_range[i])) for i in range(3)]
        super().__init__(1, "refine_module.py:106-108", embed_dims, pc_range, scale_range, unit, restrict_xyz, refine_manual,
                         semantics, semantic_dim, include_opa, semantics_activation, xyz_activation, scale_activation)


class SparseGaussian3DRefinementModuleV2(_Refinement):
    """The same for refine_module_v2.py:12-108; ``unit_xyz`` is a non-persistent buffer as there."""

    def __init__(self, embed_dims=256, pc_range=None, scale_range=None, unit_xyz=None, semantics=False, semantic_dim=None,
                 include_opa=True, semantics_activation="softmax", xyz_activation="sigmoid", scale_activation="sigmoid",
                 **kwargs):
        # the library takes the buffer's values from the host: the constructor's, rounded to the buffer's float32
        unit = [float(np.float32(v)) for v in unit_xyz]
        super().__init__(2, "refine_module_v2.py:88-90", embed_dims, pc_range, scale_range, unit, False, (), semantics,
                         semantic_dim, include_opa, semantics_activation, xyz_activation, scale_activation)
        self.register_buffer("unit_xyz", torch.tensor(unit_xyz, dtype=torch.float), persistent=False)
