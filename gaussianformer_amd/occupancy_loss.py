"""Occupancy loss (weighted cross-entropy + Lovász-softmax) as one differentiable HIP op.

``occupancy_loss`` computes, for a list of L decoder layers, what ``OccupancyLoss.loss_voxel``
(loss/occupancy_loss.py:104-149) computes for the shipped configs; ``OccupancyLoss`` takes the reference
constructor's keyword arguments and its ``forward(inputs)`` dict contract (loss/base_loss.py).  Forward and backward are
HIP kernels (csrc/occ_loss.hip) with no host synchronisation.  Forward and backward can be captured in one
graph, on torch's condition that no autograd graph of an eager run is alive at the capture (keep only detached results):
a live one leaves the leaves' AccumulateGrad nodes on the default stream, and any captured backward then breaks.

Contract
--------
Inputs: ``pred_occ``, a list of L (1 <= L <= 8) fp32 tensors ``[1, C, N]`` with C = 18 -- either the head's
``semantics[None].transpose(1, 2)`` (a transposed view of a contiguous ``[1, N, C]`` tensor, read in place) or a
contiguous ``[1, C, N]`` tensor; all layers share one layout.  ``sampled_label`` ``[1, N]`` integer; optional ``occ_mask``
(bool, anything that flattens to ``[N]``).

    loss = (1/L) * sum_layers (ce_weight * CE + lovasz_weight * Lovasz [+ sem_scal_weight * sem + geo_scal_weight * geo])

over the voxels kept by ``occ_mask`` and, with ``ignore_empty``, by ``label != empty_label``.

* CE, softmax mode: ``sum w[y] * (-log softmax(x)[y]) / sum w[y]`` over kept voxels with ``y != ignore_index``
  (``nn.CrossEntropyLoss(weight, ignore_index, reduction="mean")``).  Prob mode (``use_softmax=False``): the same with
  ``log(clamp(p, 1e-6, 1 - 1e-6))``, whose gradient passes only where ``1e-6 <= p <= 1 - 1e-6`` (endpoints included, as
  ``torch.clamp``).  If every kept voxel is ignored the CE is 0/0 = NaN, as in torch.
* Lovász-softmax on ``p`` (the softmax, or the input in prob mode) over the kept voxels whose label is not ``lovasz_ignore``.
  Voxels labelled ``ignore_index`` are NOT dropped: the reference removes only ``lovasz_ignore``, so they count as
  background of every class -- mirrored here on purpose.  For each class c present among these voxels (``G_c > 0``):
  errors ``e = |fg - p_c|`` sorted in descending order, **ties to the lower voxel index** (this op's own rule: torch's tie
  order is unspecified), and ``sum_i e_(i) * (J_i - J_{i-1})`` with ``J_i = 1 - (G - F_i) / (G + B_i)`` (``lovasz_grad``,
  evaluated in fp32 as the reference does), ``F_i`` / ``B_i`` the foreground / background counts among the first i.  The
  Lovász term is the mean over present classes, 0 if none.  ``d|.|/dx`` is 0 at 0, as torch defines it (this matters in
  prob mode, where the prob head produces exact zeros).
* A non-finite input on a voxel that enters either term, or a label outside ``[0, C)`` that is not ``ignore_index``, makes
  the loss NaN (flagged on the device; no host check).

* The scene-class affinity terms (``sem_scal_loss`` / ``geo_scal_loss``, loss/occupancy_loss.py:185-268; only with
  ``sem_scal_weight`` or ``geo_scal_weight``).  ``V`` = the CE's voxels (kept, ``y != ignore_index``, ``0 <= y < C``); per
  layer ``S_c = sum_V p_c``, ``N_c = sum_{V, y=c} p_c`` (accumulated in double in a fixed order, each rounded to fp32 once),
  ``T_c = #{V, y=c}``, ``eps = 1e-5``; every ratio and ``f`` below is evaluated in fp32, operation by operation.
  ``f(x)`` is ``binary_cross_entropy_with_logits(inverse_sigmoid(x), 1)``: while ``x >= float32(1 - 1e-5)``: ``x -= 1e-5``;
  while ``x < 1e-5``: ``x += 1e-5``; ``f = softplus(log(1/x - 1))`` (``-log x`` in exact arithmetic), ``f' = -1/x`` at the
  shifted ``x`` (the shifts pass gradient 1).  The loops run on the device, at most 8 steps each (a ratio of probabilities
  needs 3); a ratio still out of range then -- inputs that are no probabilities, prob mode only -- makes the loss NaN.
  ``sem = (1/count) sum_i [f(N_i/(S_i+eps)) if S_i > 0] + f(N_i/(T_i+eps)) + [f(((|V|-T_i) - (S_i-N_i)) / ((|V|-T_i)+eps)) if
  |V| > T_i]`` over the classes ``i`` in ``0 .. C-2`` with ``T_i > 0``, ``count`` of them; ``count == 0`` gives NaN (the
  reference divides by zero in Python).  ``geo``, with ``e = empty_label`` in ``[0, C)`` and ``I = (|V|-T_e) - (S_e-N_e)``:
  ``f(I/((|V|-S_e)+eps)) + f(I/((|V|-T_e)+eps)) + f(N_e/(T_e+eps))``, no guards, as the reference.  The gradient is
  ``a_c + b_c [y = c]`` in ``p``-space on the voxels of ``V`` (Lovász voxels or not), through the softmax Jacobian in softmax
  mode.  The NaN rules below apply to the voxels of ``V``.

The loss is bitwise reproducible: every partial is summed in a fixed order, with no float atomics.  ``use_lovasz=False``
computes the CE term alone (the reference's ``use_lovasz_loss=False``): no sort, and non-finite inputs count only on CE
voxels.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

_C = _lib.GF_NUM_CHANNELS


def _layout(pred_occ):
    if not isinstance(pred_occ, (list, tuple)) or not 1 <= len(pred_occ) <= _lib.GF_OCC_MAX_LAYERS:
        raise ValueError(f"pred_occ must be a list of 1..{_lib.GF_OCC_MAX_LAYERS} tensors")
    p0 = pred_occ[0]
    _lib.require_gpu(*pred_occ)
    if p0.dim() != 3 or p0.shape[0] != 1 or p0.shape[1] != _C:
        raise ValueError(f"each pred_occ entry must be [1, {_C}, N]; got {tuple(p0.shape)}")
    for p in pred_occ:
        if p.dtype != torch.float32:
            raise ValueError(f"pred_occ must be float32; got {p.dtype}")
        if p.shape != p0.shape or p.stride()[1:] != p0.stride()[1:]:
            raise ValueError("every layer of pred_occ must have the same shape and layout")
    sc, sn = p0.stride(1), p0.stride(2)
    if sc < 1 or sn < 1:
        raise ValueError(f"unsupported pred_occ strides {p0.stride()}")
    return p0.shape[2], sc, sn


class _OccLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, label, mask, class_weights, *preds):
        L = len(preds)
        N, sc, sn = _layout(list(preds))
        lib = _lib.load()
        dev = preds[0].device
        nbytes = lib.gf_occ_loss_workspace_bytes(L, N, _C, cfg["flags"])
        if nbytes == 0:
            raise ValueError(f"gf_occ_loss_workspace_bytes refused L={L}, N={N}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # kept for the backward
        sbytes = lib.gf_occ_loss_scratch_bytes(L, N, _C, cfg["flags"])
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)     # the forward's own: freed when it returns
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ptrs = (ctypes.c_void_p * L)(*[p.data_ptr() for p in preds])
        _lib.call("gf_occ_loss_scal_forward" if cfg["scal"] else "gf_occ_loss_forward", dev, L, N, _C, cfg["flags"], ptrs, sc, sn,
                  label, mask, class_weights, cfg["ce_weight"], cfg["lovasz_weight"], *cfg["scal"], cfg["lovasz_ignore"],
                  cfg["ignore_index"], cfg["empty_label"], loss, ws, nbytes, scratch, sbytes)
        ctx.cfg, ctx.layout = cfg, (N, sc, sn)
        ctx.save_for_backward(label, mask, class_weights, ws, *preds)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        label, mask, class_weights, ws, *preds = ctx.saved_tensors
        cfg, (N, sc, sn) = ctx.cfg, ctx.layout
        L = len(preds)
        dev = preds[0].device
        grads = [torch.empty_strided(p.shape, p.stride(), dtype=torch.float32, device=dev) for p in preds]
        g = _lib.as_arg(grad_loss)
        pp = (ctypes.c_void_p * L)(*[p.data_ptr() for p in preds])
        gp = (ctypes.c_void_p * L)(*[t.data_ptr() for t in grads])
        _lib.call("gf_occ_loss_scal_backward" if cfg["scal"] else "gf_occ_loss_backward", dev, L, N, _C, cfg["flags"], pp, sc, sn,
                  label, mask, class_weights, cfg["ce_weight"], cfg["lovasz_weight"], *cfg["scal"], cfg["lovasz_ignore"],
                  cfg["ignore_index"], cfg["empty_label"], g, gp, ws, ws.numel())
        return (None, None, None, None, *grads)


def occupancy_loss(pred_occ, sampled_label, occ_mask=None, *, class_weights, ce_weight=1.0, lovasz_weight=1.0,
                   lovasz_ignore=None, use_softmax=True, ignore_index=255, empty_label=17, ignore_empty=False, use_lovasz=True,
                   sem_scal_weight=None, geo_scal_weight=None):
    """The occupancy loss of the module docstring for ``pred_occ`` (list of ``[1, C, N]``); returns a 0-dim tensor.
    No ``.item()``, ``nonzero()`` or boolean indexing: forward and backward never wait for the device.

    ``sem_scal_weight`` / ``geo_scal_weight``: with both ``None`` the loss is CE + Lovász, by ``gf_occ_loss_*``.  With either
    given, the scene-class affinity terms are added by ``gf_occ_loss_scal_*`` (the one not given weighs 0).  Where the
    reference's ``sem_scal_loss`` divides by zero in Python -- no class of ``0 .. C-2`` among the voxels of ``V`` -- the loss
    is NaN, flagged on the device; so it is for a ratio that more than 8 shift steps do not bring into range."""
    pred_occ = list(pred_occ)
    N, _, _ = _layout(pred_occ)
    dev = pred_occ[0].device
    label = sampled_label.reshape(-1)
    if label.numel() != N:
        raise ValueError(f"sampled_label has {label.numel()} entries, pred_occ {N} voxels")
    if label.dtype != torch.int64:
        label = label.to(torch.int64)
    label = label.contiguous()
    flags = 0 if use_softmax else _lib.GF_OCC_PROB
    mask = None
    if occ_mask is not None:
        mask = occ_mask.reshape(-1)
        if mask.numel() != N or mask.dtype != torch.bool:
            raise ValueError("occ_mask must be bool and flatten to [N]")
        mask = mask.contiguous().view(torch.uint8)
        flags |= _lib.GF_OCC_MASK
    if lovasz_ignore is not None:
        flags |= _lib.GF_OCC_LOVASZ_IGNORE
    if ignore_empty:
        flags |= _lib.GF_OCC_IGNORE_EMPTY
    if not use_lovasz:
        flags |= _lib.GF_OCC_NO_LOVASZ
    _lib.require_gpu(label, mask)
    cw = torch.as_tensor(class_weights, dtype=torch.float32, device=dev).reshape(-1).contiguous()
    if cw.numel() != _C:
        raise ValueError(f"class_weights must have {_C} entries")
    scal = ()
    if sem_scal_weight is not None or geo_scal_weight is not None:
        if not 0 <= int(empty_label) < _C:
            raise ValueError(f"empty_label={empty_label}: the geo_scal term needs a class in [0, {_C})")
        flags |= _lib.GF_OCC_SCAL
        scal = (float(sem_scal_weight or 0.0), float(geo_scal_weight or 0.0))
    cfg = dict(flags=flags, scal=scal, ce_weight=float(ce_weight), lovasz_weight=float(lovasz_weight),
               lovasz_ignore=int(lovasz_ignore) if lovasz_ignore is not None else 0, ignore_index=int(ignore_index),
               empty_label=int(empty_label))
    return _OccLoss.apply(cfg, label, mask, cw, *pred_occ)


class OccupancyLoss(nn.Module):
    """Drop-in for the reference's ``OccupancyLoss`` (register it in its place): the same constructor keywords and the
    ``forward(inputs)`` dict contract of ``BaseLoss`` (``weight * loss_voxel(**{k: inputs[v] for k, v in input_dict})``).
    Options this op does not cover raise ``ValueError`` naming them.

    ``native_scal``: opt-in for ``use_sem_geo_scal_loss=True`` (the reference's default).  Set the class attribute to ``True``
    and the constructor accepts the option: the two affinity terms run in the HIP op, weighted by
    ``loss_voxel_sem_scal_weight`` and ``loss_voxel_geo_scal_weight`` of ``multi_loss_weights`` (default 1.0)."""

    native_scal = False

    def __init__(self, weight=1.0, empty_label=17, num_classes=18, use_focal_loss=False, focal_loss_args=dict(),
                 use_dice_loss=False, balance_cls_weight=False, multi_loss_weights=dict(), use_sem_geo_scal_loss=True,
                 use_lovasz_loss=True, lovasz_ignore=255, manual_class_weight=None, ignore_empty=False,
                 lovasz_use_softmax=True, input_dict=None):
        super().__init__()
        if use_focal_loss:
            raise ValueError("OccupancyLoss: use_focal_loss is not supported by the HIP op")
        if use_dice_loss:
            raise ValueError("OccupancyLoss: use_dice_loss is not supported by the HIP op")
        if use_sem_geo_scal_loss and not self.native_scal:
            raise ValueError("OccupancyLoss: use_sem_geo_scal_loss is off by default in the HIP op (the shipped configs set it "
                             "False); set OccupancyLoss.native_scal = True to run the two terms natively")
        if balance_cls_weight and manual_class_weight is None:
            raise ValueError("OccupancyLoss: balance_cls_weight without manual_class_weight is not supported")
        if num_classes != _C:
            raise ValueError(f"OccupancyLoss: num_classes={num_classes}; the HIP op supports {_C}")
        self.weight = weight
        self.input_dict = input_dict if input_dict is not None else {
            'pred_occ': 'pred_occ', 'sampled_xyz': 'sampled_xyz', 'sampled_label': 'sampled_label', 'occ_mask': 'occ_mask'}
        self.empty_label = empty_label
        self.num_classes = num_classes
        self.use_sem_geo_scal_loss = use_sem_geo_scal_loss
        self.use_lovasz_loss = use_lovasz_loss
        self.lovasz_ignore = lovasz_ignore
        self.ignore_empty = ignore_empty
        self.lovasz_use_softmax = lovasz_use_softmax
        self.loss_voxel_ce_weight = multi_loss_weights.get('loss_voxel_ce_weight', 1.0)
        self.loss_voxel_sem_scal_weight = multi_loss_weights.get('loss_voxel_sem_scal_weight', 1.0)
        self.loss_voxel_geo_scal_weight = multi_loss_weights.get('loss_voxel_geo_scal_weight', 1.0)
        self.loss_voxel_lovasz_weight = multi_loss_weights.get('loss_voxel_lovasz_weight', 1.0)
        if balance_cls_weight:
            # as the reference: num_classes * L1-normalised manual weights, in fp32
            w = num_classes * F.normalize(torch.tensor(manual_class_weight), 1, -1)
        else:
            w = torch.ones(num_classes)
        self.register_buffer("class_weights", w.to(torch.float32), persistent=False)

    def loss_voxel(self, pred_occ, sampled_xyz, sampled_label, occ_mask=None):
        return occupancy_loss(pred_occ, sampled_label, occ_mask, class_weights=self.class_weights.to(pred_occ[0].device),
                              ce_weight=self.loss_voxel_ce_weight,
                              lovasz_weight=self.loss_voxel_lovasz_weight, lovasz_ignore=self.lovasz_ignore,
                              use_softmax=self.lovasz_use_softmax, ignore_index=255, empty_label=self.empty_label,
                              ignore_empty=self.ignore_empty, use_lovasz=self.use_lovasz_loss,
                              sem_scal_weight=self.loss_voxel_sem_scal_weight if self.use_sem_geo_scal_loss else None,
                              geo_scal_weight=self.loss_voxel_geo_scal_weight if self.use_sem_geo_scal_loss else None)

    def forward(self, inputs):
        actual = {k: inputs[v] for k, v in self.input_dict.items()}
        return self.weight * self.loss_voxel(**actual)
