"""Fused caller-side preparation of the deformable aggregation.

Host mirror of the block between the ``weights_fc`` GEMM and ``DAF.apply`` in
``DeformableFeatureAggregation.forward`` (model/encoder/gaussian_encoder/deformable_module.py:
174-214) and of ``project_points`` (:268-285), backed by ``gf_daf_prepare`` /
``gf_daf_prepare_backward`` (include/gf_hip.h).  One kernel reads the raw attention logits
once and writes the sampling locations and the softmaxed weights in the layouts ``DAF.apply``
takes; the reference runs ~15 permute / mask / softmax kernels over the 88-498 MB tensor.
"""
import torch
from torch.autograd.function import Function, once_differentiable

from . import _lib
from ._lib import as_arg

f32 = torch.float32


class DeformablePrepareFunction(Function):
    """``(points_2d [bs, A*pts, cams, 2], weights [bs, A*pts, cams, L, G]) =
    apply(key_points [bs,A,pts,3], projection_mat [bs,cams,4,4], image_wh [bs,cams,2] | None,
    raw_weights [bs,A,cams,L,pts,G], weight_mask bool same shape | None)``."""

    @staticmethod
    def forward(ctx, key_points, projection_mat, image_wh, raw_weights, weight_mask):
        _lib.require_gpu(key_points, projection_mat, image_wh, raw_weights, weight_mask)
        kp, pm, wh, raw = as_arg(key_points), as_arg(projection_mat), as_arg(image_wh), as_arg(raw_weights)
        wm = as_arg(weight_mask, torch.uint8)
        B, A, pts = kp.shape[:3]
        cams, L, G = raw.shape[2], raw.shape[3], raw.shape[5]
        assert raw.shape == (B, A, cams, L, pts, G) and pm.shape == (B, cams, 4, 4)
        points_2d = torch.empty(B, A * pts, cams, 2, dtype=f32, device=kp.device)
        weights = torch.empty(B, A * pts, cams, L, G, dtype=f32, device=kp.device)
        _lib.call("gf_daf_prepare", kp.device, B, A, pts, cams, L, G, kp, pm, wh, raw, wm, points_2d, weights)
        ctx.save_for_backward(kp, pm, wh if wh is not None else torch.empty(0, device=kp.device), weights)
        ctx.has_wh = wh is not None
        ctx.dims = (B, A, pts, cams, L, G)
        ctx.mark_non_differentiable()
        return points_2d, weights

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_points_2d, grad_weights):
        kp, pm, wh, weights = ctx.saved_tensors
        B, A, pts, cams, L, G = ctx.dims
        need_kp, need_raw = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        g_kp = torch.empty_like(kp) if need_kp else None
        g_raw = torch.empty(B, A, cams, L, pts, G, dtype=f32, device=kp.device) if need_raw else None
        _lib.call("gf_daf_prepare_backward", kp.device, B, A, pts, cams, L, G, kp, pm, wh if ctx.has_wh else None, weights,
                  as_arg(grad_weights), as_arg(grad_points_2d), g_raw, g_kp)
        return g_kp, None, None, g_raw, None


def deformable_prepare(key_points, projection_mat, image_wh, raw_weights, weight_mask=None):
    """Functional form; see :class:`DeformablePrepareFunction`."""
    return DeformablePrepareFunction.apply(key_points, projection_mat, image_wh, raw_weights, weight_mask)


def deformable_fused_forward(key_points, projection_mat, image_wh, mc_ms_feat, spatial_shape, scale_start_index,
                             raw_weights=None, raw_anchor=None, raw_cam=None):
    """INFERENCE only (no autograd): ``features [bs, A, C]`` of ``DeformableFeatureAggregation.forward`` -- project_points,
    mask / all_miss / softmax, ``DAF.apply`` and ``features.sum(dim=2)`` (deformable_module.py:174-233,242) -- in ONE launch
    (``gf_daf_fused_forward``): no ``[A*pts, cams, L, G]`` weights tensor, no ``[A*pts, C]`` sampled features.
    The attention logits come either as ``raw_weights [bs, A, cams, L, pts, G]`` (the ``weights_fc`` output as the reference
    reshapes it, :243-253) or -- ``use_camera_embed``, where ``weights_fc`` acts on ``feature + camera_embed`` and is linear
    (:253-262) -- as its two parts ``raw_anchor [bs, A, L, pts, G]`` and ``raw_cam [bs, cams, L, pts, G]``, added on the fly."""
    _lib.require_gpu(key_points, projection_mat, image_wh, mc_ms_feat, spatial_shape, scale_start_index, raw_weights, raw_anchor, raw_cam)
    if any(t is not None and t.requires_grad for t in (key_points, mc_ms_feat, raw_weights, raw_anchor, raw_cam)) and torch.is_grad_enabled():
        raise RuntimeError("deformable_fused_forward computes no gradients: use deformable_prepare + DeformableAggregationFunction "
                           "for training, or call it under torch.no_grad()")
    kp, pm, wh = as_arg(key_points), as_arg(projection_mat), as_arg(image_wh)
    raw, ra, rc_ = as_arg(raw_weights), as_arg(raw_anchor), as_arg(raw_cam)
    feat = as_arg(mc_ms_feat)
    B, A, pts = kp.shape[:3]
    cams, num_feat, C = feat.shape[1], feat.shape[2], feat.shape[3]
    L = spatial_shape.shape[0]
    if raw is not None:
        G = raw.shape[5]
        assert raw.shape == (B, A, cams, L, pts, G) and ra is None and rc_ is None
    else:
        G = ra.shape[4]
        assert ra.shape == (B, A, L, pts, G) and rc_.shape == (B, cams, L, pts, G)
    assert pm.shape == (B, cams, 4, 4)
    ss, st = as_arg(spatial_shape, torch.int32), as_arg(scale_start_index, torch.int32)
    out = torch.empty(B, A, C, dtype=f32, device=kp.device)
    _lib.call("gf_daf_fused_forward", kp.device, B, A, pts, cams, L, G, C, num_feat, kp, pm, wh, raw, ra, rc_, feat, ss, st, out)
    return out


def _mask_u8(weight_mask):
    """The keep-mask as bytes without a copy where it already is one byte per entry (bool / uint8)."""
    if weight_mask is None:
        return None
    m = weight_mask.detach()
    return (m if m.dtype in (torch.bool, torch.uint8) else m.to(torch.uint8)).contiguous()


class DeformableFusedFunction(Function):
    """``features [bs, A, C] = apply(key_points, projection_mat, image_wh, mc_ms_feat, spatial_shape, scale_start_index,
    raw_weights, raw_anchor, raw_cam, weight_mask)``: the training form of :func:`deformable_fused_forward`, backed by
    ``gf_daf_fused_forward_masked`` / ``gf_daf_fused_backward``.  Differentiable in ``key_points``, ``mc_ms_feat`` and the logits;
    the context keeps the inputs only (the backward forms the projection and the softmax again)."""

    @staticmethod
    def forward(ctx, key_points, projection_mat, image_wh, mc_ms_feat, spatial_shape, scale_start_index,
                raw_weights, raw_anchor, raw_cam, weight_mask):
        _lib.require_gpu(key_points, projection_mat, image_wh, mc_ms_feat, spatial_shape, scale_start_index, raw_weights,
                         raw_anchor, raw_cam, weight_mask)
        kp, pm, wh = as_arg(key_points), as_arg(projection_mat), as_arg(image_wh)
        raw, ra, rc_ = as_arg(raw_weights), as_arg(raw_anchor), as_arg(raw_cam)
        feat, wm = as_arg(mc_ms_feat), _mask_u8(weight_mask)
        B, A, pts = kp.shape[:3]
        cams, num_feat, C = feat.shape[1], feat.shape[2], feat.shape[3]
        L = spatial_shape.shape[0]
        if raw is not None:
            if ra is not None or rc_ is not None:
                raise ValueError("give raw_weights, or raw_anchor and raw_cam")
            G = raw.shape[5]
            assert raw.shape == (B, A, cams, L, pts, G)
        else:
            if ra is None or rc_ is None:
                raise ValueError("give raw_weights, or raw_anchor and raw_cam")
            G = ra.shape[4]
            assert ra.shape == (B, A, L, pts, G) and rc_.shape == (B, cams, L, pts, G)
        assert pm.shape == (B, cams, 4, 4) and feat.shape[0] == B
        assert wm is None or wm.shape == (B, A, cams, L, pts, G)
        ss, st = as_arg(spatial_shape, torch.int32), as_arg(scale_start_index, torch.int32)
        out = torch.empty(B, A, C, dtype=f32, device=kp.device)
        _lib.call("gf_daf_fused_forward_masked", kp.device, B, A, pts, cams, L, G, C, num_feat, kp, pm, wh, raw, ra, rc_, wm,
                  feat, ss, st, out)
        ctx.save_for_backward(kp, pm, wh, feat, ss, st, raw, ra, rc_, wm)
        ctx.dims = (B, A, pts, cams, L, G, C, num_feat)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        kp, pm, wh, feat, ss, st, raw, ra, rc_, wm = ctx.saved_tensors
        B, A, pts, cams, L, G, C, num_feat = ctx.dims
        need = ctx.needs_input_grad
        dev = kp.device
        g_kp = torch.empty_like(kp) if need[0] else None
        g_feat = torch.zeros_like(feat) if need[3] else None
        g_raw = torch.empty_like(raw) if raw is not None and need[6] else None
        g_ra = torch.empty_like(ra) if ra is not None and need[7] else None
        g_rc = torch.empty_like(rc_) if rc_ is not None and need[8] else None
        if not any(t is not None for t in (g_kp, g_feat, g_raw, g_ra, g_rc)):
            return (None,) * 10
        lib = _lib.load()
        go = as_arg(grad_out)
        ws_bytes = lib.gf_daf_fused_backward_workspace_bytes(B, A, pts, cams, L, G) if g_rc is not None else 0
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev) if g_rc is not None else None
        _lib.call("gf_daf_fused_backward", dev, B, A, pts, cams, L, G, C, num_feat, kp, pm, wh, raw, ra, rc_, wm, feat, ss, st,
                  go, g_feat, g_kp, g_raw, g_ra, g_rc, ws, ws_bytes)
        return g_kp, None, None, g_feat, None, None, g_raw, g_ra, g_rc, None


def deformable_fused(key_points, projection_mat, image_wh, mc_ms_feat, spatial_shape, scale_start_index,
                     raw_weights=None, raw_anchor=None, raw_cam=None, weight_mask=None):
    """``features [bs, A, C]`` of ``DeformableFeatureAggregation.forward`` for TRAINING (deformable_module.py:174-242): the
    one-launch block of :func:`deformable_fused_forward` with the attention-dropout keep-mask ``weight_mask``
    (``[bs, A, cams, L, pts, G]``, bool / uint8, ``True`` = keep; the reference draws it with ``torch.rand_like(weights) >
    attn_drop``, :263-282) and a backward (``gf_daf_fused_backward``) into ``key_points``, ``mc_ms_feat`` (and through it
    ``DAF.feature_maps_format`` to the pyramid levels) and the logits -- ``raw_weights`` or ``raw_anchor`` + ``raw_cam``.
    No ``[A*pts, cams, L, G]`` weights tensor and no ``[A*pts, C]`` sampled features in either direction."""
    return DeformableFusedFunction.apply(key_points, projection_mat, image_wh, mc_ms_feat, spatial_shape, scale_start_index,
                                         raw_weights, raw_anchor, raw_cam, weight_mask)
