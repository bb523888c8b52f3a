"""GaussianFormer-2's pixel lifting and pixel loss as HIP ops (csrc/lifter.hip).

``lift_pixels`` does the per-frame pixel work of ``GaussianLifterV2.forward`` from the pixel logits to the FPS call
(model/lifter/gaussian_lifter_v2.py:169-233, model/utils/sampler.py): the per-batch candidate points in row-major
(camera, row, column, sample) order and, unless asked not to, the ``pixel_gt`` target.  ``pixel_distribution_loss`` is
``PixelDistributionLoss.loss_voxel`` (loss/bce_loss.py:60-87) with its backward.  ``PixelDistributionLoss`` and
``GaussianLifterV2`` are drop-ins with the reference's constructors, parameter and buffer names and forward contracts.

Semantics (include/gf_hip.h has the full statement):

* rays: ``u = (j + 0.5) / w * image_w``, ``v = (i + 0.5) / h * image_h`` in fp32; bin ``k``'s point is
  ``img2lidar @ (u d_k, v d_k, d_k, 1)`` with ``img2lidar = projection_mat.inverse()`` (torch's, in the wrapper);
* ``pdf = softmax(logits)`` over ``S + 1`` entries; a pixel is disabled when ``argmax(pdf) == S`` (the argmax, not the
  sample; ties to the lower index);
* stochastic sampling (``uniforms`` given): ``index = #{k : cdf_k <= u}`` clipped to ``S`` with
  ``cdf = cumsum(pdf / (FLT_EPSILON + sum pdf))``; deterministic: the top ``a`` entries of the pdf, ties to the lower
  index; the candidate is the point of bin ``min(index, S - 1)``, dropped when out of ``pc_range`` (min inclusive, max
  exclusive);
* ``pixel_gt[..., k] = in_range(p_k) & occ_label[idx] != empty_label & occ_cam_mask[idx]`` with
  ``idx = trunc((p - pc_min) / voxel_size)`` clamped to the grid, and ``pixel_gt[..., S] = ~any(pixel_gt[..., :S])``.

``lift_pixels`` reads the candidate counts back once per call (a host synchronisation, as FPS needs host offsets anyway),
so it cannot be captured in a graph.  The points carry no gradient, as in the reference.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .sampling import farthest_point_sampling

MAX_BINS = _lib.GF_LIFT_MAX_BINS
MAX_ANCHORS = _lib.GF_LIFT_MAX_ANCHORS


def pack_occupancy(occ_label, occ_cam_mask, empty_label=17):
    """``[b, X, Y, Z]`` uint8: 1 where ``occ_label != empty_label`` and ``occ_cam_mask`` (the table the lift kernel reads)."""
    occ = occ_label != empty_label
    if occ_cam_mask is not None:
        occ = occ & occ_cam_mask.to(torch.bool)
    return occ.to(torch.uint8).contiguous()


def lift_pixels(logits, projection_mat, image_wh, *, depth_bins, pc_range, voxel_size, occ_resolution, anchors_per_pixel,
                uniforms=None, occ_label=None, occ_cam_mask=None, empty_label=17, return_src=False):
    """Candidate points and ``pixel_gt`` of ``logits [b, n, h, w, S + 1]``.

    ``projection_mat [b, n, 4, 4]`` (lidar to image; inverted here with torch), ``image_wh [b, n, 2]``, ``depth_bins [S]``.
    ``uniforms [b, n, h, w, a]`` selects stochastic sampling (None: deterministic top-a).  ``pixel_gt`` is computed when
    ``occ_label`` is given (``occ_cam_mask`` then too, or None for all-valid).  Returns ``(scans, pixel_gt)``: ``scans`` a
    list of ``b`` tensors ``[count_i, 3]`` (views of one padded buffer), ``pixel_gt [b, n, h, w, S + 1]`` bool or None;
    with ``return_src=True`` also a list of ``b`` int32 tensors, the slot ``(cam h w + row w + col) a + sample`` of each
    candidate."""
    _lib.require_gpu(logits, projection_mat, image_wh, depth_bins, uniforms, occ_label, occ_cam_mask)
    if logits.dim() != 5:
        raise ValueError(f"lift_pixels: logits must be [b, n, h, w, S + 1], got {tuple(logits.shape)}")
    b, n, h, w, nb = logits.shape
    S, a = nb - 1, int(anchors_per_pixel)
    dev = logits.device
    if tuple(projection_mat.shape) != (b, n, 4, 4) or tuple(image_wh.shape) != (b, n, 2):
        raise ValueError(f"lift_pixels: projection_mat must be [{b}, {n}, 4, 4] and image_wh [{b}, {n}, 2]")
    if depth_bins.numel() != S:
        raise ValueError(f"lift_pixels: {depth_bins.numel()} depth bins for S = {S}")
    if uniforms is not None and tuple(uniforms.shape) != (b, n, h, w, a):
        raise ValueError(f"lift_pixels: uniforms must be [{b}, {n}, {h}, {w}, {a}], got {tuple(uniforms.shape)}")
    X, Y, Z = (int(r) for r in occ_resolution)
    lib = _lib.load()
    x, wh, d, u = (_lib.as_arg(t) for t in (logits, image_wh, depth_bins, uniforms))
    img2lidar = _lib.as_arg(projection_mat).inverse().contiguous()
    occ = gt = None
    if occ_label is not None:
        occ = pack_occupancy(occ_label, occ_cam_mask, empty_label)
        if tuple(occ.shape) != (b, X, Y, Z):
            raise ValueError(f"lift_pixels: occ_label must be [{b}, {X}, {Y}, {Z}], got {tuple(occ.shape)}")
        gt = torch.empty((b, n, h, w, nb), dtype=torch.uint8, device=dev)
    npix = n * h * w
    ws_bytes = lib.gf_lift_workspace_bytes(b, npix, a)
    if ws_bytes == 0:
        raise ValueError(f"lift_pixels: unsupported shape b={b}, n h w={npix}, a={a} (1 <= a <= {MAX_ANCHORS})")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    points = torch.empty((b, npix * a, 3), dtype=torch.float32, device=dev)
    counts = torch.empty(b, dtype=torch.int32, device=dev)
    src = torch.empty((b, npix * a), dtype=torch.int32, device=dev) if return_src else None
    pc = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    _lib.call("gf_lift_pixels", dev, b, n, h, w, S, a, x, img2lidar, wh, d, pc, float(voxel_size), X, Y, Z, occ, u, points,
              counts, src, gt, ws, ws_bytes)
    cnt = counts.cpu().tolist()   # the one host synchronisation of the call
    scans = [points[i, :c] for i, c in enumerate(cnt)]
    pixel_gt = None if gt is None else gt.view(torch.bool)
    if return_src:
        return scans, pixel_gt, [src[i, :c] for i, c in enumerate(cnt)]
    return scans, pixel_gt


class _PixelLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, gt, flags):
        lib = _lib.load()
        dev = logits.device
        nb = logits.shape[-1]
        rows = logits.numel() // nb
        ws_bytes = lib.gf_pixel_loss_workspace_bytes(rows, nb)
        if ws_bytes == 0:
            raise ValueError(f"pixel_distribution_loss: unsupported shape {tuple(logits.shape)} (last dim <= {MAX_BINS})")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.call("gf_pixel_loss_forward", dev, rows, nb, flags, logits, gt, loss, ws, ws_bytes)
        ctx.flags = flags
        ctx.save_for_backward(logits, gt)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        logits, gt = ctx.saved_tensors
        nb = logits.shape[-1]
        grad = torch.empty_like(logits)
        _lib.call("gf_pixel_loss_backward", logits.device, logits.numel() // nb, nb, ctx.flags, logits, gt,
                  _lib.as_arg(grad_loss), grad)
        return grad, None, None


def pixel_distribution_loss(pixel_logits, pixel_gt, use_sigmoid=True):
    """``binary_cross_entropy(softmax(pixel_logits, -1) or sigmoid(pixel_logits), pixel_gt.float())`` (mean over every
    entry, torch's clamp of the log at -100 and its backward floor of 1e-12 on ``p (1 - p)``); differentiable in
    ``pixel_logits``.  ``pixel_gt`` is bool with the logits' shape."""
    _lib.require_gpu(pixel_logits, pixel_gt)
    if pixel_gt.shape != pixel_logits.shape:
        raise ValueError(f"pixel_distribution_loss: pixel_gt {tuple(pixel_gt.shape)} != logits {tuple(pixel_logits.shape)}")
    if pixel_gt.dtype != torch.bool:
        raise ValueError(f"pixel_distribution_loss: pixel_gt must be bool, got {pixel_gt.dtype}")
    if pixel_logits.dtype != torch.float32:
        raise ValueError(f"pixel_distribution_loss: pixel_logits must be float32, got {pixel_logits.dtype}")
    flags = _lib.GF_PIXEL_LOSS_SIGMOID if use_sigmoid else _lib.GF_PIXEL_LOSS_SOFTMAX
    return _PixelLoss.apply(pixel_logits.contiguous(), pixel_gt.contiguous().view(torch.uint8), flags)


class PixelDistributionLoss(nn.Module):
    """Drop-in for the reference's ``PixelDistributionLoss``: the same constructor and the ``BaseLoss.forward(inputs)``
    dict contract (``weight * loss_voxel(**{k: inputs[v] for k, v in input_dict.items()})``)."""

    def __init__(self, weight=1.0, use_sigmoid=True, input_dict=None):
        super().__init__()
        self.weight = weight
        self.input_dict = input_dict if input_dict is not None else {'pixel_logits': 'pixel_logits', 'pixel_gt': 'pixel_gt'}
        self.use_sigmoid = use_sigmoid

    def loss_voxel(self, pixel_logits, pixel_gt):
        return pixel_distribution_loss(pixel_logits, pixel_gt, self.use_sigmoid)

    def forward(self, inputs):
        actual = {k: inputs[v] for k, v in self.input_dict.items()}
        return self.weight * self.loss_voxel(**actual)


_LOGIT_MAX = 0.9999


def _safe_inverse_sigmoid(x):
    x = torch.clamp(x, 1 - _LOGIT_MAX, _LOGIT_MAX)
    return torch.log(x / (1 - x))


class GaussianLifterV2(nn.Module):
    """Drop-in for the reference's ``GaussianLifterV2`` (model/lifter/gaussian_lifter_v2.py): the same constructor,
    parameter and buffer names (a reference checkpoint's ``state_dict`` loads) and ``forward(metas, **kwargs)`` output
    keys.  The pixel work runs in ``lift_pixels``; the padding of short scans, the random or FPS selection, the
    normalisation and the inverse sigmoid stay torch and draw from the same RNG streams in the same order
    (``torch.rand``, ``torch.randn_like``, ``np.random.*``), so a seeded run consumes what the reference consumes.
    ``initializer`` must be an ``nn.Module`` (a config dict needs mmseg, which this package does not use) or None, in which
    case ``forward`` takes ``secondfpn_out``.  A frame without any candidate raises ``RuntimeError``."""

    def __init__(self, num_anchor, embed_dims, anchor_grad=True, feat_grad=True, semantics=False, semantic_dim=None,
                 include_opa=True, xyz_activation="sigmoid", scale_activation="sigmoid", num_samples=64,
                 pc_range=[-50, -50, -5, 50, 50, 3], voxel_size=0.5, occ_resolution=[200, 200, 16], empty_label=17,
                 anchors_per_pixel=1, random_sampling=True, projection_in=None, initializer=None,
                 initializer_img_downsample=None, pretrained_path=None, deterministic=True, random_samples=0, **kwargs):
        super().__init__()
        self.embed_dims = embed_dims
        self.xyz_act = xyz_activation
        self.scale_act = scale_activation
        self.include_opa = include_opa
        self.semantics = semantics
        self.semantic_dim = semantic_dim
        self.random_samples = random_samples
        # construction order = RNG order of the reference: random anchors, semantic init, instance feature, projection
        if random_samples > 0:
            self.random_anchors = nn.Parameter(self._anchor_rows(random_samples, with_xyz=True), True)
        self.num_anchor = num_anchor
        self.anchor = nn.Parameter(self._anchor_rows(num_anchor, with_xyz=False), requires_grad=anchor_grad)
        self.instance_feature = nn.Parameter(torch.zeros([num_anchor + random_samples, embed_dims]), requires_grad=feat_grad)
        self.projection = nn.Sequential(nn.ReLU(), nn.Linear(embed_dims * 4 if projection_in is None else projection_in,
                                                             num_samples + 1))
        self.num_samples = num_samples
        self.register_buffer("depth_bins", torch.linspace(1.0, 72.0, num_samples, dtype=torch.float), persistent=False)
        self.register_buffer("pc_start", torch.tensor(pc_range[:3], dtype=torch.float), persistent=False)
        self.pc_range = pc_range
        self.voxel_size = voxel_size
        self.occ_resolution = occ_resolution
        self.empty_label = empty_label
        if not 1 <= anchors_per_pixel <= MAX_ANCHORS:
            raise ValueError(f"GaussianLifterV2: anchors_per_pixel={anchors_per_pixel}; 1..{MAX_ANCHORS} supported")
        self.anchors_per_pixel = anchors_per_pixel
        self.random_sampling = random_sampling
        if initializer is not None and not isinstance(initializer, nn.Module):
            raise ValueError("GaussianLifterV2: initializer must be an nn.Module (building one from a config needs mmseg, "
                             "which is not available here); pass secondfpn_out to forward instead")
        self.initialize_backbone = initializer
        self.initializer_img_downsample = initializer_img_downsample
        self.pretrained_path = pretrained_path
        self.deterministic = deterministic
        if pretrained_path is not None:
            ckpt = torch.load(pretrained_path, map_location='cpu')
            ckpt = dict(ckpt.get("state_dict", ckpt))
            ckpt.pop('instance_feature', None)
            ckpt.pop('anchor', None)
            print(self.load_state_dict(ckpt, strict=False))

    def _anchor_rows(self, count, with_xyz):
        """[xyz,] scale, rotation, opacity, semantics of ``count`` anchors, drawing the RNG as the reference does."""
        cols = []
        if with_xyz:
            xyz = torch.rand(count, 3, dtype=torch.float)
            cols.append(_safe_inverse_sigmoid(xyz) if self.xyz_act == "sigmoid" else xyz)
        scale = torch.full((count, 3), 0.5, dtype=torch.float)
        cols.append(_safe_inverse_sigmoid(scale) if self.scale_act == "sigmoid" else scale)
        rots = torch.zeros(count, 4, dtype=torch.float)
        rots[:, 0] = 1
        cols.append(rots)
        if self.include_opa:
            cols.append(_safe_inverse_sigmoid(torch.full((count, 1), 0.5, dtype=torch.float)))
        if self.semantics and self.semantic_dim is None:
            raise ValueError("GaussianLifterV2: semantics=True needs semantic_dim")
        cols.append(torch.randn(count, self.semantic_dim if self.semantics else 0, dtype=torch.float))
        return torch.cat(cols, dim=-1)

    def init_weights(self):
        if self.pretrained_path is None and self.instance_feature.requires_grad:
            torch.nn.init.xavier_uniform_(self.instance_feature.data, gain=1)

    def _clamp_to_range(self, pts):
        for ax in range(3):
            pts[:, ax].clamp_(self.pc_range[ax], self.pc_range[ax + 3])

    def _select(self, scan, benchmarking):
        """The per-element anchor selection after the candidates (padding, random choice or FPS)."""
        m = self.num_anchor
        have = scan.shape[0]
        if have == 0:
            raise RuntimeError("GaussianLifterV2: no candidate point in this frame (every pixel disabled or out of range)")
        if have < m:
            extra = scan.repeat(int(math.ceil(m * 1.0 / have)) - 1, 1)
            extra = extra + torch.randn_like(extra) * 0.1
            if self.random_sampling:
                extra = extra[np.random.choice(extra.shape[0], m - have, False)]
            self._clamp_to_range(extra)
            scan = torch.cat([scan, extra], 0)
        elif self.random_sampling:
            scan = scan[np.random.choice(have, m, False)]
        if self.random_sampling:
            return scan
        if benchmarking:
            scan = scan[np.random.permutation(scan.shape[0])]
            offsets = torch.linspace(0, scan.shape[0], 4, dtype=torch.int, device=scan.device)[1:]
            new_offsets = torch.linspace(0, m, 4, dtype=torch.int, device=scan.device)[1:]
        else:
            offsets = torch.tensor([scan.shape[0]], device=scan.device, dtype=torch.int)
            new_offsets = torch.tensor([m], device=scan.device, dtype=torch.int)
        idx = farthest_point_sampling(scan, offsets, new_offsets)
        return scan[idx.long(), :]

    def forward(self, metas, **kwargs):
        if self.initialize_backbone is not None:
            imgs = kwargs["imgs"]
            b, n = imgs.shape[:2]
            x = imgs.flatten(0, 1)
            if self.initializer_img_downsample is not None:
                x = nn.functional.interpolate(x, scale_factor=self.initializer_img_downsample, mode='bilinear',
                                              align_corners=True)
            secondfpn_out = self.initialize_backbone(x).unflatten(0, (b, n))
        else:
            secondfpn_out = kwargs["secondfpn_out"]
        b, n, _, h, w = secondfpn_out.shape
        logits = self.projection(secondfpn_out.permute(0, 1, 3, 4, 2))   # b, n, h, w, S + 1
        benchmarking = kwargs.get("benchmarking", False)
        a = self.anchors_per_pixel
        # the reference's sampler draws its uniforms here (after the softmax, on the logits' device)
        uniforms = None if getattr(self, 'deterministic', True) else torch.rand((b, n, h, w, a), device=logits.device)
        scans, pixel_gt = lift_pixels(
            logits, metas["projection_mat"], metas['image_wh'], depth_bins=self.depth_bins, pc_range=self.pc_range,
            voxel_size=self.voxel_size, occ_resolution=self.occ_resolution, anchors_per_pixel=a, uniforms=uniforms,
            occ_label=None if benchmarking else metas["occ_label"],
            occ_cam_mask=None if benchmarking else metas["occ_cam_mask"], empty_label=self.empty_label)
        anchor_xyz = torch.stack([self._select(scan, benchmarking) for scan in scans])
        # per axis (x - min) / (max - min), the extent formed in double and applied in fp32
        pr = self.pc_range
        lo = torch.tensor(pr[:3], dtype=anchor_xyz.dtype, device=anchor_xyz.device)
        ext = torch.tensor([pr[3] - pr[0], pr[4] - pr[1], pr[5] - pr[2]], dtype=anchor_xyz.dtype, device=anchor_xyz.device)
        anchor_xyz = (anchor_xyz - lo) / ext
        if self.xyz_act != "sigmoid":
            raise ValueError(f"GaussianLifterV2: xyz_activation={self.xyz_act!r} (the reference's forward supports only "
                             "'sigmoid')")
        anchor = torch.cat([_safe_inverse_sigmoid(anchor_xyz), torch.tile(self.anchor[None], (b, 1, 1))], dim=-1)
        if self.random_samples > 0:
            anchor = torch.cat([anchor, torch.tile(self.random_anchors[None], (b, 1, 1))], dim=1)
        instance_feature = torch.tile(self.instance_feature[None], (b, 1, 1))
        return {
            'rep_features': instance_feature,
            'representation': anchor,
            'anchor_init': anchor[0].clone(),
            'pixel_logits': logits,
            'pixel_gt': pixel_gt,
        }
