"""The head: ``GaussianHead`` (drop-in for model/head/gaussian_head.py:10-197), its geosem step and its epilogue.

* ``occupancy_labels``: host mirror of the last lines of ``GaussianHead.forward`` (:164-185), backed by
  ``gf_head_labels``;
* ``geosem`` / ``geosem_labels``: the prob head's ``combine_geosem`` step (:166-168) in one launch each way
  (``gf_head_geosem_forward`` / ``gf_head_geosem_backward``), the second with the labels from the same launch;
* ``GaussianHead``: the module -- the reference's constructor keys, state dict, attributes and output dict, built from this
  package's ``GaussianArgs``, ``LocalAggregator*`` and the two ops above;
* the Gaussian-sharded inference path whose 8-GPU exchange is a reduce-scatter of the logits and an all-gather of 8-byte
  labels instead of a full all-reduce.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .gaussian_prepare import GaussianArgs, covariance_inverse
from .local_aggregate import LocalAggregator, LocalAggregatorProb, LocalAggregatorProbFast
from .sharded import shard_bounds


def occupancy_labels(logits, bin_logits=None, threshold=0.5, empty_label=17, combine_geosem=False):
    """``final_prediction`` of the head for one frame: ``logits [N,18]`` (the aggregator's
    output, before the reference's ``[None].transpose(1, 2)``), ``bin_logits [N]`` for the prob
    head.  Returns int64 ``[N]``."""
    _lib.require_gpu(logits, bin_logits)
    lg, bl = _lib.as_arg(logits), _lib.as_arg(bin_logits)
    N, C = lg.shape
    mode = _lib.GF_LABELS_ARGMAX if bl is None else (
        _lib.GF_LABELS_PROB_GEOSEM if combine_geosem else _lib.GF_LABELS_PROB_THRESHOLD)
    labels = torch.empty(N, dtype=torch.int64, device=lg.device)
    _lib.call("gf_head_labels", lg.device, N, C, mode, lg, bl, float(threshold), int(empty_label), labels)
    return labels


def _geosem_args(logits, bin_logits):
    _lib.require_gpu(logits, bin_logits)
    lg, bl = _lib.as_arg(logits), _lib.as_arg(bin_logits)
    if lg.dim() != 2 or bl.shape != lg.shape[:1]:
        raise ValueError(f"geosem takes logits [N,18] and bin_logits [N], got {tuple(lg.shape)} and {tuple(bl.shape)}")
    return lg, bl


class _Geosem(torch.autograd.Function):
    """gaussian_head.py:166-168 and its gradient, one launch each.  Saves its two inputs only -- the very tensors the prob
    splat's own ``Function`` holds for its backward, so nothing is kept alive on its account."""

    @staticmethod
    def forward(ctx, logits, bin_logits):
        lg, bl = _geosem_args(logits, bin_logits)
        out = torch.empty_like(lg)
        _lib.call("gf_head_geosem_forward", lg.device, lg.shape[0], lg.shape[1], lg, bl, out, None)
        ctx.save_for_backward(lg, bl)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lg, bl = ctx.saved_tensors
        _lib.require_gpu(grad_out)
        g = _lib.as_arg(grad_out)
        grad_logits, grad_bin = torch.empty_like(lg), torch.empty_like(bl)
        _lib.call("gf_head_geosem_backward", lg.device, lg.shape[0], lg.shape[1], lg, bl, g, grad_logits, grad_bin)
        return grad_logits, grad_bin


def geosem(logits, bin_logits):
    """``cat([logits[:, :-1] * bin_logits[:, None], 1 - bin_logits[:, None]], -1)`` (gaussian_head.py:166-168) for the prob
    aggregator's ``logits [N,18]`` and ``bin_logits [N]``: ``[N,18]``, the torch expression's bits, differentiable."""
    return _Geosem.apply(logits, bin_logits)


def geosem_labels(logits, bin_logits):
    """``(geosem [N,18], labels int64 [N])`` from one launch: the geosem rows and the head's ``final_occ`` of them
    (``occupancy_labels(..., combine_geosem=True)``, the same labels).  Records no gradient."""
    lg, bl = _geosem_args(logits, bin_logits)
    out = torch.empty_like(lg)
    labels = torch.empty(lg.shape[0], dtype=torch.int64, device=lg.device)
    _lib.call("gf_head_geosem_forward", lg.device, lg.shape[0], lg.shape[1], lg, bl, out, labels)
    return out, labels


def _covariance_inverse_torch(scales, rotations):
    """Sigma^-1 in closed form, ``R^T diag(1 / s^2) R`` with ``R`` the rotation of the normalised (w,x,y,z) quaternion --
    what gaussian_head.py:111-119 inverts numerically -- in torch ops, for the tensors ``covariance_inverse`` has no kernel
    for (CPU tensors): ``[..., 3, 3]``."""
    w, x, y, z = torch.nn.functional.normalize(rotations, dim=-1).unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(*w.shape, 3, 3)
    return R.transpose(-1, -2) @ (R / (scales * scales).unsqueeze(-1))


class GaussianHead(GaussianArgs):
    """Drop-in for the reference's ``GaussianHead`` (model/head/gaussian_head.py:10-197), built without mmengine: the same
    constructor keys and defaults, the same ``state_dict`` (``zero_tensor``, ``aggregator.pc_min`` and, ``with_empty``,
    ``empty_scalar`` and the five ``empty_*`` buffers, on the head itself), the same attributes (``with_emtpy`` (sic) ...), the
    same supervised layers -- ``'random_k'`` makes the reference's own draw from numpy's global generator -- and the same
    output dict.  ``self.aggregator`` is this package's ``LocalAggregator`` / ``LocalAggregatorProb`` /
    ``LocalAggregatorProbFast`` built from ``**cuda_kwargs`` (their extra keywords pass through).

    ``native`` (class attribute; no constructor key, not in the state dict): on fp32 GPU tensors at batch size 1 a layer runs
    as one pack launch (``gf_gaussian_pack``), ``forward_from_rotations`` (Sigma^-1, integer centres and radii in one
    launch: no 3x3 tensors), ``geosem`` and ``occupancy_labels`` -- for ``combine_geosem`` where nothing needs a gradient
    the labels come from the geosem launch itself.  Every other call -- ``native = False``, CPU tensors, other batch sizes --
    runs the reference's own op sequence on this package's pieces: ``GaussianArgs._forward_torch``, ``aggregator(...,
    CovInv)``, the three torch ops and ``argmax``.

    One departure: ``pts`` is NOT cloned.  The reference hands the aggregator ``sampled_xyz.clone().float()`` (:158); a fresh
    tensor per layer would defeat the aggregator's ``points_int`` cache (and ``register_grid``), and the aggregator does not
    write it."""
    native = True

    def __init__(self, init_cfg=None, apply_loss_type=None, num_classes=18, empty_args=None, with_empty=False,
                 cuda_kwargs=None, dataset_type='nusc', empty_label=17, use_localaggprob=False,
                 use_localaggprob_fast=False, combine_geosem=False, **kwargs):
        super().__init__(num_classes=num_classes, empty_args=empty_args, with_empty=with_empty, dataset_type=dataset_type,
                         empty_label=empty_label, use_localaggprob=use_localaggprob)
        self.init_cfg = init_cfg
        if use_localaggprob:
            self.aggregator = (LocalAggregatorProbFast if use_localaggprob_fast else LocalAggregatorProb)(**cuda_kwargs)
        else:
            self.aggregator = LocalAggregator(**cuda_kwargs)
        self.combine_geosem = combine_geosem
        self.empty_args = empty_args
        if apply_loss_type == 'all':
            self.apply_loss_type = 'all'
        elif 'random' in apply_loss_type:
            self.apply_loss_type = 'random'
            self.random_apply_loss_layers = int(apply_loss_type.split('_')[1])
        elif 'fixed' in apply_loss_type:
            self.apply_loss_type = 'fixed'
            self.fixed_apply_loss_layers = [int(item) for item in apply_loss_type.split('_')[1:]]
        else:
            raise NotImplementedError
        self.register_buffer('zero_tensor', torch.zeros(1, dtype=torch.float))

    def init_weights(self):
        for m in self.modules():
            if hasattr(m, "init_weight"):
                m.init_weight()

    def _sampling(self, gt_xyz, gt_label, gt_mask=None):
        if gt_mask is None:
            gt_label = gt_label.flatten(1)
            gt_xyz = gt_xyz.flatten(1, 3)
        else:
            assert gt_label.shape[0] == 1, "OccLoss does not support bs > 1"
            gt_label = gt_label[gt_mask].reshape(1, -1)
            gt_xyz = gt_xyz[gt_mask].reshape(1, -1, 3)
        return gt_xyz, gt_label

    @staticmethod
    def _covariance_inverse(scales, rotations):
        return covariance_inverse(scales, rotations) if scales.is_cuda else _covariance_inverse_torch(scales, rotations)

    def prepare_gaussian_args(self, gaussians):
        """The reference's tuple ``(means, origi_opa, opacities, scales, CovInv)`` (:82-120), ``CovInv [b,g,3,3]`` computed on
        the device (``GaussianArgs.forward``) instead of the reference's LAPACK inverse on the host."""
        fields = (gaussians.means, gaussians.scales, gaussians.rotations, gaussians.semantics, gaussians.opacities)
        return GaussianArgs.forward(self, *fields) if self.native else self._forward_torch(*fields)

    def _apply_loss_layers(self, num_decoder):
        """The supervised layers (:128-142)."""
        if not self.training:
            return [num_decoder - 1]
        if self.apply_loss_type == "all":
            return list(range(num_decoder))
        if self.apply_loss_type == "random":
            if self.random_apply_loss_layers > 1:
                layers = np.random.choice(num_decoder - 1, self.random_apply_loss_layers - 1, False)
                return layers.tolist() + [num_decoder - 1]
            return [num_decoder - 1]
        if self.apply_loss_type == 'fixed':
            return self.fixed_apply_loss_layers
        raise NotImplementedError

    def _runs_native(self, gaussians, pts):
        tensors = (pts, gaussians.means, gaussians.scales, gaussians.rotations, gaussians.semantics)
        return self.native and gaussians.means.shape[0] == 1 and all(t.is_cuda and t.dtype == torch.float32 for t in tensors)

    def forward(self, representation, metas=None, **kwargs):
        apply_loss_layers = self._apply_loss_layers(len(representation))
        prediction, bin_logits, density = [], [], []
        device = self.zero_tensor.device
        occ_xyz = metas['occ_xyz'].to(device)
        occ_label = metas['occ_label'].to(device)
        occ_cam_mask = metas['occ_cam_mask'].to(device)
        sampled_xyz, sampled_label = self._sampling(occ_xyz, occ_label, None)
        pts = sampled_xyz.float()   # (not cloned: see the class docstring)
        threshold = kwargs.get("sigmoid_thresh", 0.5)
        final_prediction = None
        for i, idx in enumerate(apply_loss_layers):
            gaussians = representation[idx]['gaussian']
            native = self._runs_native(gaussians, pts)
            fields = (gaussians.means, gaussians.scales, gaussians.rotations, gaussians.semantics, gaussians.opacities)
            if native:
                means, scales, rotations, opacities, origi_opa = (self._pack if self._packs(fields[0]) else self._fields_torch)(*fields)
                bs, g = means.shape[:2]
                semantics = self.aggregator.forward_from_rotations(pts, means, origi_opa.reshape(bs, g), opacities, scales, rotations)
            else:
                means, origi_opa, opacities, scales, CovInv = self._forward_torch(*fields)
                bs, g = means.shape[:2]
                semantics = self.aggregator(pts, means, origi_opa.reshape(bs, g), opacities, scales, CovInv)
            last = i == len(apply_loss_layers) - 1
            if self.use_localaggprob:
                logits, bins, dens = semantics
                if not self.combine_geosem:
                    geo = logits
                elif not native:
                    sem = logits[:, :-1] * bins.unsqueeze(-1)
                    geo = torch.cat([sem, 1 - bins.unsqueeze(-1)], dim=-1)
                elif last and not _lib.needs_grad((logits, bins)):
                    geo, labels = geosem_labels(logits, bins)
                    final_prediction = labels[None]
                else:
                    geo = geosem(logits, bins)
                prediction.append(geo[None].transpose(1, 2))
                bin_logits.append(bins[None])
                density.append(dens[None])
            else:
                logits, bins = semantics, None
                prediction.append(logits[None].transpose(1, 2))
            if last and native and final_prediction is None:
                final_prediction = occupancy_labels(logits, bins, threshold=threshold, empty_label=self.empty_label,
                                                    combine_geosem=self.combine_geosem)[None]
        if final_prediction is None:   # :178-185
            if self.use_localaggprob and not self.combine_geosem:
                final_semantics = prediction[-1].argmax(dim=1)
                final_occupancy = bin_logits[-1] > threshold
                final_prediction = torch.ones_like(final_semantics) * self.empty_label
                final_prediction[final_occupancy] = final_semantics[final_occupancy]
            else:
                final_prediction = prediction[-1].argmax(dim=1)
        return {
            'pred_occ': prediction,
            'bin_logits': bin_logits,
            'density': density,
            'sampled_label': sampled_label,
            'sampled_xyz': sampled_xyz,
            'occ_mask': occ_cam_mask,
            'final_occ': final_prediction,
            'gaussian': representation[-1]['gaussian'],
            'gaussians': [r['gaussian'] for r in representation],
        }


def sharded_splat_labels(local_splat, pts, means3D, opacities, semantics, scales, cov3D, labels_fn=occupancy_labels,
                         group=None):
    """Gaussian-sharded inference that ends in labels: every rank splats its slice of the
    Gaussians into a full partial grid (as ``sharded_splat_forward``), the partial grids are
    REDUCE-SCATTERED (each rank receives the summed logits of 1/world of the points), labelled
    locally with ``labels_fn`` and the int64 labels all-gathered: half the xGMI traffic of the
    all-reduce, and the label exchange is 5 MB instead of 46 MB.  Returns labels ``[N]``."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    P = means3D.shape[1]
    lo, hi = shard_bounds(P, rank, world)
    logits = local_splat(pts, means3D[:, lo:hi], opacities[:, lo:hi], semantics[:, lo:hi], scales[:, lo:hi],
                         cov3D[:, lo:hi]).contiguous()
    if world == 1:
        return labels_fn(logits)
    N, C = logits.shape
    per = (N + world - 1) // world          # points per rank, the last slice is padded
    if per * world != N:
        logits = torch.cat([logits, logits.new_zeros(per * world - N, C)])
    mine = torch.empty(per, C, dtype=logits.dtype, device=logits.device)
    if dist.get_backend(group) == "gloo":   # gloo has no reduce_scatter: same result through an all-reduce
        dist.all_reduce(logits, op=dist.ReduceOp.SUM, group=group)
        mine.copy_(logits[rank * per:(rank + 1) * per])
    else:
        dist.reduce_scatter_tensor(mine, logits, op=dist.ReduceOp.SUM, group=group)
    labels_mine = labels_fn(mine)
    labels = torch.empty(per * world, dtype=labels_mine.dtype, device=labels_mine.device)
    dist.all_gather_into_tensor(labels, labels_mine.contiguous(), group=group)
    return labels[:N]
