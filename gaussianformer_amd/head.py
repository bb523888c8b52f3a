"""Head epilogue: occupancy labels straight from the splat outputs.

Host mirror of the last lines of ``GaussianHead.forward`` (model/head/gaussian_head.py:164-185),
backed by ``gf_head_labels``; plus the Gaussian-sharded inference path whose 8-GPU exchange is a
reduce-scatter of the logits and an all-gather of 8-byte labels instead of a full all-reduce.
"""
import torch
import torch.distributed as dist

from . import _lib
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
