#!/usr/bin/env python
"""One training step of the hot path, chained through torch autograd (BASELINE.json configs[2] without
the parts that stay torch / mmcv in the reference: image backbone, FFNs, norms, refinement, losses).

    image pyramid -> feature_maps_format
    4 encoder blocks: SparseConv3D (rulebook + gather-GEMM) -> weights_fc (torch GEMM) ->
                      deformable_prepare (projection + masked softmax) -> DAF.apply -> sum over key points
                      (--daf fused: deformable_fused, the same block in one launch each way)
    head:             LocalAggregator.forward_from_rotations (fused Gaussian pre-processing + splat)
                      (--head empty: gf_gaussian_pack appends the whole-grid empty Gaussian first; --head prob: the pack's
                      fused softmax, then LocalAggregatorProb)
    loss = <logits, fixed target>; backward through everything.  ``build`` makes the chain, ``run`` times it (tests/step_ref.py
    restates the same step in float64).

Every native op of the step runs from libgf_hip.so; what torch contributes is the glue named above.
Prints one JSON line: forward and forward+backward milliseconds per step, and that every leaf received a
finite, non-zero gradient.  Needs an MI355X.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF  # noqa: E402
from gaussianformer_amd.deformable_prepare import deformable_fused, deformable_prepare  # noqa: E402
from gaussianformer_amd.gaussian_prepare import GaussianArgs, _GaussianPack  # noqa: E402
from gaussianformer_amd.local_aggregate import LocalAggregator, LocalAggregatorProb  # noqa: E402
from gaussianformer_amd.sparse_conv import SparseConv3D  # noqa: E402
from gaussianformer_amd.synthetic import DAF_LEVELS, voxel_centres  # noqa: E402

PC_RANGE = [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0]      # config/nuscenes_gs25600_solid.py:69
CAMS, LEVELS, GROUPS, KEY_PTS, EMBED = 6, 4, 4, 9, 128


def cameras(dev):
    """Six pinhole cameras 60 degrees apart, 1600x900, nuScenes-like intrinsics (a point is seen by one or two)."""
    pm = torch.eye(4).repeat(1, CAMS, 1, 1)
    K = torch.tensor([[1260.0, 0, 800.0], [0, 1260.0, 450.0], [0, 0, 1.0]])
    for c in range(CAMS):
        yaw = 2 * np.pi * c / CAMS
        R = torch.tensor([[-np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, -1.0], [np.cos(yaw), np.sin(yaw), 0.0]], dtype=torch.float32)
        pm[0, c, :3, :3] = K @ R
        pm[0, c, :3, 3] = K @ torch.tensor([0.0, 1.5, 0.0])
    return pm.to(dev), torch.tensor([[[1600.0, 900.0]] * CAMS], device=dev)


class Block(torch.nn.Module):
    def __init__(self, daf="three_step"):
        super().__init__()
        self.daf = daf
        self.spconv = SparseConv3D(EMBED, EMBED, PC_RANGE, [0.5, 0.5, 0.5], use_out_proj=False, kernel_size=5)
        self.weights_fc = torch.nn.Linear(EMBED, CAMS * LEVELS * KEY_PTS * GROUPS)
        self.key_offsets = torch.nn.Parameter(torch.randn(KEY_PTS, 3) * 0.5)

    def forward(self, feat, anchor, means, scales, table, ss, st, pm, wh):
        bs, A, _ = feat.shape
        feat = feat + self.spconv(feat, anchor)
        key_points = means.unsqueeze(2) + self.key_offsets * scales.unsqueeze(2)
        raw = self.weights_fc(feat).reshape(bs, A, CAMS, LEVELS, KEY_PTS, GROUPS)
        if self.daf == "fused":
            return feat + deformable_fused(key_points, pm, wh, table, ss, st, raw_weights=raw)
        points_2d, weights = deformable_prepare(key_points, pm, wh, raw)
        sampled = DAF.apply(table, ss, st, points_2d, weights)          # [bs, A * KEY_PTS, EMBED]
        return feat + sampled.view(bs, A, KEY_PTS, EMBED).sum(2)


HEADS = ("plain", "empty", "prob")
# nuScenes' whole-grid "empty" Gaussian (config/nuscenes_gs25600_solid.py): centred on the grid, scale (100, 100, 8) -> radius 600
EMPTY_ARGS = dict(mean=[0.0, 0.0, -1.0], scale=[100.0, 100.0, 8.0])


def build(anchors=25600, daf="three_step", head="plain", device=None, seed=0):
    """Builds the chained step: returns a namespace with ``leaves`` (the list whose gradients the step produces), ``named`` (the same
    tensors by name), ``forward()`` -> ``(loss, head outputs)`` and ``const`` (cameras, grid, targets: what a restatement of the step
    needs besides the leaves).  ``head``: ``"plain"`` -- LocalAggregator.forward_from_rotations on softplus semantics, loss
    <logits, target> / n; ``"empty"`` -- GaussianArgs' one-launch pack (gf_gaussian_pack) with nuScenes' whole-grid empty Gaussian
    (one more leaf: ``empty_scalar``) in front of the same aggregator; ``"prob"`` -- the pack's fused softmax in front of
    LocalAggregatorProb.forward_from_rotations, loss <logits, t1> / n + <bin_logits, t2> / n + <density, t3> / n.  With the
    defaults the leaves are those the benchmark has always timed: same seed, same draw order."""
    if daf not in ("three_step", "fused"):
        raise ValueError(f"daf must be 'three_step' or 'fused', not {daf!r}")
    if head not in HEADS:
        raise ValueError(f"head must be one of {HEADS}, not {head!r}")
    dev = torch.device("cuda:0") if device is None else torch.device(device)
    torch.manual_seed(seed)
    A = anchors
    H, W, D, cell = 200, 200, 16, 0.5      # grid_size 0.5 m (config :154): voxel centres are exact in fp32
    pc_min = PC_RANGE[:3]

    blocks = torch.nn.ModuleList([Block(daf) for _ in range(4)]).to(dev)
    for b in blocks:
        torch.nn.init.normal_(b.spconv.layer.weight, std=0.01)
    anchor = torch.randn(1, A, 11, device=dev).requires_grad_(True)
    sem_raw = torch.randn(1, A, 18 if head == "plain" else 17, device=dev).requires_grad_(True)
    feat0 = torch.randn(1, A, EMBED, device=dev).requires_grad_(True)
    maps = [torch.randn(1, CAMS, EMBED, h, w, device=dev).requires_grad_(True) for h, w in DAF_LEVELS]
    pm, wh = cameras(dev)
    pts = torch.from_numpy(voxel_centres(H, W, D, cell, np.asarray(pc_min, dtype=np.float32))).to(dev)[None]
    targets = [torch.randn(H * W * D, 18, device=dev)]
    if head == "prob":
        targets += [torch.randn(H * W * D, device=dev), torch.randn(H * W * D, device=dev)]
    lo = torch.tensor(PC_RANGE[:3], device=dev)
    span = torch.tensor(PC_RANGE[3:], device=dev) - lo
    args = None
    if head == "plain":
        agg = LocalAggregator(3, H, W, D, pc_min, cell, check_inputs=False).to(dev)   # asynchronous path: no host read per call
    else:
        args = GaussianArgs(num_classes=18, with_empty=head == "empty", empty_label=17, empty_args=EMPTY_ARGS,
                            use_localaggprob=head == "prob").to(dev)
        cls = LocalAggregator if head == "empty" else LocalAggregatorProb
        agg = cls(3, H, W, D, pc_min, cell, check_inputs=False).to(dev)
        empty_host = [EMPTY_ARGS["mean"], EMPTY_ARGS["scale"], [1.0, 0.0, 0.0, 0.0]] if head == "empty" else None

    def forward():
        means = anchor[..., :3].clamp(-9.21, 9.21).sigmoid() * span + lo
        scales = anchor[..., 3:6].sigmoid() * (0.64 - 0.08) + 0.08
        rots = torch.nn.functional.normalize(anchor[..., 6:10], dim=-1)
        opa = anchor[..., 10:11].sigmoid()
        table, ss, st = DAF.feature_maps_format(maps)
        feat = feat0
        for b in blocks:
            feat = b(feat, anchor, means, scales, table, ss, st, pm, wh)
        # the refinement layer of the reference would turn feat into anchor updates; here feat gates the opacity
        opa = opa * feat.mean(-1, keepdim=True).sigmoid()
        if head == "plain":
            sem = torch.nn.functional.softplus(sem_raw)
        else:
            # GaussianArgs' op sequence in one launch (gf_gaussian_pack, gaussian_head.py:88-109): the zero column and the
            # appended empty Gaussian, or the softmax and the zero column
            sem = torch.nn.functional.softplus(sem_raw) if head == "empty" else sem_raw
            means, scales, rots, sem, opa = _GaussianPack.apply(
                means, scales, rots, sem, opa, args.empty_scalar if head == "empty" else None, empty_host, 18, False,
                head == "empty", head == "prob", 17)
        out = agg.forward_from_rotations(pts, means, opa, sem, scales, rots)
        outs = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        loss = (outs[0].reshape(-1, 18) * targets[0]).mean()
        for o, t in zip(outs[1:], targets[1:]):
            loss = loss + (o.reshape(-1) * t).mean()
        return loss, outs

    leaves = [anchor, sem_raw, feat0] + maps + list(blocks.parameters())
    named = dict(anchor=anchor, sem_raw=sem_raw, feat0=feat0, maps=maps,
                 blocks=[dict(spconv=b.spconv.layer.weight, fc_weight=b.weights_fc.weight, fc_bias=b.weights_fc.bias,
                              key_offsets=b.key_offsets) for b in blocks])
    if head == "empty":
        leaves.append(args.empty_scalar)
        named["empty_scalar"] = args.empty_scalar
    const = dict(head=head, daf=daf, pm=pm, wh=wh, pts=pts, targets=targets, grid=(H, W, D), cell=cell, pc_range=list(PC_RANGE),
                 levels=[tuple(x) for x in DAF_LEVELS], scale_multiplier=3, kernel_size=5, groups=GROUPS, key_pts=KEY_PTS,
                 empty_args=EMPTY_ARGS if head == "empty" else None)
    return argparse.Namespace(leaves=leaves, named=named, forward=forward, const=const, blocks=blocks, agg=agg)


def run(anchors=25600, steps=10, warmup=3, daf="three_step", head="plain"):
    """Runs the chained step and returns the result record (raises if a leaf got no usable gradient).  ``daf="fused"`` runs
    each block's deformable aggregation as deformable_fused instead of deformable_prepare -> DAF.apply -> sum; ``head`` as in
    :func:`build`."""
    if daf not in ("three_step", "fused"):
        raise ValueError(f"daf must be 'three_step' or 'fused', not {daf!r}")
    args = argparse.Namespace(anchors=anchors, steps=steps, warmup=warmup)
    if not torch.cuda.is_available():
        raise RuntimeError("bench_step.py needs an MI355X")
    A = args.anchors
    s = build(A, daf, head)
    leaves, forward = s.leaves, s.forward

    def step(backward=True):
        for t in leaves:
            t.grad = None
        loss = forward()[0]
        if backward:
            loss.backward()
        return loss

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(backward=False)
    torch.cuda.synchronize()
    fwd = (time.perf_counter() - t0) / args.steps
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    full = (time.perf_counter() - t0) / args.steps

    bad = [i for i, t in enumerate(leaves) if t.grad is None or not torch.isfinite(t.grad).all() or float(t.grad.abs().max()) == 0.0]
    out = {"op": "hot-path training step (4 x [sparse conv + DAF prepare + DAF] + fused prepare + splat, fwd + bwd)",
           "anchors": A, "sample_points": A * KEY_PTS, "forward_ms": fwd * 1e3, "forward_backward_ms": full * 1e3,
           "loss": float(loss.detach()), "leaves": len(leaves), "leaves_without_finite_nonzero_grad": bad}
    if daf != "three_step":
        out["daf"] = daf
    if head != "plain":
        out["head"] = head
    if bad:
        raise RuntimeError(f"gradient check failed for leaves {bad}: {out}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, default=25600)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--daf", choices=("three_step", "fused"), default="three_step")
    ap.add_argument("--head", choices=HEADS, default="plain")
    args = ap.parse_args()
    print(json.dumps(run(args.anchors, args.steps, args.warmup, args.daf, args.head)))


if __name__ == "__main__":
    main()
