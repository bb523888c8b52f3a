#!/usr/bin/env python
"""The head's geosem step and the ``GaussianHead`` module at the nuScenes grid (200 x 200 x 16, N = 640 000), on one MI355X.

  (a) ``gaussianformer_amd.head.geosem`` (one launch each way) against the three-op torch composition of
      model/head/gaussian_head.py:166-168 on the same tensors: forward, and forward + backward (gradients to both inputs);
  (b) ``GaussianHead`` in train mode, forward + backward of a fixed linear loss, ``native = True`` against ``native = False``
      (the reference's op sequence on this package's pieces): the prob head with ``combine_geosem`` at P = 25 600, and the base
      head with the appended empty Gaussian at P = 25 600.  Gaussians as tools/bench_step.py draws them (uniform centres,
      scales U(0.08, 0.64)); ``check_inputs=False``, so neither side reads the device.

The two sides ALTERNATE in one process: ``--repeats`` rounds, in each round one median over ``--steps`` timed calls per side (HIP
events, ``--inner`` back-to-back runs per call).  Reported per side: the median of the rounds' medians and their spread (max -
min); the difference of the two with the larger spread; peak device memory above the inputs; for (a) the algorithmic bytes
(forward: read 18 + 1 floats per row, write 18; backward: read 18 + 18 + 1, write 18 + 1) and the share of 8 TB/s they reach.
One JSON line per row, also written to profiles/bench_head.jsonl.  Needs an MI355X.

    python tools/bench_head.py [--repeats R] [--steps K] [--warmup W] [--inner N] [--out profiles/bench_head.jsonl]
"""
import argparse
import collections
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianformer_amd.head import GaussianHead, geosem  # noqa: E402
from gaussianformer_amd.synthetic import GRID, voxel_centres  # noqa: E402

PEAK_BYTES_PER_US = 8e6   # 8 TB/s
EMPTY_ARGS = dict(mean=[0, 0, -1.0], scale=[100, 100, 8.0])
# the fields the head reads from a decoder layer's prediction (model/encoder/gaussian_encoder/utils.py)
GaussianPrediction = collections.namedtuple("GaussianPrediction", "means scales rotations opacities semantics")


def median_us(fn, steps, inner):
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(ts)


def alternate(sides, args):
    """``{side: (median of the rounds' medians, spread)}`` with the sides taking turns in every round."""
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    meds = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            meds[k].append(median_us(fn, args.steps, args.inner))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in meds.items()}


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def composition(logits, bins):
    sem = logits[:, :-1] * bins.unsqueeze(-1)
    geo = 1 - bins.unsqueeze(-1)
    return torch.cat([sem, geo], dim=-1)


def row(bench, what, res, sides, first, second, **extra):
    (m1, s1), (m2, s2) = res[first], res[second]
    r = dict(bench=bench, what=what, **{f"{first}_us": round(m1, 2), f"{first}_spread_us": round(s1, 2),
                                        f"{second}_us": round(m2, 2), f"{second}_spread_us": round(s2, 2)},
             difference_us=round(m2 - m1, 2), difference_spread_us=round(max(s1, s2), 2),
             **{f"{k}_peak_mib": round(peak_mib(fn), 1) for k, fn in sides.items()}, **extra)
    print(json.dumps(r), flush=True)
    return r


def bench_geosem(dev, args):
    N = GRID["H"] * GRID["W"] * GRID["D"]
    gen = torch.Generator().manual_seed(0)
    logits, bins, grad = (t.to(dev) for t in (torch.randn(N, 18, generator=gen), torch.rand(N, generator=gen), torch.randn(N, 18, generator=gen)))
    ll, bl = logits.clone().requires_grad_(True), bins.clone().requires_grad_(True)
    rows = []
    for what, nbytes, make in (
            ("forward", 4 * N * (18 + 1 + 18), lambda op: lambda: op(logits, bins)),
            ("forward_backward", 4 * N * (18 + 1 + 18) + 4 * N * (18 + 18 + 1 + 18 + 1), lambda op: lambda: torch.autograd.grad(op(ll, bl), (ll, bl), grad))):
        sides = dict(geosem=make(geosem), torch_composition=make(composition))
        res = alternate(sides, args)
        rows.append(row("head_geosem", what, res, sides, "geosem", "torch_composition", N=N, algorithmic_bytes=nbytes,
                        geosem_frac_of_8TBps=round(nbytes / res["geosem"][0] / PEAK_BYTES_PER_US, 4),
                        geosem_faster_beyond_spread=bool(res["torch_composition"][0] - res["geosem"][0] > max(res["geosem"][1], res["torch_composition"][1]))))
    return rows


def bench_module(dev, args, name, P):
    H, W, D = GRID["H"], GRID["W"], GRID["D"]
    cuda_kwargs = dict(H=H, W=W, D=D, pc_min=list(GRID["pc_min"]), grid_size=GRID["grid_size"], check_inputs=False)
    if name == "prob_geosem":
        head = GaussianHead(apply_loss_type="random_1", use_localaggprob=True, combine_geosem=True, cuda_kwargs=dict(scale_multiplier=4, **cuda_kwargs))
    else:
        head = GaussianHead(apply_loss_type="random_1", with_empty=True, empty_args=EMPTY_ARGS, cuda_kwargs=dict(scale_multiplier=3, **cuda_kwargs))
    head = head.to(dev).train()
    gen = torch.Generator().manual_seed(1)
    lo = torch.tensor(GRID["pc_min"])
    ext = torch.tensor([H, W, D]) * GRID["grid_size"]
    leaf = lambda t: t.to(dev).requires_grad_(True)
    means = leaf(lo + (0.001 + 0.998 * torch.rand(1, P, 3, generator=gen)) * ext)
    scales = leaf(0.08 + 0.56 * torch.rand(1, P, 3, generator=gen))
    rots = leaf(torch.nn.functional.normalize(torch.randn(1, P, 4, generator=gen), dim=-1))
    opa = leaf(torch.rand(1, P, 1, generator=gen))
    sem = leaf(torch.nn.functional.softplus(torch.randn(1, P, 17, generator=gen)))
    leaves = [means, scales, rots, opa, sem] + list(head.parameters())
    rep = [dict(gaussian=GaussianPrediction(means, scales, rots, opa, sem))]
    pts = torch.from_numpy(voxel_centres(H, W, D, GRID["grid_size"], np.asarray(GRID["pc_min"], dtype=np.float32))).to(dev)
    metas = dict(occ_xyz=pts.reshape(1, H, W, D, 3), occ_label=torch.zeros(1, H, W, D, dtype=torch.int64, device=dev),
                 occ_cam_mask=torch.ones(1, H, W, D, dtype=torch.bool, device=dev))
    N = H * W * D
    # (the loss's weights in pred_occ's own layout: a transposed view of a contiguous [1,N,18])
    weights = [torch.randn(1, N, 18, generator=gen).to(dev).transpose(1, 2)] + [torch.randn(1, N, generator=gen).to(dev) for _ in range(2)]

    def step(native):
        def run():
            head.native = native
            out = head(rep, metas)
            loss = (out["pred_occ"][-1] * weights[0]).sum()
            for o, w in zip((out["bin_logits"], out["density"]), weights[1:]):
                if o:
                    loss = loss + (o[-1] * w).sum()
            torch.autograd.grad(loss, leaves)
        return run

    sides = dict(native=step(True), reference_sequence=step(False))
    res = alternate(sides, args)
    return [row("head_module", f"{name} forward_backward", res, sides, "native", "reference_sequence", N=N, P=P)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--module-inner", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_head.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = bench_geosem(dev, a)
    a.inner = a.module_inner
    for name in ("prob_geosem", "base_empty"):
        rows += bench_module(dev, a, name, 25600)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
