#!/usr/bin/env python
"""One encoder block's deformable aggregation for TRAINING, forward + backward: deformable_fused (gf_daf_fused_forward_masked +
gf_daf_fused_backward) against the three-step path (logit add, deformable_prepare -> DAF.apply -> sum over the key points, torch
autograd), at 25 600 and 144 000 anchors, with the projected geometry of tools/bench_ops.fused_case (six cameras, nine key points
per anchor), split logits, and without / with a 0.15 attention-dropout keep-mask.  Device time per block (CUDA events) and the
peak memory allocated beyond the inputs.  Prints one JSON line per (path, anchors, mask).  Needs an MI355X."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_frame  # noqa: E402
from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF  # noqa: E402
from gaussianformer_amd.deformable_prepare import deformable_fused, deformable_prepare  # noqa: E402
from gaussianformer_amd.synthetic import make_daf_inputs  # noqa: E402

dev = torch.device("cuda:0")


def inputs(A):
    g = torch.Generator(device="cpu").manual_seed(1)
    lo = torch.tensor(bench_frame.PC_RANGE[:3]); hi = torch.tensor(bench_frame.PC_RANGE[3:])
    centre = lo + (hi - lo) * torch.rand(1, A, 3, generator=g)
    offs = torch.tensor(bench_frame.FIX_SCALE + [[0.3, 0.3, 0.0], [-0.3, 0.3, 0.0]]) * 0.35
    kp = (centre[:, :, None] + offs[None, None]).to(dev)
    pm, wh = bench_frame.cameras(dev)
    ra = torch.randn(1, A, 4, 9, 4, generator=g).to(dev)
    rc = torch.randn(1, 6, 4, 9, 4, generator=g).to(dev)
    keep = (torch.rand(1, A, 6, 4, 9, 4, generator=g) > 0.15).to(dev)
    gout = torch.randn(1, A, 128, generator=g).to(dev)
    d = make_daf_inputs(num_pts=9, seed=0)
    feat, ss, st = (torch.from_numpy(d[k]).to(dev) for k in ("mc_ms_feat", "spatial_shape", "scale_start_index"))
    return kp, pm, wh, ra, rc, keep, gout, feat, ss, st


def fused(kp, pm, wh, ra, rc, mask, gout, feat, ss, st):
    out = deformable_fused(kp, pm, wh, feat, ss, st, raw_anchor=ra, raw_cam=rc, weight_mask=mask)
    out.backward(gout)


def three(kp, pm, wh, ra, rc, mask, gout, feat, ss, st):
    A = kp.shape[1]
    raw = (ra[:, :, None] + rc[:, None]).reshape(1, A, 6, 4, 9, 4)
    loc, w = deformable_prepare(kp, pm, wh, raw, mask)
    DAF.apply(feat, ss, st, loc, w).reshape(1, A, 9, 128).sum(dim=2).backward(gout)


def measure(fn, A, masked, iters=20, warm=3):
    kp, pm, wh, ra, rc, keep, gout, feat, ss, st = inputs(A)
    leaves = [t.requires_grad_(True) for t in (kp, feat, ra, rc)]
    mask = keep if masked else None

    def once():
        for t in leaves:
            t.grad = None
        fn(kp, pm, wh, ra, rc, mask, gout, feat, ss, st)
    for _ in range(warm):
        once()
    torch.cuda.synchronize()
    for t in leaves:
        t.grad = None
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    once()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base - feat.numel() * 4    # less the grad_mc_ms_feat table
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        e0.record()
        once()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    return {"anchors": A, "mask": 0.15 if masked else None, "us_median": times[len(times) // 2], "us_min": times[0],
            "peak_MB_beyond_inputs_less_grad_feat": peak / 1e6, "weights_tensor_MB": A * 9 * 6 * 4 * 4 * 4 / 1e6}


def main():
    for A in (25600, 144000):
        for masked in (False, True):
            for name, fn in (("fused", fused), ("three_step", three)):
                r = {"op": "daf block forward + backward (training)", "path": name}
                r.update(measure(fn, A, masked))
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
