#!/usr/bin/env python
"""GaussianLifterV2's pixel work and PixelDistributionLoss at the prob configs' full shape (b = 1, 6 cameras x 108 x 200
pixels, S = 128 depth bins, a = 1, stochastic sampling; ~20 % of the pixels disabled), native against a torch restatement of
the reference's lines (model/lifter/gaussian_lifter_v2.py:169-233, model/utils/sampler.py, loss/bce_loss.py:60-87):

  candidates        the per-batch candidate points (native: gaussianformer_amd.lifter.lift_pixels without pixel_gt)
  candidates_gt     the candidates and pixel_gt (the training path)
  loss              the pixel loss forward + backward (softmax, as the configs)

Both sides take the same logits and uniforms and include their host synchronisations (the native path reads the counts
back once; the torch path's boolean indexing syncs per batch element).  Device time per call: HIP events around each call
after warm-up; median and spread over the timed calls; peak device memory above the inputs.  Writes one JSON line per
(workload, path) to profiles/bench_lifter.jsonl and prints it.  Needs an MI355X.

    python tools/bench_lifter.py [--steps K] [--warmup W] [--out profiles/bench_lifter.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianformer_amd.lifter import lift_pixels, pixel_distribution_loss  # noqa: E402

PC = [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0]
RES = (200, 200, 16)
VS = 0.5
EMPTY = 17


def lidar2img(n_cam, W_img, H_img):
    f = 0.79 * W_img
    K = np.array([[f, 0, W_img / 2, 0], [0, f, H_img / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    mats = []
    for yaw in np.deg2rad(np.linspace(0.0, 360.0, n_cam, endpoint=False)):
        c2l = np.eye(4)
        c2l[:3, 0] = [np.sin(yaw), -np.cos(yaw), 0.0]
        c2l[:3, 1] = [0.0, 0.0, -1.0]
        c2l[:3, 2] = [np.cos(yaw), np.sin(yaw), 0.0]
        c2l[:3, 3] = [0.0, 0.0, 1.5]
        mats.append(K @ np.linalg.inv(c2l))
    return np.stack(mats).astype(np.float32)


def torch_lift(logits, proj, wh, depth, u, occ_label=None, cam_mask=None):
    """The reference's pixel work restated with torch ops: all S points per pixel, softmax, searchsorted, argmax, gather,
    per-element boolean indexing; pixel_gt from two advanced-index gathers when occ_label is given."""
    b, n, h, w, nb = logits.shape
    S = nb - 1
    img2lidar = proj.inverse()
    cols = (torch.arange(w, dtype=torch.float32, device=logits.device) + 0.5) / w
    rows = (torch.arange(h, dtype=torch.float32, device=logits.device) + 0.5) / h
    uv = torch.stack([cols[None, :].expand(h, w), rows[:, None].expand(h, w)], -1)
    uv = uv[None, None].expand(b, n, h, w, 2) * wh[:, :, None, None]
    uvd = uv.unsqueeze(4).expand(b, n, h, w, S, 2)
    hom = torch.cat([uvd, torch.ones_like(uvd)], -1)
    hom[..., :3] = hom[..., :3] * depth.view(1, 1, 1, 1, -1, 1)
    pts = (img2lidar[:, :, None, None, None] @ hom[..., None]).squeeze(-1)[..., :3]
    lo = torch.tensor(PC[:3], device=logits.device)
    hi = torch.tensor(PC[3:], device=logits.device)
    gt = None
    if occ_label is not None:
        out = ((pts < lo) | (pts >= hi)).any(-1)
        idx = ((pts - lo) / VS).to(torch.int)
        for ax in range(3):
            idx[..., ax].clamp_(0, RES[ax] - 1)
        occ = torch.stack([o[i[..., 0], i[..., 1], i[..., 2]] for o, i in zip(occ_label, idx)])
        occ[out] = EMPTY
        valid = torch.stack([m[i[..., 0], i[..., 1], i[..., 2]] for m, i in zip(cam_mask, idx)])
        valid[out] = False
        gt = (occ != EMPTY) & valid
        gt = torch.cat([gt, ~gt.any(-1, keepdim=True)], -1)
    pdf = torch.softmax(logits, -1)
    norm = pdf / (torch.finfo(torch.float32).eps + pdf.sum(-1, keepdim=True))
    index = torch.searchsorted(norm.cumsum(-1), u, right=True).clip(max=S)
    disabled = (pdf.argmax(-1, keepdim=True) == S).expand_as(index)
    k = index.clamp(max=S - 1)[..., None].expand(b, n, h, w, index.shape[-1], 3)
    chosen = pts.gather(4, k)
    scans = []
    for i in range(b):
        c = chosen[i][~disabled[i]]
        scans.append(c[((c >= lo) & (c < hi)).all(-1)])
    return scans, gt


def torch_loss(logits, gt):
    x = logits.detach().requires_grad_(True)
    loss = F.binary_cross_entropy(torch.softmax(x, -1), gt.float())
    loss.backward()
    return loss


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    peak = torch.cuda.max_memory_allocated() - base
    return ms, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_lifter.jsonl"))
    ap.add_argument("--native-only", action="store_true", help="skip the torch paths (for a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    b, n, h, w, S = 1, 6, 108, 200, 128
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(b, n, h, w, S + 1, generator=g) * 2.0
    logits[..., S] += 1.5
    logits = logits.to(dev)
    u = torch.rand(b, n, h, w, 1, generator=g).to(dev)
    proj = torch.from_numpy(lidar2img(n, 1600, 864))[None].to(dev)
    wh = torch.tensor([[[1600.0, 864.0]] * n], device=dev)
    depth = torch.linspace(1.0, 72.0, S, device=dev)
    occ_label = torch.full((b,) + RES, EMPTY, dtype=torch.int64)
    occ_label[:, :, :, :2] = 11
    occ_label[:, 60:140, 60:140, 2:6] = 3
    occ_label = occ_label.to(dev)
    cam_mask = torch.ones((b,) + RES, dtype=torch.bool, device=dev)
    kw = dict(depth_bins=depth, pc_range=PC, voxel_size=VS, occ_resolution=RES, anchors_per_pixel=1, uniforms=u)

    _, gt = lift_pixels(logits, proj, wh, occ_label=occ_label, occ_cam_mask=cam_mask, empty_label=EMPTY, **kw)
    work = {
        "candidates": {"native": lambda: lift_pixels(logits, proj, wh, **kw),
                       "torch": lambda: torch_lift(logits, proj, wh, depth, u)},
        "candidates_gt": {"native": lambda: lift_pixels(logits, proj, wh, occ_label=occ_label, occ_cam_mask=cam_mask,
                                                        empty_label=EMPTY, **kw),
                          "torch": lambda: torch_lift(logits, proj, wh, depth, u, occ_label, cam_mask)},
        "loss": {"native": lambda: pixel_distribution_loss(logits.detach().requires_grad_(True), gt, use_sigmoid=False).backward(),
                 "torch": lambda: torch_loss(logits, gt)},
    }
    # the two sides agree on what they compute
    (ns,), _ = lift_pixels(logits, proj, wh, **kw)
    (ts,), tgt = torch_lift(logits, proj, wh, depth, u, occ_label, cam_mask)
    agree = dict(candidates_native=int(ns.shape[0]), candidates_torch=int(ts.shape[0]),
                 pixel_gt_mismatch=int((tgt != gt).sum()))
    print(json.dumps(agree))
    lines = []
    for name, paths in work.items():
        for path, fn in paths.items():
            if args.native_only and path != "native":
                continue
            ms, peak = timed(fn, args.steps, args.warmup)
            rec = dict(workload=name, path=path, shape=[b, n, h, w, S + 1], a=1, stochastic=True,
                       median_us=round(1000 * statistics.median(ms), 1), min_us=round(1000 * min(ms), 1),
                       max_us=round(1000 * max(ms), 1), steps=args.steps, warmup=args.warmup,
                       peak_mib=round(peak / 2 ** 20, 1), **agree)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if not args.native_only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
