#!/usr/bin/env python
"""DCNv2 (modulated deformable convolution, 3 x 3, stride 1, padding 1, no bias) at the backbone's DCN shapes, native
(gaussianformer_amd.deform_conv) against a torch fp32 composition (per-tap bilinear gather, x mask, a column tensor and one
matmul on hipBLASLt: what a ROCm user without mmcv would write), with torch.nn.functional.conv2d (MIOpen) at the same shape
as context:

  layer3   [6, 256, 54, 100] -> 256  (23 blocks per backbone pass)
  layer4   [6, 512, 27, 50]  -> 512  (3 blocks)

Offsets zero, or realistic (N(0, 1.5^2) px, masks uniform in (0, 1)).  Per row: forward and forward + backward (all five
gradients) µs, the median of the timed calls by HIP events; peak device memory above the inputs; achieved TFLOP/s
(M K N 2 forward, three times that forward + backward) and the fraction of the exact-fp32 matrix floor (157.3 TF).  Writes
one JSON line per row, and a per-frame total (23 x layer3 + 3 x layer4), to profiles/bench_dcn.jsonl.  Needs an MI355X.

    python tools/bench_dcn.py [--steps K] [--warmup W] [--native-only] [--out profiles/bench_dcn.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianformer_amd.deform_conv import modulated_deform_conv2d  # noqa: E402

PEAK_TF = 157.3
SHAPES = {"layer3": (6, 256, 54, 100, 256), "layer4": (6, 512, 27, 50, 512)}
BLOCKS = {"layer3": 23, "layer4": 3}


def torch_dcn(x, off, m, w):
    """fp32 torch composition of the op: per tap, a bilinear gather of the four corners (strict window, zero corners),
    times the mask, into a [N, C kk, P] column tensor; then one matmul."""
    N, C, H, W = x.shape
    Co, _, kh, kw = w.shape
    Ho, Wo = off.shape[2:]
    kk = kh * kw
    o = off.view(N, kk, 2, Ho, Wo)
    ho = torch.arange(Ho, device=x.device, dtype=torch.float32)[:, None]
    wo = torch.arange(Wo, device=x.device, dtype=torch.float32)[None, :]
    flat = x.reshape(N, C, H * W)
    cols = []
    for k in range(kk):
        i, j = divmod(k, kw)
        y = (ho - 1 + i) + o[:, k, 0]
        xx = (wo - 1 + j) + o[:, k, 1]
        inside = (y > -1) & (xx > -1) & (y < H) & (xx < W)
        y0, x0 = torch.floor(y), torch.floor(xx)
        ly, lx = y - y0, xx - x0
        val = 0
        for dy, dx, wt in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
            yy, xq = y0 + dy, x0 + dx
            ok = inside & (yy >= 0) & (yy < H) & (xq >= 0) & (xq < W)
            idx = (yy.clamp(0, H - 1) * W + xq.clamp(0, W - 1)).long().view(N, 1, Ho * Wo).expand(N, C, Ho * Wo)
            val = val + torch.gather(flat, 2, idx) * (wt * ok).view(N, 1, Ho * Wo)
        cols.append(val * m[:, k].reshape(N, 1, Ho * Wo))
    col = torch.stack(cols, 2).reshape(N, C * kk, Ho * Wo)
    return torch.matmul(w.reshape(Co, C * kk), col).view(N, Co, Ho, Wo)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_dcn.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    frame = {}
    for name, (N, C, H, W, Co) in SHAPES.items():
        flop = 2.0 * N * H * W * C * 9 * Co
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn(N, C, H, W, generator=g).to(dev)
        w = ((torch.rand(Co, C, 3, 3, generator=g) * 2 - 1) / (C * 9) ** 0.5).to(dev)
        gout = torch.randn(N, Co, H, W, generator=g).to(dev)
        for kind in ("zero", "realistic"):
            if kind == "zero":
                off, m = torch.zeros(N, 18, H, W, device=dev), torch.ones(N, 9, H, W, device=dev)
            else:
                off = (torch.randn(N, 18, H, W, generator=g) * 1.5).to(dev)
                m = torch.rand(N, 9, H, W, generator=g).to(dev)
            paths = {"native": lambda *t: modulated_deform_conv2d(*t[:4], None, 1, 1, 1, 1, 1),
                     "torch_composition": lambda *t: torch_dcn(*t)}
            if a.native_only:
                paths = {"native": paths["native"]}
            for path, op in paths.items():
                leaves = [t.clone().requires_grad_(True) for t in (x, off, m, w)]

                def fwd():
                    with torch.no_grad():
                        op(x, off, m, w)

                def fwd_bwd():
                    for t in leaves:
                        t.grad = None
                    op(*leaves).backward(gout)

                f = timed(fwd, a.steps, a.warmup)
                fb = timed(fwd_bwd, a.steps, a.warmup)
                row = dict(bench="dcn", shape=name, offsets=kind, path=path, N=N, C=C, H=H, W=W, Co=Co,
                           fwd_us=round(f[0], 1), fwd_us_min=round(f[1], 1), fwd_bwd_us=round(fb[0], 1),
                           fwd_bwd_us_min=round(fb[1], 1), peak_fwd_mib=round(peak(fwd), 1),
                           peak_fwd_bwd_mib=round(peak(fwd_bwd), 1),
                           fwd_tflops=round(flop / f[0] / 1e6, 2), fwd_bwd_tflops=round(3 * flop / fb[0] / 1e6, 2))
                row["fwd_floor_frac"] = round(row["fwd_tflops"] / PEAK_TF, 3)
                row["fwd_bwd_floor_frac"] = round(row["fwd_bwd_tflops"] / PEAK_TF, 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
                if kind == "realistic":
                    fr = frame.setdefault(path, [0.0, 0.0])
                    fr[0] += BLOCKS[name] * f[0]
                    fr[1] += BLOCKS[name] * fb[0]
                del leaves
                torch.cuda.empty_cache()
        if not a.native_only:   # MIOpen conv2d at the same shape, context only
            xc = x.clone().requires_grad_(True)
            wc = w.clone().requires_grad_(True)

            def cfwd():
                with torch.no_grad():
                    F.conv2d(x, w, None, 1, 1)

            def cfb():
                xc.grad = wc.grad = None
                F.conv2d(xc, wc, None, 1, 1).backward(gout)

            f, fb = timed(cfwd, a.steps, a.warmup), timed(cfb, a.steps, a.warmup)
            row = dict(bench="dcn", shape=name, offsets="none", path="conv2d_miopen_context", fwd_us=round(f[0], 1),
                       fwd_bwd_us=round(fb[0], 1), fwd_tflops=round(flop / f[0] / 1e6, 2),
                       fwd_bwd_tflops=round(3 * flop / fb[0] / 1e6, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
    for path, (f, fb) in frame.items():
        row = dict(bench="dcn", shape="frame_23xlayer3_3xlayer4", offsets="realistic", path=path, fwd_us=round(f, 1),
                   fwd_bwd_us=round(fb, 1))
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
