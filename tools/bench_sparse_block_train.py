#!/usr/bin/env python
"""One training step, forward + backward, of the prob configs' sparse convolution block (``SparseConv3D`` with
``use_multi_layer``: 3 x (conv + bias, LayerNorm, ReLU), ``output_proj``, "add", "norm"; kernel 5, grid 1 m, width 128) with
``native_training = True`` -- the stages' saving forward and their backward inside the data-gradient convolutions (DESIGN.md
§3.7c) -- against the SAME module with ``native_training = False``: torch's bias add, LayerNorm and ReLU and their backwards
around the same convolution kernels, on the same GPU, weights and anchors, at A = 6 400, 12 800 and 25 600.

The rulebook is sized by ``pairs_per_point`` (taken from one exact build of the same anchors, rounded up), so the step reads
nothing back.  The two sides ALTERNATE in one process: --repeats rounds, each timing first one side, then the other (the median
of --steps timings by HIP events, each over --inner back-to-back steps); a row holds the median of those medians, their spread
(max - min) and the least single timing, and the peak device memory of one step above the inputs and the weights.  Writes one
JSON line per row to profiles/bench_sparse_block_train.jsonl.  There is no threshold: the attribute is opt-in.  Needs an MI355X.

    python tools/bench_sparse_block_train.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--shape I] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_refine import peak, timed  # noqa: E402
from gaussianformer_amd.sparse_conv import SparseConv3D  # noqa: E402

PC_RANGE = [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0]
SHAPES = [6400, 12800, 25600]
PATHS = (("native_training", True), ("torch_tail", False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_sparse_block_train.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows = []
    for A in (SHAPES if a.shape is None else SHAPES[a.shape:a.shape + 1]):
        torch.manual_seed(0)
        module = SparseConv3D(128, 128, PC_RANGE, [1.0] * 3, use_out_proj=True, kernel_size=5, use_multi_layer=True).to(dev).train()
        norm = torch.nn.LayerNorm(128).to(dev)
        anchor = torch.randn(1, A, 28, generator=g)
        anchor[..., :3] *= 1.5
        anchor = anchor.to(dev)
        inst = torch.randn(1, A, 128, generator=g).to(dev).requires_grad_(True)
        residual = torch.randn(1, A, 128, generator=g).to(dev).requires_grad_(True)
        cot = torch.randn(1, A, 128, generator=g).to(dev)
        with torch.no_grad():
            module(inst, anchor)
            pairs = int(module.last_rulebook.total)
        module.pairs_per_point = -(-pairs // A) + 1
        leaves = [inst, residual, *module.parameters(), *norm.parameters()]

        def step(native):
            def run():
                module.native_training = native
                out = module(inst, anchor, residual=residual, norm=norm)
                torch.autograd.grad((out * cot).sum(), leaves)
            return run
        meds = {path: [] for path, _ in PATHS}
        least = {path: float("inf") for path, _ in PATHS}
        for _ in range(a.repeats):                  # the sides alternate: a drift of the clocks meets both
            for path, native in PATHS:
                med, low = timed(step(native), a.steps, a.warmup, a.inner)
                meds[path].append(med)
                least[path] = min(least[path], low)
        pair_rows = []
        for path, native in PATHS:
            m = meds[path]
            row = dict(bench="sparse_block_train", family="multi_proj", A=A, pairs=pairs, pairs_per_point=module.pairs_per_point, path=path,
                       step_us=round(statistics.median(m), 2), step_us_spread=round(max(m) - min(m), 2), step_us_min=round(least[path], 2),
                       peak_step_mib=round(peak(step(native)), 2))
            pair_rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        nat, base = pair_rows
        rows += pair_rows + [dict(bench="sparse_block_train", family="multi_proj", A=A, path="speedup_native_over_torch",
                                  step_us=round(base["step_us"] / nat["step_us"], 3),
                                  faster_by_more_than_spread=bool(base["step_us"] - nat["step_us"] > max(base["step_us_spread"], nat["step_us_spread"])),
                                  slower_by_more_than_spread=bool(nat["step_us"] - base["step_us"] > max(base["step_us_spread"], nat["step_us_spread"])),
                                  peak_mib_torch_over_native=round(base["peak_step_mib"] / max(nat["peak_step_mib"], 1e-9), 2))]
        print(json.dumps(rows[-1]), flush=True)
        del module.native_training
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
