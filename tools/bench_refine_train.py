#!/usr/bin/env python
"""One training step of the refinement modules at E = 128: the module with ``native_training = True`` (the saving forward
gf_refine_mlp_forward_train and gf_refine_mlp_backward) against the SAME module with the attribute False on the same build --
the torch MLP with torch's backward and the one-launch tail each way, what a training call runs by default:

  solid (version 1, D = 28) at A = 25 600, 144 000
  prob  (version 2, D = 28) at A = 6 400, 25 600

One step = the forward, the fixed scalar ``refine_ref.weighted_sum`` over its outputs and ``torch.autograd.grad`` of it for the
three inputs and the 15 parameters.  Per shape and path, eager and replayed from a captured graph: µs as the median of the
timed calls by HIP events (each call timed over --inner back-to-back steps), repeated --repeats times -- the row holds the
median of those medians and their spread (max - min) --, and the peak device memory of a step above the inputs and the weights.
The statement a row makes or withholds: "faster than the default route by more than BOTH spreads, with peak memory not above
it".  Writes one JSON line per row to profiles/bench_refine_train.jsonl.  Needs an MI355X.

    python tools/bench_refine_train.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--native-only] [--shape I] [--out FILE]

Kernel time comes from runs of their own, one per shape: ``rocprofv3 --kernel-trace --stats ... -- python
tools/bench_refine_train.py --native-only --shape I --steps 5 --repeats 1 --out /dev/null`` for I = 0 .. 3;
profiles/kernel_stats_refine_train.csv holds the four runs' rows of the step's kernels, the shape in front."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refine_ref  # noqa: E402
from bench_anchor_embed import repeated  # noqa: E402
from bench_refine import captured, peak  # noqa: E402
from bench_refine_fused import SHAPES, E  # noqa: E402
from gaussianformer_amd import refine as R  # noqa: E402

PATHS = ("native_training", "default")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_refine_train.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for family, A in (SHAPES if a.shape is None else SHAPES[a.shape:a.shape + 1]):
        g = refine_ref.FAMILIES[family]
        cls = R.SparseGaussian3DRefinementModule if g["version"] == 1 else R.SparseGaussian3DRefinementModuleV2
        torch.manual_seed(0)
        module = cls(embed_dims=E, **{k: v for k, v in g.items() if k != "version"})
        rng = np.random.default_rng(0)
        with torch.no_grad():   # LayerNorm and Scale away from the identity
            for p in module.parameters():
                p.add_(torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)) * 0.1)
        module.to(dev).train()
        D = module.output_dim
        gen = torch.Generator().manual_seed(0)
        feat, embed = (torch.randn(1, A, E, generator=gen).to(dev).requires_grad_(True) for _ in range(2))
        anchor = (torch.randn(1, A, D, generator=gen) * 1.5).to(dev).requires_grad_(True)
        leaves = [feat, anchor, embed] + list(module.parameters())

        def named(res):
            return dict(anchor_out=res[0], **{k: v for k, v in res[1]._asdict().items() if v is not None})

        with torch.no_grad():
            weights = refine_ref.fixed_weights(named(module(feat, anchor, embed)))
        by_path = {}
        for path in (PATHS[:1] if a.native_only else PATHS):
            module.native_training = path == "native_training"

            def step():
                torch.autograd.grad(refine_ref.weighted_sum(named(module(feat, anchor, embed)), weights), leaves)

            row = dict(bench="refine_train", family=family, version=g["version"], A=A, D=D, path=path)
            for mode in ("eager", "graph"):
                med, spread, least = repeated(step if mode == "eager" else captured(step), a)
                row.update({f"step_us_{mode}": round(med, 2), f"step_us_{mode}_spread": round(spread, 2), f"step_us_{mode}_min": round(least, 2)})
            R._train_scratch._cache.clear()     # the backward's cached workspace counts towards the step's peak
            torch.cuda.empty_cache()
            row.update(peak_step_mib=round(peak(step), 2))
            rows.append(row)
            by_path[path] = row
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        module.native_training = False
        if not a.native_only:
            base, nat = by_path["default"], by_path["native_training"]
            row = dict(bench="refine_train", family=family, A=A, path="speedup_native_training_over_default")
            for mode in ("eager", "graph"):
                k = f"step_us_{mode}"
                row[k] = round(base[k] / nat[k], 2)
                row[f"{mode}_faster_by_more_than_both_spreads"] = bool(base[k] - nat[k] > max(base[k + "_spread"], nat[k + "_spread"]))
            row["peak_mib_default_over_native"] = round(base["peak_step_mib"] / max(nat["peak_step_mib"], 1e-9), 2)
            row["peak_memory_not_above_default"] = bool(nat["peak_step_mib"] <= base["peak_step_mib"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
