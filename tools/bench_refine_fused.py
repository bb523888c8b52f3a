#!/usr/bin/env python
"""The refinement modules' whole forward under ``no_grad`` at E = 128: the module with ``fused_mlp = True`` (the MLP and the
tail in ONE launch, gf_refine_mlp_forward) against the SAME module with the attribute False on the same build -- the torch MLP
(a dozen kernels) and the one-launch tail, what the module runs by default:

  solid (version 1, D = 28) at A = 25 600, 144 000
  prob  (version 2, D = 28) at A = 6 400, 25 600

Per shape and path, forward only, eager and replayed from a captured graph: µs as the median of the timed calls by HIP events
(each call timed over --inner back-to-back runs), repeated --repeats times -- the row holds the median of those medians and
their spread (max - min), and "faster" means by more than BOTH paths' spreads; peak device memory above the inputs and the
weights; and for the fused path the TFLOP/s of its products (2 (4 x 128 x 128 + 128 D) FLOP per anchor) with the share of the
fp32 matrix rate (157.3 TFLOP/s: the products are exact fp32 MFMAs) they reach.  Writes one JSON line per row to
profiles/bench_refine_fused.jsonl.  Needs an MI355X.

    python tools/bench_refine_fused.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--fused-only] [--shape I] [--out FILE]

Kernel time comes from runs of their own, one per shape: ``rocprofv3 --kernel-trace --stats ... -- python
tools/bench_refine_fused.py --fused-only --shape I --steps 5 --repeats 1 --out /dev/null`` for I = 0 .. 3;
profiles/kernel_stats_refine_fused.csv holds the four runs' rows of the kernel, the shape in front."""
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
from bench_anchor_embed import FP32_MATRIX_TFLOPS, repeated  # noqa: E402
from bench_refine import captured, peak  # noqa: E402
from gaussianformer_amd import refine as R  # noqa: E402

E = 128
SHAPES = [("solid", 25600), ("solid", 144000), ("prob", 6400), ("prob", 25600)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_refine_fused.jsonl"))
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
        module.to(dev).eval()
        D = module.output_dim
        gen = torch.Generator().manual_seed(0)
        feat, embed = (torch.randn(1, A, E, generator=gen).to(dev) for _ in range(2))
        anchor = (torch.randn(1, A, D, generator=gen) * 1.5).to(dev)
        for path in (("fused",) if a.fused_only else ("fused", "default")):
            def fwd():
                module.fused_mlp = path == "fused"
                with torch.no_grad():
                    module(feat, anchor, embed)

            row = dict(bench="refine_fused", family=family, version=g["version"], A=A, D=D, path=path)
            for mode in ("eager", "graph"):
                med, spread, least = repeated(fwd if mode == "eager" else captured(fwd), a)
                row.update({f"fwd_us_{mode}": round(med, 2), f"fwd_us_{mode}_spread": round(spread, 2), f"fwd_us_{mode}_min": round(least, 2)})
            row.update(peak_fwd_mib=round(peak(fwd), 2))
            if path == "fused":
                flop = 2 * (4 * E * E + E * D)
                tf = flop * A / row["fwd_us_graph"] / 1e6
                row.update(flop_per_anchor=flop, tflops_graph=round(tf, 2), frac_of_fp32_matrix_rate=round(tf / FP32_MATRIX_TFLOPS, 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        module.fused_mlp = False
    if not a.fused_only:
        for fused, base in zip(rows[0::2], rows[1::2]):
            row = dict(bench="refine_fused", family=fused["family"], A=fused["A"], path="speedup_fused_over_default")
            for mode in ("eager", "graph"):
                k = f"fwd_us_{mode}"
                row[k] = round(base[k] / fused[k], 2)
                row[f"{mode}_faster_by_more_than_both_spreads"] = bool(base[k] - fused[k] > max(base[k + "_spread"], fused[k + "_spread"]))
            row["peak_mib_default_over_fused"] = round(base["peak_fwd_mib"] / max(fused["peak_fwd_mib"], 1e-9), 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
