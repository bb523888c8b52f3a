#!/usr/bin/env python
"""The anchor encoder's forward under ``no_grad``: the native op (gaussianformer_amd.anchor_encoder: one launch) against the
SAME module's torch layers (``forward_torch``, the reference's composition: about 40 kernels) on the same GPU and weights --
what a user of the reference's class runs today:

  (opa, S = 17; Da = 28) at A = 6 400, 25 600, 144 000        (no opa, S = 18; Da = 28) at A = 144 000

Per shape and path, eager and replayed from a captured graph: µs as the median of the timed calls by HIP events (each call
timed over --inner back-to-back runs), repeated --repeats times -- the row holds the median of those medians and their spread
(max - min), and "faster" means by more than the baseline's spread; peak device memory above the input and the weights; and
for the native op the TFLOP/s of its square layers -- one per branch present plus output_fc's two: seven at (opa, 17), six
at (no opa, 18), 2 x 128^2 FLOP per anchor each -- with the share of the fp32 matrix rate (157.3 TFLOP/s: the products are
exact fp32 MFMAs) they reach.  Writes one JSON line per row to
profiles/bench_anchor_embed.jsonl.  Needs an MI355X.

    python tools/bench_anchor_embed.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--native-only] [--shape I] [--out FILE]

Kernel time comes from runs of their own, one per shape so that no two shapes share a row of the statistics:
``rocprofv3 --kernel-trace --stats ... -- python tools/bench_anchor_embed.py --native-only --shape I --steps 5 --out /dev/null``
for I = 0 .. 3; profiles/kernel_stats_anchor_embed.csv holds the four runs' rows of the kernel, the shape in front."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import anchor_embed_ref as ref  # noqa: E402
from bench_refine import captured, peak, timed  # noqa: E402
from gaussianformer_amd.anchor_encoder import SparseGaussian3DEncoder  # noqa: E402

FP32_MATRIX_TFLOPS = 157.3
SQUARE_LAYER_FLOP_PER_ANCHOR = 2 * 128 * 128
SHAPES = [(True, 17, 6400), (True, 17, 25600), (True, 17, 144000), (False, 18, 144000)]


def repeated(fn, a):
    """(median of the repeats' medians, their spread, the least single timing)"""
    runs = [timed(fn, a.steps, a.warmup, a.inner) for _ in range(a.repeats)]
    meds = [r[0] for r in runs]
    return statistics.median(meds), max(meds) - min(meds), min(r[1] for r in runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_anchor_embed.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for opa, S, A in (SHAPES if a.shape is None else SHAPES[a.shape:a.shape + 1]):
        module = SparseGaussian3DEncoder(embed_dims=128, include_opa=opa, semantics=True, semantic_dim=S)
        module.load_state_dict(ref.fixed_weights(opa, S), strict=True)
        module.to(dev)
        Da = 10 + int(opa) + S
        x = torch.randn(1, A, Da, generator=torch.Generator().manual_seed(0)).to(dev)
        paths = {"native": module} if a.native_only else {"native": module, "torch_layers": module.forward_torch}
        for path, op in paths.items():
            def fwd():
                with torch.no_grad():
                    op(x)

            row = dict(bench="anchor_embed", include_opa=bool(opa), S=S, A=A, path=path)
            for mode in ("eager", "graph"):
                med, spread, least = repeated(fwd if mode == "eager" else captured(fwd), a)
                row.update({f"fwd_us_{mode}": round(med, 2), f"fwd_us_{mode}_spread": round(spread, 2), f"fwd_us_{mode}_min": round(least, 2)})
            row.update(peak_fwd_mib=round(peak(fwd), 2))
            if path == "native":
                square_layers = 3 + int(opa) + int(S > 0) + 2     # the branches present, then output_fc's two
                tf = square_layers * SQUARE_LAYER_FLOP_PER_ANCHOR * A / row["fwd_us_graph"] / 1e6
                row.update(square_layers=square_layers, square_tflops_graph=round(tf, 2), frac_of_fp32_matrix_rate=round(tf / FP32_MATRIX_TFLOPS, 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    if not a.native_only:
        for nat, base in zip(rows[0::2], rows[1::2]):
            row = dict(bench="anchor_embed", include_opa=nat["include_opa"], S=nat["S"], A=nat["A"], path="speedup_native_over_torch_layers")
            for mode in ("eager", "graph"):
                k = f"fwd_us_{mode}"
                row[k] = round(base[k] / nat[k], 2)
                row[f"{mode}_faster_by_more_than_baseline_spread"] = bool(base[k] - nat[k] > base[k + "_spread"])
            row["peak_mib_torch_over_native"] = round(base["peak_fwd_mib"] / max(nat["peak_fwd_mib"], 1e-9), 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
