#!/usr/bin/env python
"""The anchor encoder's training step, forward + backward: ``SparseGaussian3DEncoder`` with ``native_training = True``
(gf_anchor_embed_forward_train + gf_anchor_embed_backward: five launches) against the SAME module's torch layers (the route a
training call takes by default: about 40 forward kernels and torch's backward of them) on the same GPU and weights:

  (opa, S = 17; Da = 28) at A = 6 400, 25 600, 144 000        (no opa, S = 18; Da = 28) at A = 144 000

One step = the forward, the scalar ``sum(out * w)`` and ``torch.autograd.grad`` of it for the anchor and every parameter.  Per
shape and path, eager and replayed from a captured graph: µs as the median of the timed calls by HIP events (each call timed
over --inner back-to-back steps), repeated --repeats times -- the row holds the median of those medians and their spread
(max - min) --, and the peak device memory of a step above the input and the weights.  The statement a row makes or withholds:
"faster than the torch route by more than BOTH spreads, with peak memory not above it".  Writes one JSON line per row to
profiles/bench_anchor_embed_train.jsonl.  Needs an MI355X.

    python tools/bench_anchor_embed_train.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--native-only] [--shape I] [--out FILE]

Kernel time comes from runs of their own, one per shape so that no two shapes share a row of the statistics:
``rocprofv3 --kernel-trace --stats ... -- python tools/bench_anchor_embed_train.py --native-only --shape I --steps 5 --repeats 1
--out /dev/null`` for I = 0 .. 3; profiles/kernel_stats_anchor_embed_train.csv holds the runs' rows of the op's kernels, the
shape in front."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import anchor_embed_ref as ref  # noqa: E402
from bench_anchor_embed import SHAPES, repeated  # noqa: E402
from bench_refine import captured, peak  # noqa: E402
from gaussianformer_amd.anchor_encoder import SparseGaussian3DEncoder  # noqa: E402

PATHS = {"native_training": True, "torch_layers": False}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_anchor_embed_train.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for opa, S, A in (SHAPES if a.shape is None else SHAPES[a.shape:a.shape + 1]):
        Da = 10 + int(opa) + S
        x = torch.randn(1, A, Da, generator=torch.Generator().manual_seed(0)).to(dev).requires_grad_(True)
        w = ref.output_weights((1, A, 128), torch.float32).to(dev)
        for path, native in PATHS.items():
            if a.native_only and not native:
                continue
            module = SparseGaussian3DEncoder(embed_dims=128, include_opa=opa, semantics=True, semantic_dim=S)
            module.native_training = native
            module.load_state_dict(ref.fixed_weights(opa, S), strict=True)
            module.to(dev)
            leaves = [x] + list(module.parameters())

            def step():
                torch.autograd.grad((module(x) * w).sum(), leaves)

            row = dict(bench="anchor_embed_train", include_opa=bool(opa), S=S, A=A, path=path)
            for mode in ("eager", "graph"):
                med, spread, least = repeated(step if mode == "eager" else captured(step), a)
                row.update({f"step_us_{mode}": round(med, 2), f"step_us_{mode}_spread": round(spread, 2), f"step_us_{mode}_min": round(least, 2)})
            row.update(peak_step_mib=round(peak(step), 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del module, leaves
            torch.cuda.empty_cache()
    if not a.native_only:
        for nat, base in zip(rows[0::2], rows[1::2]):
            row = dict(bench="anchor_embed_train", include_opa=nat["include_opa"], S=nat["S"], A=nat["A"], path="speedup_native_over_torch_layers")
            for mode in ("eager", "graph"):
                k = f"step_us_{mode}"
                row[k] = round(base[k] / nat[k], 2)
                row[f"{mode}_faster_by_more_than_both_spreads"] = bool(base[k] - nat[k] > max(base[k + "_spread"], nat[k + "_spread"]))
            row["peak_mib_torch_over_native"] = round(base["peak_step_mib"] / max(nat["peak_step_mib"], 1e-9), 2)
            row["peak_memory_not_above_torch"] = bool(nat["peak_step_mib"] <= base["peak_step_mib"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
