#!/usr/bin/env python
"""The feed-forward block's training step, forward + backward, in train mode with ``ffn_drop = 0.1``: ``AsymmetricFFN`` with
``native_training = True`` (gf_ffn_forward_train + gf_ffn_backward, masks drawn as uint8) and the ``"add"`` / ``"norm"`` that
follow it as torch ops, against the SAME module's torch layers (the route a training call takes by default) with the same add
and norm, on the same GPU and weights -- and, as a third path, ``ffn_block_autograd``, which takes the add and the norm into
the native step as well:

  base (Cin = 256, pre_norm, identity_fc; "ffn", "norm")                at A = 6 400, 25 600, 144 000
  prob (Cin = 128, no pre_norm, no identity; "ffn", "add", "norm")      at A = 6 400, 25 600

One step = the forward, the scalar ``sum(out * w)`` and ``torch.autograd.grad`` of it for x (which is the residual too, where
the family adds) and every parameter.  Per shape and path, eager and replayed from a captured graph: µs as the median of the
timed calls by HIP events (each call timed over --inner back-to-back steps), repeated --repeats times -- the row holds the
median of those medians and their spread (max - min) --, and the peak device memory of a step above the input and the weights.
The statement a row makes or withholds: "faster than the torch route by more than BOTH spreads, with peak memory not above it".
Writes one JSON line per row to profiles/bench_ffn_train.jsonl.  Needs an MI355X.

    python tools/bench_ffn_train.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--native-only] [--shape I] [--out FILE]

Kernel time comes from runs of their own, one per shape: ``rocprofv3 --kernel-trace --stats ... -- python
tools/bench_ffn_train.py --native-only --shape I --steps 5 --repeats 1 --out /dev/null`` for I = 0 .. 4."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ffn_ref as ref  # noqa: E402
from anchor_embed_ref import output_weights  # noqa: E402
from bench_anchor_embed import repeated  # noqa: E402
from bench_ffn import SHAPES  # noqa: E402
from bench_refine import captured, peak  # noqa: E402
from gaussianformer_amd.ffn import AsymmetricFFN, ffn_block_autograd  # noqa: E402

PATHS = ("native_training", "native_block", "torch_layers")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_ffn_train.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for family, A in (SHAPES if a.shape is None else SHAPES[a.shape:a.shape + 1]):
        shapes = ref.family_shapes(family)
        cin, ident = shapes["layers.0.0.weight"][1], "identity_fc.weight" in shapes
        weights = ref.fixed_weights(cin, "pre_norm.weight" in shapes, ident)
        add = ref.FOLLOWED_BY_ADD[family]
        x = torch.randn(1, A, cin, generator=torch.Generator().manual_seed(0)).to(dev).requires_grad_(True)
        w = output_weights((1, A, ref.E), torch.float32).to(dev)
        by_path = {}
        for path in PATHS:
            if a.native_only and path == "torch_layers":
                continue
            module = AsymmetricFFN(**ref.FAMILIES[family])      # ffn_drop = 0.1
            module.load_state_dict(ref.module_state(weights), strict=True)
            module.native_training = path == "native_training"
            norm = torch.nn.LayerNorm(ref.E)
            norm.load_state_dict({"weight": weights["norm.weight"], "bias": weights["norm.bias"]})
            module.to(dev).train()
            norm.to(dev).train()
            leaves = [x] + list(module.parameters()) + list(norm.parameters())
            p_hidden, p_out = module.layers[0][2].p, module.layers[2].p

            def step():
                if path == "native_block":
                    out = ffn_block_autograd(x, module, norm=norm, residual=x if add else None, p_hidden=p_hidden, p_out=p_out)
                else:
                    out = module(x)
                    out = norm(out + x if add else out)
                torch.autograd.grad((out * w).sum(), leaves)

            row = dict(bench="ffn_train", family=family, Cin=cin, A=A, path=path)
            for mode in ("eager", "graph"):
                med, spread, least = repeated(step if mode == "eager" else captured(step), a)
                row.update({f"step_us_{mode}": round(med, 2), f"step_us_{mode}_spread": round(spread, 2), f"step_us_{mode}_min": round(least, 2)})
            row.update(peak_step_mib=round(peak(step), 2))
            rows.append(row)
            by_path[path] = row
            print(json.dumps(row), flush=True)
            del module, norm, leaves
            torch.cuda.empty_cache()
        if not a.native_only:
            base = by_path["torch_layers"]
            for path in PATHS[:2]:
                nat = by_path[path]
                row = dict(bench="ffn_train", family=family, Cin=cin, A=A, path=f"speedup_{path}_over_torch_layers")
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
