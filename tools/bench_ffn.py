#!/usr/bin/env python
"""The encoder's feed-forward block under ``no_grad``: the native ``ffn_block`` (gaussianformer_amd.ffn: the FFN and the
LayerNorm that follows it in ONE launch) against the SAME module's torch layers (``forward_torch``, the reference's
composition) plus the ``"add"`` where the family has one and an ``nn.LayerNorm(128)``, on the same GPU and weights -- what a
user of the reference's class runs today:

  base (Cin = 256, pre_norm, identity_fc; "ffn", "norm")                at A = 6 400, 25 600, 144 000
  prob (Cin = 128, no pre_norm, no identity; "ffn", "add", "norm")      at A = 6 400, 25 600

Per shape and path, eager and replayed from a captured graph: µs as the median of the timed calls by HIP events (each call
timed over --inner back-to-back runs), repeated --repeats times -- the row holds the median of those medians and their spread
(max - min), and "faster" means by more than the baseline's spread; peak device memory above the input and the weights; and
for the native op the TFLOP/s of its products (2 (Cin 512 + 512 128 + Cin 128) FLOP per anchor, the last term only with
identity_fc) with the share of the fp32 matrix rate (157.3 TFLOP/s: the products are exact fp32 MFMAs) they reach.  Writes
one JSON line per row to profiles/bench_ffn.jsonl.  Needs an MI355X.

    python tools/bench_ffn.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--native-only] [--shape I] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ffn_ref as ref  # noqa: E402
from bench_anchor_embed import FP32_MATRIX_TFLOPS, repeated  # noqa: E402
from bench_refine import captured, peak  # noqa: E402
from gaussianformer_amd.ffn import AsymmetricFFN, ffn_block  # noqa: E402

SHAPES = [("base", 6400), ("base", 25600), ("base", 144000), ("prob", 6400), ("prob", 25600)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_ffn.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for family, A in (SHAPES if a.shape is None else SHAPES[a.shape:a.shape + 1]):
        shapes = ref.family_shapes(family)
        cin, ident = shapes["layers.0.0.weight"][1], "identity_fc.weight" in shapes
        weights = ref.fixed_weights(cin, "pre_norm.weight" in shapes, ident)
        module = AsymmetricFFN(**ref.FAMILIES[family])
        module.load_state_dict(ref.module_state(weights), strict=True)
        norm = torch.nn.LayerNorm(ref.E)
        norm.load_state_dict({"weight": weights["norm.weight"], "bias": weights["norm.bias"]})
        module.to(dev).eval()
        norm.to(dev)
        add = ref.FOLLOWED_BY_ADD[family]
        x = torch.randn(1, A, cin, generator=torch.Generator().manual_seed(0)).to(dev)

        def native():
            return ffn_block(x, module, norm=norm, residual=x if add else None)

        def torch_layers():
            out = module.forward_torch(x)
            return norm(out + x if add else out)
        paths = {"native": native} if a.native_only else {"native": native, "torch_layers": torch_layers}
        for path, op in paths.items():
            def fwd():
                with torch.no_grad():
                    op()

            row = dict(bench="ffn", family=family, Cin=cin, A=A, path=path)
            for mode in ("eager", "graph"):
                med, spread, least = repeated(fwd if mode == "eager" else captured(fwd), a)
                row.update({f"fwd_us_{mode}": round(med, 2), f"fwd_us_{mode}_spread": round(spread, 2), f"fwd_us_{mode}_min": round(least, 2)})
            row.update(peak_fwd_mib=round(peak(fwd), 2))
            if path == "native":
                flop = 2 * (cin * ref.HIDDEN + ref.HIDDEN * ref.E + (cin * ref.E if ident else 0))
                tf = flop * A / row["fwd_us_graph"] / 1e6
                row.update(flop_per_anchor=flop, tflops_graph=round(tf, 2), frac_of_fp32_matrix_rate=round(tf / FP32_MATRIX_TFLOPS, 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    if not a.native_only:
        for nat, base in zip(rows[0::2], rows[1::2]):
            row = dict(bench="ffn", family=nat["family"], Cin=nat["Cin"], A=nat["A"], path="speedup_native_over_torch_layers")
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
