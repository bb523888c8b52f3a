#!/usr/bin/env python
"""The sparse convolution block under ``no_grad``: ``SparseConv3D.forward`` with its dense tail native (``native_tail = True``:
bias, LayerNorm, ReLU, residual and the post norm inside the convolutions' last pass, ``output_proj`` with the add and the norm
in one ``gf_deform_output_forward`` launch) against the SAME module with ``native_tail = False`` (the torch layers behind the
same convolution kernels: what the block ran before), on the same GPU, weights and anchors, kernel 5:

  single      conv -> "norm"                                    grid 0.5 m   at A = 144 000   (nuscenes_gs144000)
  single_proj conv -> output_proj -> "norm"                     grid 0.5 m   at A = 25 600    (nuscenes_gs25600_solid)
  multi_proj  3 x (conv + bias, LN, ReLU), output_proj, "add", "norm"   grid 1 m   at A = 6 400, 25 600   (prob/)

The rulebook is sized by ``pairs_per_point`` (taken from one exact build of the same anchors, rounded up), so nothing is read
back and the call can be captured.  Per shape and path, eager and replayed from a captured graph: µs as the median of the timed
calls by HIP events (each call timed over --inner back-to-back runs), repeated --repeats times -- the row holds the median of
those medians and their spread (max - min); and the peak device memory above the inputs and the weights.  Writes one JSON line
per row to profiles/bench_sparse_block.jsonl.  Needs an MI355X.

    python tools/bench_sparse_block.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--shape I] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_anchor_embed import repeated  # noqa: E402
from bench_refine import captured, peak  # noqa: E402
from gaussianformer_amd.sparse_conv import SparseConv3D  # noqa: E402

PC_RANGE = [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0]
SHAPES = [("single_proj", 25600), ("single", 144000), ("multi_proj", 6400), ("multi_proj", 25600)]
FAMILIES = {"single": dict(use_out_proj=False, use_multi_layer=False, grid=0.5, residual=False),
            "single_proj": dict(use_out_proj=True, use_multi_layer=False, grid=0.5, residual=False),
            "multi_proj": dict(use_out_proj=True, use_multi_layer=True, grid=1.0, residual=True)}


def speedup_row(bench, nat, base, **keys):
    row = dict(bench=bench, path="speedup_native_over_torch", **keys)
    for timing in ("eager", "graph"):
        k = f"fwd_us_{timing}"
        row[k] = round(base[k] / nat[k], 3)
        row[f"{timing}_faster_by_more_than_baseline_spread"] = bool(base[k] - nat[k] > base[k + "_spread"])
        row[f"{timing}_slower_by_more_than_spread"] = bool(nat[k] - base[k] > max(base[k + "_spread"], nat[k + "_spread"]))
    row["peak_mib_torch_over_native"] = round(base["peak_fwd_mib"] / max(nat["peak_fwd_mib"], 1e-9), 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_sparse_block.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows = []
    for family, A in (SHAPES if a.shape is None else SHAPES[a.shape:a.shape + 1]):
        fam = FAMILIES[family]
        torch.manual_seed(0)
        module = SparseConv3D(128, 128, PC_RANGE, [fam["grid"]] * 3, use_out_proj=fam["use_out_proj"], kernel_size=5,
                              use_multi_layer=fam["use_multi_layer"]).to(dev).eval()
        norm = torch.nn.LayerNorm(128).to(dev)
        anchor = torch.randn(1, A, 28, generator=g)
        anchor[..., :3] *= 1.5
        anchor = anchor.to(dev)
        inst = torch.randn(1, A, 128, generator=g).to(dev)
        residual = torch.randn(1, A, 128, generator=g).to(dev) if fam["residual"] else None
        with torch.no_grad():
            module(inst, anchor)
            pairs = int(module.last_rulebook.total)
        module.pairs_per_point = -(-pairs // A) + 1
        pair_rows = []
        for path, native in (("native_tail", True), ("torch_tail", False)):
            def fwd():
                module.native_tail = native
                with torch.no_grad():
                    module(inst, anchor, residual=residual, norm=norm)

            row = dict(bench="sparse_block", family=family, A=A, pairs=pairs, pairs_per_point=module.pairs_per_point, path=path)
            for timing in ("eager", "graph"):
                med, spread, least = repeated(fwd if timing == "eager" else captured(fwd), a)
                row.update({f"fwd_us_{timing}": round(med, 2), f"fwd_us_{timing}_spread": round(spread, 2), f"fwd_us_{timing}_min": round(least, 2)})
            row.update(peak_fwd_mib=round(peak(fwd), 2))
            pair_rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        rows += pair_rows + [speedup_row("sparse_block", *pair_rows, family=family, A=A)]
        print(json.dumps(rows[-1]), flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
