#!/usr/bin/env python
"""The whole encoder under ``no_grad``: the drop-in ``GaussianOccEncoder`` (gaussianformer_amd.encoder) built from the recorded
settings of the shipped configs (tests/golden/encoder_orders.json), with ``fold = True`` (one fused call per step of the plan)
against the SAME module with ``fold = False`` (the reference's loop: every ``"add"`` and ``"norm"`` a torch op of its own), on
the same GPU, weights, anchors and feature pyramid:

  nuscenes_gs25600_solid   A = 25 600     ("cat"; "ffn", "norm" and "spconv", "norm" fold)
  nuscenes_gs144000        A = 144 000    (the same order, no output_proj in the sparse block)
  prob/nuscenes_gs6400     A = 6 400      (every "identity", X, "add", "norm" folds; multi-layer sparse block)
  prob/nuscenes_gs25600    A = 25 600

The sparse block's rulebook is sized by ``pairs_per_point`` so that nothing is read back and the frame can be captured; after
the eager run every rulebook is checked (a refused one would time an empty convolution).  Per shape and path, eager and
replayed from a captured graph: µs as the median of the timed calls by HIP events, repeated --repeats times -- the row holds
the median of those medians and their spread (max - min); the number of library launches per frame; and the peak device memory
above the inputs and the weights.  Writes one JSON line per row to profiles/bench_encoder.jsonl.  Needs an MI355X.

    python tools/bench_encoder.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--shape I] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_anchor_embed import repeated  # noqa: E402
from bench_deform_block import CAMS, cameras  # noqa: E402
from bench_refine import captured, peak  # noqa: E402
from bench_sparse_block import speedup_row  # noqa: E402
from gaussianformer_amd import GaussianOccEncoder, _lib, synthetic  # noqa: E402
from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF  # noqa: E402

SHAPES = [("nuscenes_gs25600_solid", 25600, 64), ("nuscenes_gs144000", 144000, 96), ("prob/nuscenes_gs6400", 6400, 64),
          ("prob/nuscenes_gs25600", 25600, 64)]      # (family, anchors, pairs_per_point)


def launches(fn):
    """The library calls of one run of ``fn``."""
    names, real = [], _lib.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = call
    try:
        fn()
    finally:
        _lib.call = real
    return len(names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_encoder.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "encoder_orders.json")) as f:
        recorded = json.load(f)
    g = torch.Generator().manual_seed(0)
    table = DAF.feature_maps_format([torch.randn(1, CAMS, 128, h, w, generator=g).to(dev) for h, w in synthetic.DAF_LEVELS])
    pm, wh = cameras(dev)
    metas = dict(projection_mat=pm, image_wh=wh)
    rows = []
    for family, A, ppp in (SHAPES if a.shape is None else SHAPES[a.shape:a.shape + 1]):
        cfg = dict(recorded[family])
        cfg["spconv_layer"] = dict(cfg["spconv_layer"], pairs_per_point=ppp)
        torch.manual_seed(0)
        enc = GaussianOccEncoder(**cfg)
        enc.init_weights()
        enc.to(dev).eval()
        dim = 10 + int(cfg["anchor_encoder"]["include_opa"]) + cfg["anchor_encoder"]["semantic_dim"]
        anchor = torch.randn(1, A, dim, generator=g)
        anchor[..., :3] *= 1.5
        anchor = anchor.to(dev)
        inst = torch.randn(1, A, 128, generator=g).to(dev)
        pair_rows = []
        for path, fold in (("fold", True), ("op_by_op", False)):
            def fwd():
                enc.fold = fold
                with torch.no_grad():
                    enc(anchor, inst, table, metas)

            n_launches = launches(fwd)
            refused = False
            for m in enc.layers:                       # a refused rulebook would time an empty convolution: say so in the row
                if getattr(m, "last_rulebook", None) is not None:
                    try:
                        m.last_rulebook.check()
                    except RuntimeError:
                        refused = True
            row = dict(bench="encoder", family=family, A=A, ops=len(enc.operation_order), steps=len(enc.steps), path=path,
                       library_launches=n_launches, rulebook_refused=refused)
            for timing in ("eager", "graph"):
                med, spread, least = repeated(fwd if timing == "eager" else captured(fwd), a)
                row.update({f"fwd_us_{timing}": round(med, 2), f"fwd_us_{timing}_spread": round(spread, 2), f"fwd_us_{timing}_min": round(least, 2)})
            row.update(peak_fwd_mib=round(peak(fwd), 2))
            pair_rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        rows += pair_rows + [speedup_row("encoder", *pair_rows, family=family, A=A)]
        print(json.dumps(rows[-1]), flush=True)
        del enc
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
