#!/usr/bin/env python
"""The encoder's refinement tail (everything after the MLP), native (gaussianformer_amd.refine: one launch each way) against
the fp32 torch composition of tests/refine_ref.py on the same GPU -- what a user of the library runs today:

  version 1 (solid settings: restrict_xyz, refine_manual [0, 1, 2], softplus, opacity, 17 semantics; D = 28) at A = 25 600, 144 000
  version 2 (prob settings: unit_xyz [4, 4, 1], identity semantics; D = 28)                                  at A = 6 400, 25 600

Per shape and path: forward and forward + backward (gradients of every output, to output and anchor), eager and replayed from
a captured graph, µs as the median of the timed calls by HIP events (each call timed over --inner back-to-back runs); peak
device memory above the inputs; and for the native forward the fraction of 8 TB/s its algorithmic bytes
4 (2 D + Da + 10 + opa + S [+ 6]) per row reach (the kernel is memory-bound; at these sizes launch latency still shows).
Writes one JSON line per row to profiles/bench_refine.jsonl.  Needs an MI355X.

    python tools/bench_refine.py [--steps K] [--warmup W] [--inner N] [--native-only] [--out profiles/bench_refine.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refine_ref  # noqa: E402
from gaussianformer_amd import refine as R  # noqa: E402

PEAK_BYTES_PER_US = 8e6   # 8 TB/s
SHAPES = [("solid", 25600), ("solid", 144000), ("prob", 6400), ("prob", 25600)]


def timed(fn, steps, warmup, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(ts), min(ts)


def peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def captured(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_refine.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for family, A in SHAPES:
        g = refine_ref.FAMILIES[family]
        opa, S = int(g["include_opa"]), g["semantic_dim"]
        D = Da = 10 + opa + S
        gen = torch.Generator().manual_seed(0)
        o = (torch.randn(1, A, D, generator=gen) * 1.5).to(dev)
        an = (torch.randn(1, A, Da, generator=gen) * 1.5).to(dev)
        cfg = R.refine_config(g["version"], g["pc_range"], g["scale_range"], refine_ref.unit_of(g), g.get("restrict_xyz", False),
                              g.get("refine_manual", ()), S, g["include_opa"], g["semantics_activation"])

        def native(oo, aa):
            anchor_out, pred = R.refine(oo, aa, cfg)
            return [anchor_out] + [t for t in pred if t is not None and t.numel()]

        unit_xyz = torch.tensor(refine_ref.unit_of(g), dtype=torch.float32, device=dev) if g["version"] == 2 else None

        def composition(oo, aa):
            return [t for t in refine_ref.refine_tail(oo, aa, g, unit_xyz).values() if t.numel()]

        fwd_bytes = 4 * A * (2 * D + Da + 10 + opa + S + (6 if g["version"] == 2 else 0))
        paths = {"native": native} if a.native_only else {"native": native, "torch_composition": composition}
        for path, op in paths.items():
            ol, al = o.clone().requires_grad_(True), an.clone().requires_grad_(True)
            with torch.no_grad():
                gouts = [torch.randn_like(t) for t in op(o, an)]

            def fwd():
                with torch.no_grad():
                    op(o, an)

            def fwd_bwd():
                torch.autograd.grad(op(ol, al), (ol, al), gouts)

            row = dict(bench="refine", family=family, version=g["version"], A=A, D=D, path=path)
            for mode in ("eager", "graph"):
                f = timed(fwd if mode == "eager" else captured(fwd), a.steps, a.warmup, a.inner)
                fb = timed(fwd_bwd if mode == "eager" else captured(fwd_bwd), a.steps, a.warmup, a.inner)
                row.update({f"fwd_us_{mode}": round(f[0], 2), f"fwd_us_{mode}_min": round(f[1], 2),
                            f"fwd_bwd_us_{mode}": round(fb[0], 2), f"fwd_bwd_us_{mode}_min": round(fb[1], 2)})
            row.update(peak_fwd_mib=round(peak(fwd), 2), peak_fwd_bwd_mib=round(peak(fwd_bwd), 2), fwd_algorithmic_bytes=fwd_bytes,
                       fwd_graph_frac_of_8TBps=round(fwd_bytes / row["fwd_us_graph"] / PEAK_BYTES_PER_US, 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del ol, al, gouts
            torch.cuda.empty_cache()
    if not a.native_only:
        for nat, comp in zip(rows[0::2], rows[1::2]):
            row = dict(bench="refine", family=nat["family"], A=nat["A"], path="speedup_native_over_composition",
                       **{k: round(comp[k] / nat[k], 2) for k in ("fwd_us_eager", "fwd_bwd_us_eager", "fwd_us_graph", "fwd_bwd_us_graph")})
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
