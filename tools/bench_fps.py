"""Farthest point sampling at the lifter's shapes: N = 129 600 lifter-shaped candidates
(gaussianformer_amd.synthetic.make_lifter_points) and M = num_anchor = 4 000 / 6 400 / 19 200.  Per shape, one JSON line:
  ms          the pruned kernel, per call (device events around back-to-back calls, after a warm-up)
  us_per_pick ms / M
  exhaustive_ms   gf_set_option("fps.exhaustive", 1): every bucket updated on every pick (the brute-force baseline)
  torch_loop_ms   a torch-composed loop on the GPU (what a ROCm user without pointops would write), one timed call
and whether the pruned and exhaustive picks are identical.  ``--quick`` times M = 4 000 only."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianformer_amd import _lib  # noqa: E402
from gaussianformer_amd.synthetic import make_lifter_points  # noqa: E402
from pointops import farthest_point_sampling  # noqa: E402


def timed_ms(fn, warm=1, iters=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def torch_loop(xyz, m):
    n = xyz.shape[0]
    d = torch.full((n,), 1e10, dtype=torch.float32, device=xyz.device)
    idx = torch.empty(m, dtype=torch.long, device=xyz.device)
    cur = torch.zeros((), dtype=torch.long, device=xyz.device)
    for i in range(m):
        idx[i] = cur
        diff = xyz - xyz[cur]
        d = torch.minimum(d, (diff * diff).sum(1))
        cur = torch.argmax(d)
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch loop (e.g. under a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fps needs an MI355X"
    dev = torch.device("cuda:0")
    xyz = torch.from_numpy(make_lifter_points(seed=args.seed)).to(dev)
    n = xyz.shape[0]
    off = torch.tensor([n], dtype=torch.int32, device=dev)
    for m in ([4000] if args.quick else [4000, 6400, 19200]):
        new = torch.tensor([m], dtype=torch.int32, device=dev)
        call = lambda: farthest_point_sampling(xyz, off, new)  # noqa: E731
        ms = timed_ms(call)
        with _lib.option("fps.exhaustive", 1):
            ex_ms = timed_ms(call, warm=1, iters=2)
            ex = call()
        same = bool(torch.equal(call(), ex))
        row = {"op": "farthest_point_sampling", "N": n, "M": m, "ms": round(ms, 3), "us_per_pick": round(ms * 1e3 / m, 3),
               "exhaustive_ms": round(ex_ms, 3), "pruned_equals_exhaustive": same}
        if not args.no_torch:
            row["torch_loop_ms"] = round(timed_ms(lambda: torch_loop(xyz, m), warm=1, iters=1), 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
