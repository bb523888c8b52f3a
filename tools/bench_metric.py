#!/usr/bin/env python
"""The evaluation metric's per-frame step at the evaluation's own shape: 200 x 200 x 16 = 640 000 voxels, int64 predictions
and targets drawn by the nuScenes class frequencies (about 78 % empty), a camera mask that keeps about a third -- eval.py:163's
call ``miou_metric._after_step(pred_occ, gt_occ, occ_mask)``.

  step            MeanIoU._after_step on labels (gf_miou_step: counting pass + finish pass)
  step_logits     MeanIoU._after_step_logits on the head's [N,18] logits (the labels are never written)
  labels+step     occupancy_labels (gf_head_labels) followed by _after_step
  step_dict       _after_step in the dict form on the same frame as a [200,200,16] grid: uint8 ``semantics`` and ``mask_camera``
                  (device tensors), remap, filter_minmax over 16 z slices, use_mask
  torch_loop      a torch restatement of the reference's loop (misc/metric_util.py:53-66) WITH its 51 ``.item()`` round trips
                  and its float32 totals: the baseline, not the code under test; eager only -- a step that reads back cannot be
                  captured

Per path, eager and (native paths) replayed from a captured graph: µs per call as the median of the timed calls by HIP events
(each timed over --inner back-to-back calls), repeated --repeats times -- the row holds the median of those medians and
their spread (max - min); peak device memory above the inputs.  The native totals are checked against the loop's after one
frame.  Prints one JSON line per row and writes them to --out.  Needs an MI355X.

    python tools/bench_metric.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_anchor_embed import repeated  # noqa: E402
from bench_refine import captured, peak  # noqa: E402
from gaussianformer_amd.head import occupancy_labels  # noqa: E402
from gaussianformer_amd.metric import MeanIoU  # noqa: E402

CLASSES = list(range(1, 17))
NAMES = ['barrier', 'bicycle', 'bus', 'car', 'construction_vehicle', 'motorcycle', 'pedestrian', 'traffic_cone', 'trailer',
         'truck', 'driveable_surface', 'other_flat', 'sidewalk', 'terrain', 'manmade', 'vegetation']


class TorchLoop:
    """The reference's flat branch and per-class loop, restated: boolean-index compaction, three ``.item()`` per class and for
    the aggregate, float32 totals."""

    def __init__(self, dev):
        self.total_seen, self.total_correct, self.total_positive = (torch.zeros(17, device=dev) for _ in range(3))

    def step(self, outputs, targets, mask):
        outputs, targets = outputs[mask], targets[mask]
        for i, c in enumerate(CLASSES):
            self.total_seen[i] += torch.sum(targets == c).item()
            self.total_correct[i] += torch.sum((targets == c) & (outputs == c)).item()
            self.total_positive[i] += torch.sum(outputs == c).item()
        self.total_seen[-1] += torch.sum(targets != 17).item()
        self.total_correct[-1] += torch.sum((targets != 17) & (outputs != 17)).item()
        self.total_positive[-1] += torch.sum(outputs != 17).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_metric.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metric.py needs an MI355X")
    dev = torch.device("cuda:0")
    N = 200 * 200 * 16
    g = torch.Generator().manual_seed(0)
    occupied = torch.rand(N, generator=g) < 0.22
    gt = torch.where(occupied, torch.randint(0, 17, (N,), generator=g), torch.full((N,), 17))
    logits = torch.randn(N, 18, generator=g)
    logits[torch.arange(N), gt] += 3.0                      # a head that is right more often than not
    gt, logits = gt.to(dev), logits.to(dev)
    mask = (torch.rand(N, generator=g) < 0.35).to(dev)
    pred = occupancy_labels(logits)
    m = MeanIoU(CLASSES, 17, NAMES, True, 17, filter_minmax=False, device=dev)
    loop = TorchLoop(dev)

    # one frame through each path: the same totals
    loop.step(pred, gt, mask)
    want = torch.stack([loop.total_seen, loop.total_correct, loop.total_positive]).to(torch.int64)
    for step in (lambda: m._after_step(pred, gt, mask), lambda: m._after_step_logits(logits, gt, mask)):
        m.reset()
        step()
        assert torch.equal(m._totals, want), "the native step and the torch loop disagree"

    md = MeanIoU(CLASSES, 17, NAMES, True, 17, filter_minmax=True, device=dev)
    grid = {"semantics": gt.to(torch.uint8).view(200, 200, 16), "mask_camera": mask.to(torch.uint8).view(200, 200, 16)}
    paths = {"step": lambda: m._after_step(pred, gt, mask),
             "step_dict": lambda: md._after_step(pred, grid),
             "step_logits": lambda: m._after_step_logits(logits, gt, mask),
             "labels+step": lambda: m._after_step(occupancy_labels(logits), gt, mask),
             "torch_loop": lambda: loop.step(pred, gt, mask)}
    rows = []
    for path, fn in paths.items():
        for mode in (("eager",) if path == "torch_loop" else ("eager", "graph")):
            med, spread, least = repeated(fn if mode == "eager" else captured(fn), a)
            row = dict(path=path, mode=mode, N=N, kept_frac=round(float(mask.float().mean()), 3), us=round(med, 2),
                       spread_us=round(spread, 2), least_us=round(least, 2), steps=a.steps, inner=a.inner, repeats=a.repeats)
            if mode == "eager":
                row["peak_mib"] = round(peak(fn), 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    base = next(r for r in rows if r["path"] == "torch_loop")
    for r in rows:
        if r["path"] != "torch_loop":
            r["torch_loop_over_native"] = round(base["us"] / r["us"], 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
