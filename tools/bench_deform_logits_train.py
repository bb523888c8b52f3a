#!/usr/bin/env python
"""The training step of the deformable block's dense front, forward + backward, at the shipped shapes --
prob (3K = 18, Nw = 208) at A = 6 400 and 25 600, solid (6, 144) at A = 25 600 and 144 000, and the prob width without the camera
embedding (18, 1 248) at A = 25 600:

  op       ``deformable_logits_autograd`` (gf_deform_logits_forward + gf_deform_logits_backward) against the torch composition:
           the add and two ``F.linear`` under autograd
  module   ``DeformableFeatureAggregation`` with ``native_front_training`` True against the SAME module with the attribute False
           (the yardstick: the parent's route)

One step = the forward, the scalar ``sum(raw * w) + sum(learned * w)`` (the module: ``sum(out * w)``) and ``torch.autograd.grad``
of it for the inputs and every parameter.  The two sides ALTERNATE in one process: --repeats rounds, each timing first one side,
then the other (the median of --steps timings by HIP events, each over --inner back-to-back steps), eager and replayed from a
captured graph; a row holds the median of those medians, their spread (max - min), the least single timing and the peak device
memory of one step above the inputs and the weights.  The statement a pair makes or withholds: "faster than the torch side by
more than BOTH spreads".  There is no threshold: the attribute is opt-in.  Writes one JSON line per row to
profiles/bench_deform_logits_train.jsonl.  Needs an MI355X.

    python tools/bench_deform_logits_train.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--part op|module] [--shape I]
                                              [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deform_block_ref as ref  # noqa: E402
from bench_deform_block import CAMS, cameras  # noqa: E402
from bench_refine import captured, peak, timed  # noqa: E402
from gaussianformer_amd import synthetic  # noqa: E402
from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF  # noqa: E402
from gaussianformer_amd.deformable_block import DeformableFeatureAggregation, deformable_logits_autograd  # noqa: E402

BENCH = "deform_logits_train"
# family: (num_learnable_pts, residual_mode, the encoder's add and norm behind the block, use_camera_embed)
FAMILIES = {"prob": (6, "none", True, True), "solid": (2, "cat", False, True), "nocam": (6, "none", True, False)}
SHAPES = [("prob", 6400), ("prob", 25600), ("solid", 25600), ("solid", 144000), ("nocam", 25600)]


def compare(a, sides, **labels):
    """The rows of one pair ``{native label: step, torch label: step}`` (the native side first), and the row that compares them."""
    rows = {path: dict(bench=BENCH, path=path, **labels) for path in sides}
    for timing in ("eager", "graph"):
        fns = {path: fn if timing == "eager" else captured(fn) for path, fn in sides.items()}
        meds, least = {path: [] for path in sides}, {path: float("inf") for path in sides}
        for _ in range(a.repeats):                  # the sides alternate: a drift of the clocks meets both
            for path, fn in fns.items():
                med, low = timed(fn, a.steps, a.warmup, a.inner)
                meds[path].append(med)
                least[path] = min(least[path], low)
        for path, m in meds.items():
            rows[path].update({f"step_us_{timing}": round(statistics.median(m), 2), f"step_us_{timing}_spread": round(max(m) - min(m), 2),
                               f"step_us_{timing}_min": round(least[path], 2)})
        del fns
    for path, fn in sides.items():
        rows[path]["peak_step_mib"] = round(peak(fn), 2)
        print(json.dumps(rows[path]), flush=True)
        torch.cuda.empty_cache()
    nat, base = rows.values()
    ratio = dict(bench=BENCH, path=f"speedup_{nat['path']}_over_{base['path']}", **labels)
    for timing in ("eager", "graph"):
        k = f"step_us_{timing}"
        spread = max(base[k + "_spread"], nat[k + "_spread"])
        ratio.update({k: round(base[k] / nat[k], 3), f"{timing}_faster_by_more_than_both_spreads": bool(base[k] - nat[k] > spread),
                      f"{timing}_slower_by_more_than_both_spreads": bool(nat[k] - base[k] > spread)})
    ratio["peak_mib_torch_over_native"] = round(base["peak_step_mib"] / max(nat["peak_step_mib"], 1e-9), 2)
    print(json.dumps(ratio), flush=True)
    return [nat, base, ratio]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--part", choices=("op", "module"), default=None, help="that part alone")
    ap.add_argument("--shape", type=int, default=None, help="index into the shapes: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_deform_logits_train.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    table = DAF.feature_maps_format([torch.randn(1, CAMS, 128, h, w, generator=g).to(dev) for h, w in synthetic.DAF_LEVELS])
    pm, wh = cameras(dev)
    metas = dict(projection_mat=pm, image_wh=wh)
    rows = []
    for family, A in (SHAPES if a.shape is None else SHAPES[a.shape:a.shape + 1]):
        learnable, mode, post, cam = FAMILIES[family]
        cfg = dict(embed_dims=128, num_groups=4, num_levels=4, num_cams=CAMS, use_deformable_func=True, use_camera_embed=cam, residual_mode=mode,
                   kps_generator=dict(num_learnable_pts=learnable, fix_scale=ref.FIX7, pc_range=[-50.0, -50.0, -5.0, 50.0, 50.0, 3.0],
                                      scale_range=[0.08, 0.64]))
        sd = ref.fixed_weights(ref.shapes(cfg, norm=True))
        module = DeformableFeatureAggregation(**cfg)
        module.load_state_dict(ref.module_state(sd), strict=True)
        module.to(dev).eval()                       # (eval keeps both sides deterministic; the front's route does not ask for the mode)
        norm = torch.nn.LayerNorm(128)
        norm.load_state_dict({"weight": sd["norm.weight"], "bias": sd["norm.bias"]})
        norm.to(dev)
        anchor = torch.randn(1, A, 28, generator=g)
        anchor[..., :3] *= 1.5
        anchor = anchor.to(dev)
        inst, emb = (torch.randn(1, A, 128, generator=g).to(dev).requires_grad_(True) for _ in range(2))
        wfc, lfc = module.weights_fc, module.kps_generator.learnable_fc
        Nw, K3 = wfc.weight.shape[0], lfc.weight.shape[0]
        cot_raw, cot_learned = torch.randn(1, A, Nw, generator=g).to(dev), torch.randn(1, A, K3, generator=g).to(dev)
        cot = torch.randn(1, A, 256 if mode == "cat" else 128, generator=g).to(dev)
        kw = dict(residual=inst, norm=norm) if post else {}
        front = [inst, emb, wfc.weight, wfc.bias, lfc.weight, lfc.bias]

        def op_native():
            raw, learned = deformable_logits_autograd(inst, emb, wfc, lfc)
            torch.autograd.grad((raw * cot_raw).sum() + (learned.flatten(-2) * cot_learned).sum(), front)

        def op_torch():
            raw, learned = F.linear(inst + emb, wfc.weight, wfc.bias), F.linear(inst, lfc.weight, lfc.bias)
            torch.autograd.grad((raw * cot_raw).sum() + (learned * cot_learned).sum(), front)

        def block(native):
            leaves = [inst, emb, *module.parameters()] + (list(norm.parameters()) if post else [])

            def run():
                module.native_front_training = native
                out = module(inst, anchor, emb, table, metas, **kw)
                torch.autograd.grad((out * cot).sum(), leaves)
            return run
        labels = dict(family=family, A=A, K3=K3, Nw=Nw)
        if a.part in (None, "op"):
            rows += compare(a, {"native_op": op_native, "torch_composition": op_torch}, what="op", **labels)
        if a.part in (None, "module"):
            rows += compare(a, {"native_front_training": block(True), "torch_front": block(False)}, what="module", **labels)
        vars(module).pop("native_front_training", None)      # (back to the class attribute)
        del module
        torch.cuda.empty_cache()
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
