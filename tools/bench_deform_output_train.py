#!/usr/bin/env python
"""The training step of the deformable block's dense back, forward + backward, at the shipped shapes --
prob ("none" + residual + norm) at A = 6 400 and 25 600, solid ("cat") at A = 25 600 and 144 000:

  op       ``deformable_output_autograd`` (gf_deform_output_forward_train + gf_deform_output_backward) against the torch
           composition: nn.Linear, the add or the cat, nn.LayerNorm under autograd
  module   ``DeformableFeatureAggregation`` with ``native_training`` True against the SAME module with the attribute False
  encoder  one prob decoder block of ``GaussianOccEncoder`` in train mode with ``set_native(training=True)``,
           ``fold_training`` True against False (A = 6 400 and 25 600)

One step = the forward, the scalar ``sum(out * w)`` and ``torch.autograd.grad`` of it for the inputs and every parameter.  The
two sides ALTERNATE in one process: --repeats rounds, each timing first one side, then the other (the median of --steps timings
by HIP events, each over --inner back-to-back steps), eager and replayed from a captured graph (the encoder block: eager
only); a row holds the median of those
medians, their spread (max - min), the least single timing and the peak device memory of one step above the inputs and the
weights.  The statement a pair makes or withholds: "faster than the torch side by more than BOTH spreads".  There is no
threshold: all three attributes are opt-in.  Writes one JSON line per row to profiles/bench_deform_output_train.jsonl.  Needs an
MI355X.

    python tools/bench_deform_output_train.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--part op|module|encoder]
                                              [--shape I] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deform_block_ref as ref  # noqa: E402
from bench_deform_block import CAMS, FAMILIES, cameras  # noqa: E402
from bench_refine import captured, peak, timed  # noqa: E402
from gaussianformer_amd import GaussianOccEncoder, synthetic  # noqa: E402
from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF  # noqa: E402
from gaussianformer_amd.deformable_block import DeformableFeatureAggregation, deformable_output_autograd  # noqa: E402

SHAPES = [("prob", 6400), ("prob", 25600), ("solid", 25600), ("solid", 144000)]
ENCODER_SHAPES = [("prob/nuscenes_gs6400", 6400, 64), ("prob/nuscenes_gs25600", 25600, 64)]      # (family, anchors, pairs_per_point)


def compare(a, sides, timings=("eager", "graph"), **labels):
    """The rows of one pair ``{native label: step, torch label: step}`` (the native side first), and the row that compares them."""
    rows = {path: dict(bench="deform_output_train", path=path, **labels) for path in sides}
    for timing in timings:
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
    ratio = dict(bench="deform_output_train", path=f"speedup_{nat['path']}_over_{base['path']}", **labels)
    for timing in timings:
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
    ap.add_argument("--part", choices=("op", "module", "encoder"), default=None, help="that part alone")
    ap.add_argument("--shape", type=int, default=None, help="index into the part's shapes: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_deform_output_train.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    table = DAF.feature_maps_format([torch.randn(1, CAMS, 128, h, w, generator=g).to(dev) for h, w in synthetic.DAF_LEVELS])
    pm, wh = cameras(dev)
    metas = dict(projection_mat=pm, image_wh=wh)
    pick = lambda shapes: shapes if a.shape is None else shapes[a.shape:a.shape + 1]
    rows = []
    for family, A in (pick(SHAPES) if a.part in (None, "op", "module") else []):
        fam = FAMILIES[family]
        mode = fam["residual_mode"]
        cfg = dict(embed_dims=128, num_groups=4, num_levels=4, num_cams=CAMS, use_deformable_func=True, use_camera_embed=True, residual_mode=mode,
                   kps_generator=dict(num_learnable_pts=fam["num_learnable_pts"], fix_scale=ref.FIX7, pc_range=[-50.0, -50.0, -5.0, 50.0, 50.0, 3.0],
                                      scale_range=[0.08, 0.64]))
        sd = ref.fixed_weights(ref.shapes(cfg, norm=True))
        module = DeformableFeatureAggregation(**cfg)
        module.load_state_dict(ref.module_state(sd), strict=True)
        module.to(dev).eval()                       # (attn_drop is not a constructor default here; eval keeps both sides deterministic)
        norm = torch.nn.LayerNorm(128)
        norm.load_state_dict({"weight": sd["norm.weight"], "bias": sd["norm.bias"]})
        norm.to(dev)
        anchor = torch.randn(1, A, 28, generator=g)
        anchor[..., :3] *= 1.5
        anchor = anchor.to(dev)
        inst, emb, feats = (torch.randn(1, A, 128, generator=g).to(dev).requires_grad_(True) for _ in range(3))
        width = 256 if mode == "cat" else 128
        cot = torch.randn(1, A, width, generator=g).to(dev)
        post = dict(residual=inst, norm=norm) if fam["post"] else {}
        tail = [module.output_proj.weight, module.output_proj.bias] + (list(norm.parameters()) if fam["post"] else [])

        def op_native():
            out = deformable_output_autograd(feats, module.output_proj, inst, mode, **post)
            torch.autograd.grad((out * cot).sum(), [feats, inst] + tail)

        def op_torch():
            y = module.output_proj(feats)
            out = torch.cat([y, inst], dim=-1) if mode == "cat" else norm(y + inst)
            torch.autograd.grad((out * cot).sum(), [feats, inst] + tail)

        def block(native):
            leaves = [inst, emb, *module.parameters()] + (list(norm.parameters()) if fam["post"] else [])

            def run():
                module.native_training = native
                out = module(inst, anchor, emb, table, metas, **post)
                torch.autograd.grad((out * cot).sum(), leaves)
            return run
        if a.part in (None, "op"):
            rows += compare(a, {"native_op": op_native, "torch_composition": op_torch}, what="op", family=family, A=A)
        if a.part in (None, "module"):
            rows += compare(a, {"native_training": block(True), "torch_tail": block(False)}, what="module", family=family, A=A)
        vars(module).pop("native_training", None)      # (back to the class attribute)
    if a.part in (None, "encoder"):
        with open(os.path.join(ROOT, "tests", "golden", "encoder_orders.json")) as f:
            recorded = json.load(f)
    for family, A, ppp in (pick(ENCODER_SHAPES) if a.part in (None, "encoder") else []):
        cfg = dict(recorded[family])
        cfg["operation_order"] = cfg["operation_order"][:17]          # one decoder block
        cfg["spconv_layer"] = dict(cfg["spconv_layer"], pairs_per_point=ppp)
        torch.manual_seed(0)
        enc = GaussianOccEncoder(**cfg)
        enc.init_weights()
        enc.to(dev).train()
        enc.set_native(training=True)
        dim = 10 + int(cfg["anchor_encoder"]["include_opa"]) + cfg["anchor_encoder"]["semantic_dim"]
        anchor = torch.randn(1, A, dim, generator=g)
        anchor[..., :3] *= 1.5
        anchor = anchor.to(dev)
        inst = torch.randn(1, A, 128, generator=g).to(dev).requires_grad_(True)
        leaves = [inst, *enc.parameters()]

        def frame(fold):
            def run():
                enc.set_native(fold_training=fold)
                preds = enc(anchor, inst, table, metas)["representation"]
                loss = sum(t.square().mean() for p in preds for t in p["gaussian"] if t is not None)
                torch.autograd.grad(loss, leaves, allow_unused=True)
            return run
        # (eager only: a whole training frame of the encoder is captured nowhere in the suite, so its replay is not timed here)
        rows += compare(a, {"fold_training": frame(True), "op_by_op": frame(False)}, timings=("eager",), what="encoder_block", family=family, A=A)
        del enc
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
