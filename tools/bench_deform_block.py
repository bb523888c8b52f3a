#!/usr/bin/env python
"""The deformable block under ``no_grad``: the drop-in ``DeformableFeatureAggregation`` (gaussianformer_amd.deformable_block)
with its dense ends native (``native_dense = True``: ``deformable_logits`` -> ``key_points`` -> ``deformable_fused_forward`` ->
``deformable_output``, four launches) against the SAME module with ``native_dense = False`` (its torch layers around the same
native middle: what every hand-assembled block ran before), on the same GPU, weights and formatted feature table:

  solid (pts = 9,  residual_mode "cat")                                          at A = 25 600, 144 000
  prob  (pts = 13, residual_mode "none", then the encoder's "add", "norm")       at A = 6 400, 25 600

and the two dense kernels alone against their torch compositions: the add, two GEMMs and biases for the front; the GEMM, bias
and cat / add + LayerNorm for the back.  Per shape and path, eager and replayed from a captured graph: µs as the median of the
timed calls by HIP events (each call timed over --inner back-to-back runs), repeated --repeats times -- the row holds the
median of those medians and their spread (max - min), and "faster" means by more than the baseline's spread; and the peak
device memory above the inputs and the weights.  Writes one JSON line per row to profiles/bench_deform_block.jsonl.  Needs an
MI355X.

    python tools/bench_deform_block.py [--steps K] [--warmup W] [--inner N] [--repeats R] [--shape I] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deform_block_ref as ref  # noqa: E402
from bench_anchor_embed import repeated  # noqa: E402
from bench_refine import captured, peak  # noqa: E402
from gaussianformer_amd import synthetic  # noqa: E402
from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF  # noqa: E402
from gaussianformer_amd.deformable_block import DeformableFeatureAggregation, deformable_logits, deformable_output  # noqa: E402

SHAPES = [("solid", 25600), ("solid", 144000), ("prob", 6400), ("prob", 25600)]
FAMILIES = {"solid": dict(num_learnable_pts=2, residual_mode="cat", post=False), "prob": dict(num_learnable_pts=6, residual_mode="none", post=True)}
CAMS = 6


def cameras(dev, wh=(1600.0, 864.0)):
    """A ring of pinhole cameras looking outwards (tools/bench_frame.py's)."""
    pm = torch.eye(4).repeat(1, CAMS, 1, 1)
    K = torch.tensor([[1260.0, 0, wh[0] / 2], [0, 1260.0, wh[1] / 2], [0, 0, 1.0]])
    for c in range(CAMS):
        yaw = 2 * np.pi * c / CAMS
        R = torch.tensor([[-np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, -1.0], [np.cos(yaw), np.sin(yaw), 0.0]], dtype=torch.float32)
        pm[0, c, :3, :3] = K @ R
        pm[0, c, :3, 3] = K @ torch.tensor([0.0, 1.5, 0.0])
    return pm.to(dev), torch.tensor([[list(wh)] * CAMS], device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_deform_block.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    table = DAF.feature_maps_format([torch.randn(1, CAMS, 128, h, w, generator=g).to(dev) for h, w in synthetic.DAF_LEVELS])
    pm, wh = cameras(dev)
    metas = dict(projection_mat=pm, image_wh=wh)
    rows = []
    for family, A in (SHAPES if a.shape is None else SHAPES[a.shape:a.shape + 1]):
        fam = FAMILIES[family]
        cfg = dict(embed_dims=128, num_groups=4, num_levels=4, num_cams=CAMS, use_deformable_func=True, use_camera_embed=True,
                   residual_mode=fam["residual_mode"],
                   kps_generator=dict(num_learnable_pts=fam["num_learnable_pts"], fix_scale=ref.FIX7, pc_range=[-50.0, -50.0, -5.0, 50.0, 50.0, 3.0],
                                      scale_range=[0.08, 0.64]))
        sd = ref.fixed_weights(ref.shapes(cfg, norm=True))
        module = DeformableFeatureAggregation(**cfg)
        module.load_state_dict(ref.module_state(sd), strict=True)
        module.to(dev).eval()
        norm = torch.nn.LayerNorm(128)
        norm.load_state_dict({"weight": sd["norm.weight"], "bias": sd["norm.bias"]})
        norm.to(dev)
        anchor = torch.randn(1, A, 28, generator=g)
        anchor[..., :3] *= 1.5
        anchor = anchor.to(dev)
        inst, emb, feats = (torch.randn(1, A, 128, generator=g).to(dev) for _ in range(3))
        post = dict(residual=inst, norm=norm) if fam["post"] else {}
        gen, mode = module.kps_generator, fam["residual_mode"]

        def block(native):
            def run():
                module.native_dense = native
                return module(inst, anchor, emb, table, metas, **post)
            return run

        def front_torch():
            return module.weights_fc(inst + emb), gen.learnable_fc(inst)

        def back_torch():
            y = module.output_proj(feats)
            return torch.cat([y, inst], dim=-1) if mode == "cat" else norm(y + inst)
        ops = [("block", "native", block(True)), ("block", "torch_dense", block(False)),
               ("front", "native", lambda: deformable_logits(inst, emb, module.weights_fc, gen.learnable_fc)), ("front", "torch_dense", front_torch),
               ("back", "native", lambda: deformable_output(feats, module.output_proj, inst, mode, **post)), ("back", "torch_dense", back_torch)]
        for what, path, op in ops:
            def fwd():
                with torch.no_grad():
                    op()

            row = dict(bench="deform_block", family=family, pts=module.num_pts, Nw=module.weights_fc.out_features, A=A, what=what, path=path)
            for timing in ("eager", "graph"):
                med, spread, least = repeated(fwd if timing == "eager" else captured(fwd), a)
                row.update({f"fwd_us_{timing}": round(med, 2), f"fwd_us_{timing}_spread": round(spread, 2), f"fwd_us_{timing}_min": round(least, 2)})
            row.update(peak_fwd_mib=round(peak(fwd), 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        module.native_dense = True
    for nat, base in zip(rows[0::2], rows[1::2]):
        row = dict(bench="deform_block", family=nat["family"], A=nat["A"], what=nat["what"], path="speedup_native_over_torch_dense")
        for timing in ("eager", "graph"):
            k = f"fwd_us_{timing}"
            row[k] = round(base[k] / nat[k], 2)
            row[f"{timing}_faster_by_more_than_baseline_spread"] = bool(base[k] - nat[k] > base[k + "_spread"])
            row[f"{timing}_slower_by_more_than_spread"] = bool(nat[k] - base[k] > max(base[k + "_spread"], nat[k + "_spread"]))
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
