"""Generates the two fixtures that let tests/test_ref_callers.py's CPU tests run without the reference tree:

* tests/golden/caller_construct.json -- what the REFERENCE's ``GaussianHead.__init__`` (model/head/gaussian_head.py:29-39)
  builds on the drop-ins from config-shaped kwargs: which drop-in package's ``LocalAggregator`` it took, with which
  ``cuda_kwargs``, and the ``aggregator.*`` entries of the head's state dict (eval.py:108 loads checkpoints with
  strict=True); and what ``DeformableFeatureAggregation`` built through the registry with ``use_deformable_func``.
* tests/golden/caller_kps_activations.npz -- the reference's ``SparseGaussian3DKeyPointsGenerator`` (float64) under the
  four activation switches (deformable_module.py:27-28, :66-67, :79-80): inputs, the layer's parameters, outputs.

The reference's caller code is imported unmodified through tests/ref_shim.py (build container only; needs the reference
tree at GF_REFERENCE_ROOT, no GPU).

Run:  python tools/make_golden_caller_facts.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
PACKAGES = ("local_aggregate", "local_aggregate_prob", "local_aggregate_prob_fast")
# the cuda_kwargs of config/nuscenes_gs25600_solid.py:174-191 and config/prob/nuscenes_gs6400.py on the reduced grid of
# the caller_head_*.npz fixtures
GRID = dict(H=16, W=16, D=8, pc_min=[-4.0, -4.0, -2.0], grid_size=0.5)
HEADS = [
    dict(apply_loss_type="random_1", num_classes=18, with_empty=True, empty_args=dict(mean=[0, 0, -1.0], scale=[100, 100, 8.0]),
         cuda_kwargs=dict(scale_multiplier=3, **GRID)),
    dict(apply_loss_type="all", use_localaggprob=True, cuda_kwargs=dict(scale_multiplier=4, **GRID)),
    dict(apply_loss_type="fixed_0", use_localaggprob=True, use_localaggprob_fast=True,
         cuda_kwargs=dict(radii_min=2, scale_multiplier=4, **GRID)),
]
DFA = dict(type="DeformableFeatureAggregation", embed_dims=32, num_groups=4, num_levels=3, num_cams=3, use_deformable_func=True,
           use_camera_embed=True, residual_mode="cat",
           kps_generator=dict(type="SparseGaussian3DKeyPointsGenerator", num_learnable_pts=2, fix_scale=[[0, 0, 0]],
                              pc_range=[-1, -1, -1, 1, 1, 1], scale_range=[0.1, 0.6]))
KPS_FIX = [[0, 0, 0], [0.45, 0, 0], [-0.45, 0, 0], [0, 0.45, 0], [0, -0.45, 0], [0, 0, 0.45], [0, 0, -0.45]]
KPS_PC_RANGE, KPS_SCALE_RANGE = [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0], [0.08, 0.64]
KPS_ACTIVATIONS = [("sigmoid", "sigmoid"), ("identity", "sigmoid"), ("sigmoid", "none"), ("identity", "identity")]


def construct_facts(ref):
    import importlib
    heads = []
    for kw in HEADS:
        head = ref.GaussianHead(**kw)
        pkg = [p for p in PACKAGES if type(head.aggregator) is importlib.import_module(p).LocalAggregator]
        assert len(pkg) == 1, pkg
        state = {k: {"shape": list(v.shape), "values": v.flatten().tolist()}
                 for k, v in head.state_dict().items() if k.startswith("aggregator.")}
        heads.append(dict(head_kwargs=kw, aggregator_package=pkg[0], aggregator_kwargs=kw["cuda_kwargs"], state_dict=state,
                          radii_min=getattr(head.aggregator, "radii_min", None)))
    dfa = ref_shim.build_from_cfg(DFA, ref_shim.MODELS)
    from model.encoder.gaussian_encoder.ops import DeformableAggregationFunction
    assert ref.DAF is DeformableAggregationFunction
    facts = dict(producer="tools/make_golden_caller_facts.py: the reference's GaussianHead / DeformableFeatureAggregation "
                          "constructors on the drop-ins",
                 heads=heads, dfa=dict(config=DFA, use_deformable_func=bool(dfa.use_deformable_func), num_pts=int(dfa.num_pts),
                                       op_module="model.encoder.gaussian_encoder.ops"))
    with open(os.path.join(OUT, "caller_construct.json"), "w") as f:
        json.dump(facts, f, indent=1)
        f.write("\n")


def kps_activation_facts():
    g = torch.Generator().manual_seed(11)
    anchor = torch.randn(2, 50, 12, generator=g, dtype=torch.float64)
    feat = torch.randn(2, 50, 16, generator=g, dtype=torch.float64)
    d = dict(producer=np.array("tools/make_golden_caller_facts.py: the reference's SparseGaussian3DKeyPointsGenerator, float64"),
             anchor=anchor.numpy(), instance_feature=feat.numpy(), fix_scale=np.array(KPS_FIX, np.float64),
             pc_range=np.array(KPS_PC_RANGE), scale_range=np.array(KPS_SCALE_RANGE))
    for xyz_act, scale_act in KPS_ACTIVATIONS:
        torch.manual_seed(0)
        gen = ref_shim.build_from_cfg(dict(type="SparseGaussian3DKeyPointsGenerator", embed_dims=16, num_learnable_pts=2,
                                           fix_scale=KPS_FIX, pc_range=KPS_PC_RANGE, scale_range=KPS_SCALE_RANGE,
                                           xyz_activation=xyz_act, scale_activation=scale_act), ref_shim.MODELS).double()
        key = f"{xyz_act}_{scale_act}"
        d[f"{key}_weight"] = gen.learnable_fc.weight.detach().numpy()
        d[f"{key}_bias"] = gen.learnable_fc.bias.detach().numpy()
        d[f"{key}_key_points"] = gen(anchor, feat).detach().numpy()
    np.savez_compressed(os.path.join(OUT, "caller_kps_activations.npz"), **d)


if __name__ == "__main__":
    if not ref_shim.available():
        sys.exit(f"reference tree not found at {ref_shim.REFERENCE}")
    reference = ref_shim.load_reference()
    construct_facts(reference)
    kps_activation_facts()
    print("wrote", os.path.join(OUT, "caller_construct.json"), "and", os.path.join(OUT, "caller_kps_activations.npz"))
