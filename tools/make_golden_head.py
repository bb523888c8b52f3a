"""Generates tests/golden/head_module.npz by executing the REFERENCE's own ``GaussianHead`` (model/head/gaussian_head.py:10-197),
unmodified, as a MODULE (build container only; needs the reference tree, no GPU): what its constructor registers and which
decoder layers its ``forward`` supervises, for the drop-in ``gaussianformer_amd.head.GaussianHead`` to be held to.

Like tools/make_golden_callers.py: mmengine / mmseg are the stand-ins of tests/ref_shim.py, ``import local_aggregate*``
resolves to the drop-in packages, whose raw kernel entry points are served by the CPU oracle (``ref_shim.cpu_kernels``), and
``Tensor.cuda()`` (gaussian_head.py:119) is an identity in this process.

Three constructions -- ``base`` (appended empty Gaussian), ``prob`` (threshold epilogue), ``prob_geosem`` -- on an 8 x 8 x 8
grid (N = 512) with three decoder layers of 24 different Gaussians each.  Per construction ``<c>``:

* ``<c>_head_kwargs``, ``<c>_cases``: the constructor keywords and the list of cases (case, apply_loss_type, numpy seed, train
  mode, forward keywords), as JSON;
* ``<c>_state_names`` and ``<c>_state_<name>``: the full state dict;  ``<c>_param_names``;  ``<c>_out_keys``: the output dict's keys;
* ``<c>_in_<field>``: ``[3, 1, g, k]`` the inputs of the three layers (means, scales, rotations, opacities, semantics);
* ``<c>_layer_pred`` ``[3, 1, 18, N]`` (and ``_layer_bin``, ``_layer_density`` ``[3, 1, N]``): what a layer's ``pred_occ`` entry
  is.  A layer's entry does not depend on which other layers are supervised, so every case below stores the LAYERS of its
  entries -- after this tool has compared each entry of each run with the layer's, bit for bit;
* per case ``<k>`` of ``CASES`` (``all``; ``random_2`` under three numpy seeds; ``fixed_0_2``; eval; for ``prob`` also eval with
  ``sigmoid_thresh = 0.4``): ``<c>_<k>_layers`` (one per ``pred_occ`` entry, in order) and ``<c>_<k>_final_occ`` ``[1, N]``.

Run:  python tools/make_golden_head.py
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

OUT = os.path.join(ROOT, "tests", "golden", "head_module.npz")
GRID = dict(H=8, W=8, D=8, pc_min=[-2.0, -2.0, -2.0], grid_size=0.5)
LAYERS, G = 3, 24
FIELDS = ("means", "scales", "rotations", "opacities", "semantics")
# (case, apply_loss_type, numpy seed, train mode, forward kwargs)
CASES = [("all", "all", 0, True, {}), ("random_2_seed0", "random_2", 0, True, {}), ("random_2_seed1", "random_2", 1, True, {}),
         ("random_2_seed5", "random_2", 5, True, {}), ("fixed_0_2", "fixed_0_2", 0, True, {}), ("eval", "random_2", 0, False, {})]
THRESH_CASE = ("eval_thresh", "random_2", 0, False, dict(sigmoid_thresh=0.4))
EMPTY_ARGS = dict(mean=[0, 0, -1.0], scale=[100, 100, 8.0])
CONSTRUCTIONS = {
    "base": (dict(num_classes=18, with_empty=True, empty_args=EMPTY_ARGS, cuda_kwargs=dict(scale_multiplier=3, **GRID)), (0.08, 0.64), 21, 60.0),   # (semantics that compete with the empty Gaussian's 10)
    "prob": (dict(num_classes=18, use_localaggprob=True, cuda_kwargs=dict(scale_multiplier=4, **GRID)), (0.05, 1.2), 22, 1.0),
    "prob_geosem": (dict(num_classes=18, use_localaggprob=True, combine_geosem=True, cuda_kwargs=dict(scale_multiplier=4, **GRID)),
                    (0.05, 1.2), 23, 1.0),
}


def voxel_centres():
    ax = [(np.arange(n, dtype=np.float32) + np.float32(0.5)) * np.float32(GRID["grid_size"]) + np.float32(o)
          for n, o in zip((GRID["H"], GRID["W"], GRID["D"]), GRID["pc_min"])]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)[None].astype(np.float32)      # [1,H,W,D,3]


def layer_inputs(rng, scale_range, sem_gain):
    lo = np.array(GRID["pc_min"])
    ext = np.array([GRID["H"], GRID["W"], GRID["D"]]) * GRID["grid_size"]
    rot = rng.standard_normal((1, G, 4))
    rot /= np.linalg.norm(rot, axis=-1, keepdims=True)
    sem = sem_gain * np.log1p(np.exp(rng.standard_normal((1, G, 17))))   # softplus, as the encoder hands them over
    f = dict(means=lo + (0.02 + 0.96 * rng.random((1, G, 3))) * ext,
             scales=scale_range[0] + (scale_range[1] - scale_range[0]) * rng.random((1, G, 3)),
             rotations=rot, opacities=rng.random((1, G, 1)), semantics=sem)
    return {k: v.astype(np.float32) for k, v in f.items()}


def construction(ref, name, head_kwargs, scale_range, seed, sem_gain, d):
    rng = np.random.default_rng(seed)
    layers = [layer_inputs(rng, scale_range, sem_gain) for _ in range(LAYERS)]
    rep = [dict(gaussian=ref.GaussianPrediction(**{k: torch.from_numpy(v) for k, v in f.items()})) for f in layers]
    metas = dict(occ_xyz=torch.from_numpy(voxel_centres()),
                 occ_label=torch.from_numpy(rng.integers(0, 18, (1, GRID["H"], GRID["W"], GRID["D"]))),
                 occ_cam_mask=torch.ones(1, GRID["H"], GRID["W"], GRID["D"], dtype=torch.bool))
    for k in FIELDS:
        d[f"{name}_in_{k}"] = np.stack([f[k] for f in layers])
    prob = bool(head_kwargs.get("use_localaggprob"))
    cases = CASES + ([THRESH_CASE] if prob and not head_kwargs.get("combine_geosem") else [])
    d[f"{name}_head_kwargs"] = np.array(json.dumps(head_kwargs))   # (without apply_loss_type: a case's)
    d[f"{name}_cases"] = np.array(json.dumps(cases))
    per_layer = None
    for case, apply_loss_type, np_seed, train, fwd_kwargs in cases:
        head = ref.GaussianHead(apply_loss_type=apply_loss_type, **head_kwargs)
        head.train(train)
        np.random.seed(np_seed)
        with ref_shim.cpu_kernels(), torch.no_grad():
            out = head(rep, metas, **fwd_kwargs)
        pred = [p.numpy() for p in out["pred_occ"]]
        if case == "all":
            assert len(pred) == LAYERS
            state = head.state_dict()
            d[f"{name}_state_names"] = np.array(sorted(state))
            for k, v in state.items():
                d[f"{name}_state_{k}"] = v.numpy()
            d[f"{name}_param_names"] = np.array([k for k, _ in head.named_parameters()])
            d[f"{name}_out_keys"] = np.array(list(out))
            per_layer = pred
            d[f"{name}_layer_pred"] = np.stack(pred)
            if prob:
                d[f"{name}_layer_bin"] = np.stack([b.numpy() for b in out["bin_logits"]])
                d[f"{name}_layer_density"] = np.stack([b.numpy() for b in out["density"]])
            else:
                assert out["bin_logits"] == [] and out["density"] == []
        # which layer each entry is: the one whose own entry it equals bit for bit (the three layers differ)
        which = []
        for p in pred:
            hits = [i for i, q in enumerate(per_layer) if np.array_equal(p.view(np.int32), q.view(np.int32))]
            assert len(hits) == 1, (name, case, hits)
            which.append(hits[0])
        if prob:
            for key in ("bin", "density"):
                got = out["bin_logits" if key == "bin" else key]
                assert len(got) == len(which) and all(np.array_equal(b.numpy(), d[f"{name}_layer_{key}"][i]) for b, i in zip(got, which))
        d[f"{name}_{case}_layers"] = np.array(which, dtype=np.int64)
        final = out["final_occ"].numpy()
        assert final.dtype == np.int64 and final.shape == (1, GRID["H"] * GRID["W"] * GRID["D"]) and final.min() >= 0 and final.max() < 18
        d[f"{name}_{case}_final_occ"] = final.astype(np.uint8)
        print(name, case, "layers", which, "labels used", len(np.unique(final)))
    assert all(np.isfinite(v).all() for k, v in d.items() if k.startswith(name) and v.dtype.kind == "f"), name


if __name__ == "__main__":
    assert ref_shim.available(), "needs the reference tree"
    torch.Tensor.cuda = lambda self, *a, **k: self      # gaussian_head.py:119 `.cpu().inverse().cuda()` on a CPU-only box
    ref = ref_shim.load_reference()
    d = dict(producer=np.array("tools/make_golden_head.py"), **{f"grid_{k}": np.array(v) for k, v in GRID.items()})
    for name, (head_kwargs, scale_range, seed, sem_gain) in CONSTRUCTIONS.items():
        construction(ref, name, head_kwargs, scale_range, seed, sem_gain, d)
    assert (d["prob_eval_thresh_final_occ"] != d["prob_eval_final_occ"]).any(), "the threshold case decides nothing"
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")
