"""TEST INFRASTRUCTURE shared by tests/test_head_module.py (CPU oracle) and tests/test_head_module_gpu.py: the fixtures the
drop-in ``GaussianHead`` is held to -- tests/golden/head_module.npz (tools/make_golden_head.py: the reference's module,
constructions and supervised layers) and the four tests/golden/caller_head_*.npz (tools/make_golden_callers.py: one
recorded call with its gradients) --, the tolerances of tests/test_ref_callers.py and the label judge.  Nothing here reads
the reference tree."""
import collections
import functools
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONSTRUCTIONS = ("base", "prob", "prob_geosem")
CALLER_CASES = ("base", "prob", "prob_geosem", "prob_fast")
LEAVES = ("means", "scales", "rotations", "opacities", "sem_raw")

# the fields of the reference's namedtuple (model/encoder/gaussian_encoder/utils.py), which the head reads by name
GaussianPrediction = collections.namedtuple("GaussianPrediction", "means scales rotations opacities semantics")


def out_tol(prob):
    """tests/test_ref_callers.py::test_head_fused_path_matches_the_reference_caller: the closed-form Sigma^-1 against the
    reference's fp32 LAPACK inverse (prob: through the determinant), relative to the largest magnitude."""
    return 2e-3 if prob else 1e-4


def grad_tol(prob):
    return 2e-2 if prob else 2e-3


def check(got, want, what, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-6)
    print(f"{what}: {err:.3e} of {tol}")
    assert np.isfinite(got).all() and err <= tol, f"{what}: {err:.3e} > {tol}"


def decisive(pred, tol, bins=None, threshold=0.5):
    """Which voxels of a FIXTURE's ``pred [18,N]`` (and ``bins [N]`` for the threshold head) have a decision that outputs
    within ``tol`` (relative to the largest magnitude) cannot move: the top-two margin exceeds 2 tol max|pred|, and for the
    threshold head |bin - threshold| exceeds 2 tol max|bin|."""
    top = np.sort(np.asarray(pred, np.float64), axis=0)
    ok = (top[-1] - top[-2]) > 2 * tol * np.abs(pred).max()
    if bins is not None:
        ok &= np.abs(np.asarray(bins, np.float64) - threshold) > 2 * tol * np.abs(bins).max()
    return ok


def check_labels(got, want, pred, tol, what, bins=None, threshold=0.5):
    """``got`` against the fixture's ``want`` on the decisive voxels, of which there must be at least 90 %."""
    ok = decisive(pred, tol, bins, threshold)
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1).astype(np.int64)
    assert got.shape == want.shape == ok.shape, (what, got.shape, want.shape, ok.shape)
    print(f"{what}: {100 * ok.mean():.1f} % of the voxels judged")
    assert ok.mean() >= 0.9, f"{what}: only {100 * ok.mean():.1f} % judged"
    assert np.array_equal(got[ok], want[ok]), f"{what}: {(got[ok] != want[ok]).sum()} decisive voxels differ"


# ---------------------------------------------------------------------------------------------- head_module.npz
@functools.lru_cache(maxsize=None)
def module_fixture():
    d = np.load(os.path.join(GOLDEN, "head_module.npz"))
    return {k: d[k] for k in d.files}


def module_kwargs(name):
    return json.loads(str(module_fixture()[f"{name}_head_kwargs"]))


def module_cases(name):
    """``(case, apply_loss_type, numpy seed, train mode, forward keywords)`` of a construction."""
    return [tuple(c) for c in json.loads(str(module_fixture()[f"{name}_cases"]))]


def module_inputs(name, device):
    """``(representation, metas)`` of a construction: its three decoder layers and the 8 x 8 x 8 voxel centres."""
    d = module_fixture()
    rep = [dict(gaussian=GaussianPrediction(*[torch.from_numpy(d[f"{name}_in_{k}"][i]).to(device) for k in GaussianPrediction._fields]))
           for i in range(d[f"{name}_in_means"].shape[0])]
    H, W, D, gs = int(d["grid_H"]), int(d["grid_W"]), int(d["grid_D"]), np.float32(d["grid_grid_size"])
    ax = [(np.arange(n, dtype=np.float32) + np.float32(0.5)) * gs + np.float32(o) for n, o in zip((H, W, D), d["grid_pc_min"])]
    xyz = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)[None].astype(np.float32)
    metas = dict(occ_xyz=torch.from_numpy(xyz), occ_label=torch.zeros(1, H, W, D, dtype=torch.int64),
                 occ_cam_mask=torch.ones(1, H, W, D, dtype=torch.bool))
    return rep, metas


def check_module_case(head, name, case, out, threshold=0.5):
    """The output dict of one case against the fixture: keys, containers, shapes, entries, labels."""
    d = module_fixture()
    prob = name != "base"
    tol = out_tol(prob)
    layers = d[f"{name}_{case}_layers"].tolist()
    assert list(out) == d[f"{name}_out_keys"].tolist()
    assert isinstance(out["pred_occ"], list) and len(out["pred_occ"]) == len(layers), (len(out["pred_occ"]), layers)
    N = d[f"{name}_layer_pred"].shape[-1]
    for i, (p, layer) in enumerate(zip(out["pred_occ"], layers)):
        assert p.shape == (1, 18, N) and p.dtype == torch.float32 and p.transpose(1, 2).is_contiguous()
        check(p.detach().cpu(), d[f"{name}_layer_pred"][layer], f"{name} {case} pred_occ[{i}]", tol)
    for key, fix in (("bin_logits", "bin"), ("density", "density")):
        assert isinstance(out[key], list) and len(out[key]) == (len(layers) if prob else 0)
        for i, (b, layer) in enumerate(zip(out[key], layers)):
            assert b.shape == (1, N)
            check(b.detach().cpu(), d[f"{name}_layer_{fix}"][layer], f"{name} {case} {key}[{i}]", tol)
    final = out["final_occ"]
    assert final.shape == (1, N) and final.dtype == torch.int64
    threshold_head = prob and not head.combine_geosem
    check_labels(final.cpu().numpy(), d[f"{name}_{case}_final_occ"], d[f"{name}_layer_pred"][layers[-1]][0], tol,
                 f"{name} {case} final_occ", d[f"{name}_layer_bin"][layers[-1]][0] if threshold_head else None, threshold)
    assert out["sampled_xyz"].shape == (1, N, 3) and out["sampled_label"].shape == (1, N) and out["occ_mask"].shape[0] == 1
    assert len(out["gaussians"]) == d[f"{name}_in_means"].shape[0] and out["gaussian"] is out["gaussians"][-1]


# ---------------------------------------------------------------------------------------------- caller_head_*.npz
@functools.lru_cache(maxsize=None)
def caller_fixture(name):
    d = np.load(os.path.join(GOLDEN, f"caller_head_{name}.npz"))
    return {k: d[k] for k in d.files}


def caller_kwargs(name):
    """The matching ``head_kwargs`` of tests/golden/caller_construct.json, plus ``combine_geosem`` for ``prob_geosem``, with the
    ``cuda_kwargs`` the CALL was recorded with (the fixture's ``grid_*``; tests/test_ref_callers.py ``_cuda_kwargs``): the json's
    prob_fast head was constructed with ``radii_min=2``, the recorded prob_fast call with the default."""
    with open(os.path.join(GOLDEN, "caller_construct.json")) as f:
        heads = json.load(f)["heads"]
    kw = dict(heads[{"base": 0, "prob": 1, "prob_geosem": 1, "prob_fast": 2}[name]]["head_kwargs"])
    if name == "prob_geosem":
        kw["combine_geosem"] = True
    d = caller_fixture(name)
    kw["cuda_kwargs"] = dict(scale_multiplier=3 if name == "base" else 4, H=int(d["grid_H"]), W=int(d["grid_W"]), D=int(d["grid_D"]),
                             pc_min=[float(v) for v in d["grid_pc_min"]], grid_size=float(d["grid_grid_size"]))
    return kw


def caller_leaves(name, device):
    d = caller_fixture(name)
    return {k: torch.from_numpy(d[k]).to(device).requires_grad_(True) for k in LEAVES}


def caller_call(head, name, leaves, device):
    """The recorded call through ``head``: one decoder layer (softplus of ``sem_raw`` as its semantics), the output dict and
    the fixture's scalar loss."""
    d = caller_fixture(name)
    t = lambda k: torch.from_numpy(d[k]).to(device)
    g = GaussianPrediction(leaves["means"], leaves["scales"], leaves["rotations"], leaves["opacities"],
                           torch.nn.functional.softplus(leaves["sem_raw"]))
    xyz = t("occ_xyz")
    metas = dict(occ_xyz=xyz, occ_label=torch.zeros(xyz.shape[:4], dtype=torch.int64), occ_cam_mask=torch.ones(xyz.shape[:4], dtype=torch.bool))
    out = head([dict(gaussian=g)], metas)
    loss = (out["pred_occ"][-1] * t("pred_weight")).sum()
    if name != "base":
        loss = loss + (out["bin_logits"][-1] * t("bin_weight")).sum() + (out["density"][-1] * t("density_weight")).sum()
    return out, loss


def check_caller(head, name, out, leaves, what):
    """Outputs, labels and (after ``loss.backward()``) every gradient against the fixture."""
    d = caller_fixture(name)
    prob = name != "base"
    tol, gtol = out_tol(prob), grad_tol(prob)
    assert len(out["pred_occ"]) == 1
    check(out["pred_occ"][-1].detach().cpu(), d["pred_occ"], f"{what} pred_occ", tol)
    if prob:
        check(out["bin_logits"][-1].detach().cpu(), d["bin_logits"], f"{what} bin_logits", tol)
        check(out["density"][-1].detach().cpu(), d["density"], f"{what} density", tol)
    else:
        assert out["bin_logits"] == [] and out["density"] == []
    check_labels(out["final_occ"].cpu().numpy(), d["final_occ"], d["pred_occ"][0], tol, f"{what} final_occ",
                 d["bin_logits"][0] if name in ("prob", "prob_fast") else None)
    for k in LEAVES:
        check(leaves[k].grad.cpu(), d["grad_" + k], f"{what} grad_{k}", gtol)
    if not prob:
        check(head.empty_scalar.grad.cpu(), d["grad_empty_scalar"], f"{what} grad_empty_scalar", gtol)
