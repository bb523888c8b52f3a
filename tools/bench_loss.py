#!/usr/bin/env python
"""The occupancy loss, forward + backward, at N = 640 000 voxels with labels drawn by the nuScenes class frequencies (about
78 % empty), for L = 1 and L = 4 layers, softmax mode (config/nuscenes_gs25600_solid.py's loss):

  native          gaussianformer_amd.occupancy_loss, lovasz_ignore = 17 (the shipped configs)
  torch           a torch restatement of the reference's loop (OccupancyLoss.loss_voxel + lovasz_softmax_flat): boolean
                  indexing, per class a host-synchronising ``fg.sum() == 0`` test, a sort, gathers, two cumsums and a dot,
                  and autograd backward
  native_all      the native op with lovasz_ignore = None: every kept voxel in every class's sort (the worst case)

Device time per call (CUDA events around each call, after warm-up; median and spread over the timed calls) and the loss
of each path.  Prints one JSON line per (path, L).  Needs an MI355X.

    python tools/bench_loss.py [--steps K] [--warmup W] [--n N] [--paths native,torch,native_all] [--layers 1,4]

``--scal``: the scene-class affinity terms (sem_scal / geo_scal, weights 1).  Forward + backward of

  scal            the native op with both terms
  base            the native op without them, this build
  parent          the same through another build of the library (``--parent-lib``: libgf_hip.so, or a library with the
                  occupancy-loss entry points alone, built from the parent commit)
  base+torch      ``base`` plus a torch restatement of the two terms (the reference's loop: three host synchronisations per
                  class and layer, the shift loops on a device scalar) -- what enabling the terms costs without the native ones

with the sides alternating in one process: ``--rounds`` rounds, in each the median of ``--steps`` calls per side; reported is
the median of these medians and their spread (min .. max).  The lines are appended to profiles/bench_loss_scal.jsonl.

    python tools/bench_loss.py --scal [--parent-lib PATH] [--rounds R] [--steps K] [--layers 1,4]
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianformer_amd import _lib  # noqa: E402
from gaussianformer_amd.occupancy_loss import occupancy_loss  # noqa: E402
from gaussianformer_amd.synthetic import make_occ_loss_inputs  # noqa: E402

MANUAL = [1.01552756, 1.06897009, 1.30013094, 1.07253735, 0.94637502, 1.10087012, 1.26960524, 1.06258364, 1.189019,
          1.06217292, 1.00595144, 0.85706115, 1.03923299, 0.90867526, 0.8936431, 0.85486129, 0.8527829, 0.5]


def torch_loss(pred_occ, label, mask, cw, ce_weight=10.0, lovasz_weight=1.0, lovasz_ignore=17):
    """The reference's computation for the softmax configs, restated with torch ops (per-class loop, host sync included)."""
    occ = mask.flatten(1)
    lab = label[occ][None]
    tot = 0.0
    for sem in pred_occ:
        sem = sem.transpose(1, 2)[occ][None].transpose(1, 2)
        ce = F.cross_entropy(sem, lab, weight=cw, ignore_index=255)
        probas = torch.softmax(sem, dim=1).transpose(1, 2).flatten(0, 1)
        labels = lab.flatten()
        if lovasz_ignore is not None:
            valid = labels != lovasz_ignore
            probas, labels = probas[valid], labels[valid]
        losses = []
        for c in range(probas.shape[1]):
            fg = (labels == c).float()
            if fg.sum() == 0:                     # a host synchronisation per class, as the reference
                continue
            errors = (fg - probas[:, c]).abs()
            errors_sorted, perm = torch.sort(errors, 0, descending=True)
            fg_sorted = fg[perm]
            gts = fg_sorted.sum()
            jac = 1.0 - (gts - fg_sorted.cumsum(0)) / (gts + (1.0 - fg_sorted).cumsum(0))
            jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
            losses.append(torch.dot(errors_sorted, jac))
        lov = sum(losses) / len(losses) if losses else 0.0
        tot = tot + ce_weight * ce + lovasz_weight * lov
    return tot / len(pred_occ)


def _f_torch(x):
    """-log sigmoid(inverse_sigmoid(x)) as the reference evaluates it: the shifts are host loops on a device scalar."""
    x = x.float()
    while x >= 1 - 1e-5:
        x = x - 1e-5
    while x < 1e-5:
        x = x + 1e-5
    return F.softplus(torch.log(1 / x - 1))


def torch_scal(pred_occ, label, mask, empty=17, ignore=255):
    """The two affinity terms restated with torch ops, host synchronisations included: sum over layers of sem + geo."""
    occ = mask.flatten(1)
    lab = label[occ]
    valid = lab != ignore
    y = lab[valid]
    tot = 0.0
    for sem in pred_occ:
        p = torch.softmax(sem.transpose(1, 2)[occ], dim=1)[valid]          # [|V|, C]
        loss, count = 0.0, 0
        for i in range(p.shape[1] - 1):
            t = (y == i).float()
            if t.sum() > 0:
                count += 1
                num = (p[:, i] * t).sum()
                if p[:, i].sum() > 0:
                    loss = loss + _f_torch(num / (p[:, i].sum() + 1e-5))
                loss = loss + _f_torch(num / (t.sum() + 1e-5))
                if (1 - t).sum() > 0:
                    loss = loss + _f_torch(((1 - p[:, i]) * (1 - t)).sum() / ((1 - t).sum() + 1e-5))
        occupied, q = (y != empty).float(), 1 - p[:, empty]
        inter = (occupied * q).sum()
        geo = (_f_torch(inter / (q.sum() + 1e-5)) + _f_torch(inter / (occupied.sum() + 1e-5))
               + _f_torch(((1 - occupied) * p[:, empty]).sum() / ((1 - occupied).sum() + 1e-5)))
        tot = tot + loss / count + geo
    return tot / len(pred_occ)


def bench_scal(args, dev, cw):
    out = os.path.join(ROOT, "profiles", "bench_loss_scal.jsonl")
    parent = _lib.load_other(args.parent_lib) if args.parent_lib else None
    for L in (int(v) for v in args.layers.split(",")):
        x, label, mask = make_occ_loss_inputs(args.n, L, seed=L, mask_frac=0.05)
        leaves = [torch.from_numpy(r).to(dev)[None].requires_grad_(True) for r in x]
        lab = torch.from_numpy(label).to(dev)[None]
        m = torch.from_numpy(mask).to(dev)[None]
        kw = dict(class_weights=cw, ce_weight=10.0, lovasz_ignore=17)
        sides = {
            "scal": lambda p: occupancy_loss(p, lab, m, sem_scal_weight=1.0, geo_scal_weight=1.0, **kw),
            "base": lambda p: occupancy_loss(p, lab, m, **kw),
            "base+torch": lambda p: occupancy_loss(p, lab, m, **kw) + torch_scal(p, lab, m),
        }
        if parent is not None:
            sides["parent"] = lambda p: occupancy_loss(p, lab, m, **kw)
        medians = {k: [] for k in sides}
        losses = {}
        for r in range(args.rounds + 1):                 # round 0 warms every side up and is not counted
            for name, fn in sides.items():
                times = []
                with _lib.routed_to(parent) if name == "parent" else contextlib.nullcontext():
                    for _ in range(args.warmup if r == 0 else args.steps):
                        for t in leaves:
                            t.grad = None
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        loss = fn([t.transpose(1, 2) for t in leaves])
                        loss.backward()
                        b.record()
                        b.synchronize()
                        times.append(a.elapsed_time(b) * 1e3)
                if r:
                    medians[name].append(statistics.median(times))
                losses[name] = float(loss.item())
        with open(out, "a") as f:
            for name, meds in medians.items():
                line = json.dumps(dict(bench="occ_loss_scal", path=name, L=L, N=args.n, rounds=args.rounds, steps=args.steps,
                                       median_us=round(statistics.median(meds), 1), min_us=round(min(meds), 1),
                                       max_us=round(max(meds), 1), loss=losses[name]))
                print(line, flush=True)
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=640000)
    ap.add_argument("--paths", default="native,torch,native_all", help="comma-separated subset of the paths")
    ap.add_argument("--layers", default="1,4", help="comma-separated layer counts")
    ap.add_argument("--scal", action="store_true", help="the affinity terms: native with them against the baselines")
    ap.add_argument("--rounds", type=int, default=7, help="--scal: rounds of alternating sides")
    ap.add_argument("--parent-lib", default=None, help="--scal: a build of the library at the parent commit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py needs an MI355X")
    dev = torch.device("cuda:0")
    cw = (18 * F.normalize(torch.tensor(MANUAL), 1, -1)).to(dev)
    if args.scal:
        return bench_scal(args, dev, cw)
    for L in (int(v) for v in args.layers.split(",")):
        x, label, mask = make_occ_loss_inputs(args.n, L, seed=L, mask_frac=0.05)
        leaves = [torch.from_numpy(r).to(dev)[None].requires_grad_(True) for r in x]
        lab = torch.from_numpy(label).to(dev)[None]
        m = torch.from_numpy(mask).to(dev)[None]
        paths = {
            "native": lambda p: occupancy_loss(p, lab, m, class_weights=cw, ce_weight=10.0, lovasz_ignore=17),
            "torch": lambda p: torch_loss(p, lab, m, cw),
            "native_all": lambda p: occupancy_loss(p, lab, m, class_weights=cw, ce_weight=10.0, lovasz_ignore=None),
        }
        for name, fn in paths.items():
            if name not in args.paths.split(","):
                continue
            def once():
                for t in leaves:
                    t.grad = None
                loss = fn([t.transpose(1, 2) for t in leaves])
                loss.backward()
                return loss
            for _ in range(args.warmup):
                once()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                loss = once()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b) * 1e3)
            med = statistics.median(times)
            print(json.dumps(dict(path=name, L=L, N=args.n, steps=args.steps, median_us=round(med, 1),
                                  per_layer_us=round(med / L, 1), min_us=round(min(times), 1), max_us=round(max(times), 1),
                                  loss=float(loss.item()), kept_frac_lovasz=float(((label != 17) & mask).mean()))),
                  flush=True)


if __name__ == "__main__":
    main()
