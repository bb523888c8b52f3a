"""Record the reference's own occupancy loss with its scene-class affinity terms -> tests/golden/occ_scal.npz.

As tools/make_golden_occ_loss.py (whose stubs and error-separation rule this tool imports): loss/occupancy_loss.py from the
reference tree UNMODIFIED, ``OccupancyLoss(**cfg)(inputs)`` and its backward on the CPU in fp32 -- here with
``use_sem_geo_scal_loss=True`` and the weights CE 10, Lovász 1, sem_scal 0.7, geo_scal 1.3, for the softmax and the prob
config, at N = 1 500 voxels and 2 layers, with a mask, some ignore_index (255) labels and an absent class.  The Lovász part
stays unambiguous by the same rule: within every present class no two fp32 errors within 2^-18 relative of each other.

    python tools/make_golden_occ_scal.py [reference_root]
"""
import os

import numpy as np
import torch

import make_golden_occ_loss as base

OUT = os.path.join(base.ROOT, "tests", "golden", "occ_scal.npz")
N, L, C, ABSENT = base.N, base.L, base.C, base.ABSENT
WEIGHTS = dict(loss_voxel_ce_weight=10.0, loss_voxel_lovasz_weight=1.0, loss_voxel_sem_scal_weight=0.7,
               loss_voxel_geo_scal_weight=1.3)
BASE = dict(base.BASE, multi_loss_weights=WEIGHTS, use_sem_geo_scal_loss=True)
CONFIGS = {"softmax": dict(BASE), "prob": dict(BASE, ignore_empty=False, lovasz_use_softmax=False)}


def main():
    mod = base.install_stubs()
    rng = np.random.default_rng(20261021)
    out = {}
    label = rng.integers(0, C, N)
    label[rng.random(N) < 0.5] = 17
    label[label == ABSENT] = 5
    label[rng.random(N) < 0.04] = 255
    mask = rng.random(N) < 0.8
    keep = mask & (label != 17)                     # the Lovász voxels (lovasz_ignore = 17)
    assert not np.any(label[mask] == ABSENT) and np.any(label[mask] == 255) and np.any(label[mask] == 17)
    out["label"], out["mask"] = label.astype(np.int64), mask
    for mode, cfg in CONFIGS.items():
        softmax = cfg.get("lovasz_use_softmax", True)
        if softmax:
            draw = lambda r, k: (2.0 * r.standard_normal((k, C))).astype(np.float32)
        else:
            draw = lambda r, k: torch.softmax(torch.from_numpy((2.0 * r.standard_normal((k, C))).astype(np.float32)), 1).numpy()
        layers = [base.separate(rng, draw(rng, N), label, keep, softmax, draw) for _ in range(L)]
        for rows in layers:
            e = base.errors_f32(rows, label, keep, softmax)
            for c in range(C):
                if np.any(label[keep] == c):
                    s = np.sort(e[:, c]).astype(np.float64)
                    assert np.all(s[1:] - s[:-1] > base.SEP * np.maximum(s[1:], 1e-30)), (mode, c)
        m = mod.OccupancyLoss(**cfg)
        leaves = [torch.from_numpy(r)[None].clone().requires_grad_(True) for r in layers]   # [1, N, C]
        pred = [t.transpose(1, 2) for t in leaves]                                          # the head's [1, C, N] view
        loss = m({"pred_occ": pred, "sampled_xyz": None, "sampled_label": torch.from_numpy(label)[None],
                  "occ_mask": torch.from_numpy(mask)[None]})
        loss.backward()
        out[f"{mode}_pred"] = np.stack(layers)                                    # [L, N, C]
        out[f"{mode}_loss"] = np.float64(loss.item())
        out[f"{mode}_grad"] = np.stack([t.grad[0].numpy() for t in leaves])       # [L, N, C]
        out[f"{mode}_class_weights"] = m.class_weights.float().numpy()
        print(mode, loss.item())
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", os.path.getsize(base.OUT), "bytes in", os.path.basename(base.OUT))


if __name__ == "__main__":
    main()
