"""Shared by test_miou.py and test_miou_gpu.py: the fixture's cases (tests/golden/miou.npz, recorded from the reference by
tools/make_golden_miou.py) and random frames, each with the settings to build ``MeanIoU`` and ``MiouRef`` alike."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "miou.npz")
CASES = ("eval_mask", "eval_nomask", "dict_band", "dict_nomask", "dict_d5", "absent")
PERMUTED = [7, 16, 2, 11, 1, 5, 9, 14, 3, 12, 6, 8, 15, 4, 13, 10]
WITH_EMPTY = [3, 17, 1, 0, 12]           # contains empty_label (17) and label 0


def load_case(fix, case):
    """``(settings, frames, totals [frames, 3, K + 1], (miou, occ_iou))``: ``settings`` are keyword arguments of both classes,
    a frame is ``(outputs, targets, mask)`` with ``targets`` the dict form where the case used it."""
    empty, dataset_empty, use_mask, filter_minmax, dict_form, n = (int(v) for v in fix[f"{case}_cfg"])
    settings = dict(class_indices=[int(c) for c in fix[f"{case}_classes"]], empty_label=empty, use_mask=bool(use_mask),
                    dataset_empty_label=dataset_empty, filter_minmax=bool(filter_minmax))
    frames = []
    for f in range(n):
        out, tgt = fix[f"{case}_outputs_{f}"], fix[f"{case}_targets_{f}"]
        mask = fix[f"{case}_mask_{f}"] if f"{case}_mask_{f}" in fix.files else None
        frames.append((out, {"semantics": tgt, "mask_camera": mask}, None) if dict_form else (out, tgt, mask))
    return settings, frames, fix[f"{case}_totals"], tuple(fix[f"{case}_epoch"])


def random_frame(rng, shape, dict_form, u8, masked, band=None, dataset_empty=0):
    """Predictions 0..17 with a few 255, targets with 0 and 255, about 60 % empty; ``band``: occupied targets in these z only."""
    empty_in = dataset_empty if dict_form else 17
    tgt = np.where(rng.random(shape) < 0.6, empty_in, rng.integers(0, 18, shape))
    tgt[rng.random(shape) < 0.04] = 255
    tgt[rng.random(shape) < 0.04] = 0
    if band is not None:
        z = np.arange(shape[-1])
        tgt[..., (z < band[0]) | (z > band[1])] = empty_in
    seen_as = np.where(tgt == empty_in, 17, tgt)
    out = np.where(rng.random(shape) < 0.5, np.minimum(seen_as, 17), rng.integers(0, 18, shape))
    out[rng.random(shape) < 0.02] = 255
    tgt = tgt.astype(np.uint8 if u8 else np.int64)
    mask = (rng.random(shape) < 0.7) if masked else None
    if dict_form:   # mask_camera as bytes, any non-zero value keeps the voxel (the reference's .bool())
        keep = (mask if masked else np.ones(shape, bool)).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
        return out.astype(np.int64), {"semantics": tgt, "mask_camera": keep}, None
    return out.astype(np.int64), tgt, mask
