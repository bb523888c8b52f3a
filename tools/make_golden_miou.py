"""Record the reference's own evaluation metric -> tests/golden/miou.npz.

Loads misc/metric_util.py from the reference tree UNMODIFIED and runs ``MeanIoU`` on the CPU, with two stand-ins that live
in this tool's process only: a stub ``mmengine.MMLogger`` (the module asks for a logger at import) and ``torch.Tensor.cuda``
patched to the identity.  Per case the fixture holds data only: the settings, every frame's inputs, the three totals
after every step and the two numbers of ``_after_epoch``.  The reference writes into its inputs (the label remap into
``semantics``, the z filter into ``outputs``), so it is handed copies and the fixture keeps the originals.

Cases (a few hundred voxels each):
  eval_mask     eval.py's call: flat tensors with a mask, filter_minmax=False, two frames
  eval_nomask   the same frames without a mask
  dict_band     the dict form, dataset_empty_label=0, filter_minmax=True, use_mask=True, uint8 semantics with 0 and 255,
                occupied voxels only in a middle band of z (6 x 5 x 16), two frames
  dict_nomask   the same frames with use_mask=False
  dict_d5       the dict form on a 7 x 3 x 5 grid
  absent        flat int64 targets with 0 and 255, a permuted class list, one class that never occurs

    python tools/make_golden_miou.py [reference_root]
"""
import importlib.util
import logging
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GF_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "miou.npz")
EMPTY = 17
ABSENT = 9


def load_reference():
    class MMLogger:
        @staticmethod
        def get_instance(name, **kw):
            return logging.getLogger(name)

    mm = types.ModuleType("mmengine")
    mm.MMLogger = MMLogger
    sys.modules["mmengine"] = mm
    torch.Tensor.cuda = lambda self, *a, **k: self
    spec = importlib.util.spec_from_file_location("gf_ref_metric_util", os.path.join(REFERENCE, "misc", "metric_util.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def draw_grid(rng, shape, band, dataset_empty):
    """uint8 semantics with occupied voxels (1..16, a few 255) in the z band only, ``dataset_empty`` elsewhere; predictions
    over the whole grid (so the filter has something to remove); a camera mask that keeps about 70 %."""
    sem = np.full(shape, dataset_empty, dtype=np.uint8)
    occ = rng.random(shape) < 0.35
    occ[..., :band[0]] = False
    occ[..., band[1] + 1:] = False
    occ[0, 0, band[0]] = occ[-1, -1, band[1]] = True      # both ends of the band are occupied
    sem[occ] = rng.integers(1, 17, size=int(occ.sum()))
    sem[sem == ABSENT] = 3
    ign = occ & (rng.random(shape) < 0.05)
    sem[ign] = 255
    out = np.where(rng.random(shape) < 0.6, np.where(sem == dataset_empty, EMPTY, sem).astype(np.int64),
                   rng.integers(0, 18, size=shape))
    mask = (rng.random(shape) < 0.7).astype(np.uint8)
    return out.astype(np.int64), sem, mask


def main():
    mod = load_reference()
    rng = np.random.default_rng(20261021)
    names = [f"class{c}" for c in range(1, 17)]
    fix = {}

    def record(case, classes, frames, dict_form, use_mask=False, dataset_empty=17, filter_minmax=True):
        m = mod.MeanIoU(list(classes), EMPTY, names[:len(classes)], use_mask, dataset_empty, filter_minmax, name=case)
        m.reset()
        totals = []
        for f, (out, tgt, mask) in enumerate(frames):
            fix[f"{case}_outputs_{f}"], fix[f"{case}_targets_{f}"] = out, tgt
            if mask is not None:
                fix[f"{case}_mask_{f}"] = mask
            o = torch.from_numpy(out.copy())
            if dict_form:
                m._after_step(o, {"semantics": tgt.copy(), "mask_camera": mask.copy()})
            else:
                m._after_step(o, torch.from_numpy(tgt.copy()), None if mask is None else torch.from_numpy(mask.copy()).bool())
            step = torch.stack([m.total_seen, m.total_correct, m.total_positive]).numpy()
            assert step.dtype == np.float32 and np.all(step == np.round(step)) and step.max() < 2 ** 24   # still exact here
            totals.append(step.astype(np.int64))
        miou, occ_iou = m._after_epoch()
        fix[f"{case}_classes"] = np.array(list(classes), dtype=np.int64)
        fix[f"{case}_cfg"] = np.array([EMPTY, dataset_empty, int(use_mask), int(filter_minmax), int(dict_form), len(frames)], dtype=np.int64)
        fix[f"{case}_totals"] = np.stack(totals)                      # [frames, 3, K + 1]
        fix[f"{case}_epoch"] = np.array([float(miou), float(occ_iou)], dtype=np.float64)
        print(case, float(miou), float(occ_iou))

    # eval.py's call: pred_occ / gt_occ [1, N] with occ_mask, labels 0..17 (17 = empty)
    flat = []
    for _ in range(2):
        N = 480
        tgt = np.where(rng.random(N) < 0.6, EMPTY, rng.integers(0, 17, N)).astype(np.int64)
        out = np.where(rng.random(N) < 0.5, tgt, rng.integers(0, 18, N)).astype(np.int64)
        flat.append((out[None], tgt[None], (rng.random(N) < 0.7)[None]))
    record("eval_mask", range(1, 17), flat, False, filter_minmax=False)
    record("eval_nomask", range(1, 17), [(o, t, None) for o, t, _ in flat], False, filter_minmax=False)
    band = [draw_grid(rng, (6, 5, 16), (5, 11), 0), draw_grid(rng, (6, 5, 16), (3, 3), 0)]
    record("dict_band", range(1, 17), band, True, use_mask=True, dataset_empty=0)
    record("dict_nomask", range(1, 17), band, True, use_mask=False, dataset_empty=0)
    record("dict_d5", range(1, 17), [draw_grid(rng, (7, 3, 5), (1, 3), 0)], True, use_mask=True, dataset_empty=0)
    N = 300
    tgt = np.where(rng.random(N) < 0.5, EMPTY, rng.integers(0, 17, N)).astype(np.int64)
    tgt[tgt == ABSENT] = 2
    tgt[rng.random(N) < 0.05] = 255
    out = np.where(rng.random(N) < 0.5, np.minimum(tgt, 17), rng.integers(0, 18, N)).astype(np.int64)
    out[out == ABSENT] = 4
    perm = [5, 1, 16, ABSENT, 3, 12, 2]
    record("absent", perm, [(out, tgt, rng.random(N) < 0.8)], False, filter_minmax=False)
    assert not np.any(tgt == ABSENT) and np.any(tgt == 0) and np.any(tgt == 255)
    np.savez_compressed(OUT, **fix)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
