"""Evaluation metric: the reference's ``MeanIoU`` (misc/metric_util.py) with its per-frame step on the device.

``MeanIoU._after_step`` is what eval.py:163, train.py:317 and visualize.py:205 call after the head.  The reference compacts
predictions and targets by boolean indexing and then reads ``3 * (num_classes + 1)`` sums back with ``.item()`` -- 51 host
round trips a frame -- plus two ``nonzero()`` calls for ``filter_minmax``.  Here a frame is two launches (``gf_miou_step``,
csrc/miou.hip) that add into int64 totals on the device; nothing is read back before ``_after_epoch``, so
an evaluation loop can run ahead of the host or be captured in a graph.

Two deliberate differences from the reference:

* the totals are **int64**, not float32: the reference's float totals stop being exact at 2^24 -- the empty class alone
  receives about 6e5 voxels a frame, so after some 26 frames -- while these stay exact over any split;
* ``_after_step`` does **not** write the z-filtered values back into ``outputs`` (the reference's ``outputs[..., :min_z] =
  empty_label`` mutates the caller's tensor): the filter is applied to the counts.

A frame whose filter finds no occupied target voxel makes the reference raise (``.max()`` of an empty tensor).  The step
reads nothing back and cannot: such a frame is counted without the filter, and ``_after_epoch`` warns with their number.

GPU tensors always take the kernels.  CPU tensors take a torch composition of the same arithmetic (``torch.bincount`` of a
joint key per z slice, no ``.item()``), which makes the class logic testable without a GPU.
"""
import ctypes
import logging

import numpy as np
import torch
import torch.distributed as dist

from . import _lib

_B = _lib.GF_MIOU_MAX_CLASSES + 1     # label buckets of the CPU path: the values 0..31 and one for everything else


def _labels_torch(logits, bin_logits, threshold, empty_label, combine_geosem):
    """``occupancy_labels`` for CPU tensors (model/head/gaussian_head.py:164-185)."""
    if bin_logits is None:
        return logits.argmax(dim=1)
    if combine_geosem:
        return torch.cat([logits[:, :-1] * bin_logits[:, None], 1 - bin_logits[:, None]], dim=1).argmax(dim=1)
    return torch.where(bin_logits > threshold, logits.argmax(dim=1), torch.full_like(bin_logits, empty_label, dtype=torch.int64))


class MeanIoU:
    """Drop-in for the reference's ``MeanIoU``: its constructor arguments in its order, plus ``device`` (where the totals
    live; default: the GPU when there is one) and ``logger`` (default ``logging.getLogger('selfocc')``).  ``total_seen``,
    ``total_correct`` and ``total_positive`` are int64 views ``[num_classes + 1]`` of the device totals."""

    _scratch = _lib.StreamScratch()

    def __init__(self, class_indices, empty_label, label_str, use_mask=False, dataset_empty_label=17, filter_minmax=True,
                 name='none', device=None, logger=None):
        self.class_indices = [int(c) for c in class_indices]
        self.num_classes = len(self.class_indices)
        if not 1 <= self.num_classes <= _lib.GF_MIOU_MAX_CLASSES:
            raise ValueError(f"MeanIoU: 1..{_lib.GF_MIOU_MAX_CLASSES} classes are supported, got {self.num_classes}")
        if any(not 0 <= c < _lib.GF_MIOU_MAX_CLASSES for c in self.class_indices):
            raise ValueError(f"MeanIoU: class indices must lie in [0, {_lib.GF_MIOU_MAX_CLASSES})")
        self.empty_label = int(empty_label)
        self.dataset_empty_label = int(dataset_empty_label)
        self.label_str = label_str
        self.use_mask = use_mask
        self.filter_minmax = filter_minmax
        self.name = name
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.logger = logger if logger is not None else logging.getLogger('selfocc')
        self._cls_host = (ctypes.c_int * self.num_classes)(*self.class_indices)
        self.reset()

    def reset(self) -> None:
        K1 = self.num_classes + 1
        if getattr(self, "_state", None) is not None:
            self._state.zero_()     # in place: a captured step keeps adding into the same words
            return
        self._state = torch.zeros(3 * K1 + 2, dtype=torch.int64, device=self.device)   # the totals, then the two status words
        self._totals = self._state[:3 * K1].view(3, K1)
        self._status = self._state[3 * K1:]    # frames counted; frames whose filter found no occupied target
        self.total_seen, self.total_correct, self.total_positive = self._totals[0], self._totals[1], self._totals[2]

    # ---- inputs

    def _flat(self, x, dtype=None):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        x = x.to(self.device, non_blocking=True).reshape(-1)
        return x if dtype is None else _lib.as_arg(x, dtype)

    def _frame(self, targets, mask):
        """``(targets [N], mask [N] uint8 or None, D, flags)`` of either call form (:38-55)."""
        if not isinstance(targets, (torch.Tensor, np.ndarray)):
            assert mask is None
            sem = targets['semantics']
            D = int(sem.shape[-1])
            flags = _lib.GF_MIOU_REMAP | (_lib.GF_MIOU_FILTER_MINMAX if self.filter_minmax else 0)
            mask = targets['mask_camera'] if self.use_mask else None
            targets = sem
        else:
            D, flags = 1, 0
        t = self._flat(targets)
        if t.dtype == torch.uint8:
            flags |= _lib.GF_MIOU_TARGETS_U8
        t = _lib.as_arg(t, t.dtype if t.dtype == torch.uint8 else torch.int64)
        if mask is not None:
            mask = self._flat(mask)
            if mask.dtype not in (torch.bool, torch.uint8):
                raise TypeError(f"MeanIoU: the mask must be a bool (or uint8) tensor, got {mask.dtype}")
            mask = _lib.as_arg(mask, mask.dtype).view(torch.uint8)   # the kernel keeps a voxel whose byte is not 0, as .bool() does
            if mask.numel() != t.numel():
                raise ValueError(f"MeanIoU: mask has {mask.numel()} entries, targets {t.numel()}")
        if flags & _lib.GF_MIOU_FILTER_MINMAX and (D < 1 or t.numel() % D):
            raise ValueError(f"MeanIoU: filter_minmax needs a last dimension D >= 1 that divides the voxel count, got D = {D}")
        return t, mask, D, flags

    def _workspace(self, N, D, flags):
        nbytes = _lib.load().gf_miou_workspace_size(N, D, flags)
        if nbytes == 0:
            raise ValueError(f"gf_miou_workspace_size refused N={N}, D={D}, flags={flags}")
        return self._scratch.get(self.device, nbytes), nbytes

    # ---- steps

    def _after_step(self, outputs, targets, mask=None):
        """One frame added to the totals: ``outputs`` and ``targets`` tensors (or arrays) of one shape with an optional bool
        ``mask`` (:52-55), or ``targets`` a dict ``{'semantics', 'mask_camera'}`` (:38-51) whose labels are remapped
        (``dataset_empty_label -> empty_label``), z-filtered over the last dimension (``filter_minmax``) and masked
        (``use_mask``).  No host read, ``.item()``, ``nonzero()`` or boolean indexing.  Unlike the reference it does NOT
        write the filtered values into ``outputs``."""
        t, m, D, flags = self._frame(targets, mask)
        o = self._flat(outputs, torch.int64)
        if o.numel() != t.numel():
            raise ValueError(f"MeanIoU: outputs has {o.numel()} entries, targets {t.numel()}")
        if self.device.type != "cuda":
            return self._count_torch(o, t, m, D, flags)
        ws, nbytes = self._workspace(t.numel(), D, flags)
        _lib.call("gf_miou_step", self.device, t.numel(), D, flags, o, t, m, self.num_classes, self._cls_host, self.empty_label,
                  self.dataset_empty_label, self._totals, self._status, ws, nbytes)

    def _after_step_logits(self, logits, targets, mask=None, bin_logits=None, threshold=0.5, combine_geosem=False):
        """``_after_step(occupancy_labels(logits, bin_logits, threshold, empty_label, combine_geosem), targets, mask)`` in one
        counting pass over the head's ``logits [N,18]`` (and ``bin_logits [N]``): the labels are formed by the same rule and
        never written."""
        t, m, D, flags = self._frame(targets, mask)
        if isinstance(logits, np.ndarray):
            logits = torch.from_numpy(logits)
        lg = _lib.as_arg(logits.to(self.device, non_blocking=True))
        bl = None if bin_logits is None else self._flat(bin_logits, torch.float32)
        if lg.dim() != 2 or lg.shape[0] != t.numel():
            raise ValueError(f"MeanIoU: logits must be [N, {_lib.GF_NUM_CHANNELS}] with N = {t.numel()}, got {tuple(lg.shape)}")
        if self.device.type != "cuda":
            return self._count_torch(_labels_torch(lg, bl, threshold, self.empty_label, combine_geosem), t, m, D, flags)
        mode = _lib.GF_LABELS_ARGMAX if bl is None else (
            _lib.GF_LABELS_PROB_GEOSEM if combine_geosem else _lib.GF_LABELS_PROB_THRESHOLD)
        ws, nbytes = self._workspace(t.numel(), D, flags)
        _lib.call("gf_miou_step_logits", self.device, t.numel(), D, flags, lg.shape[1], mode, lg, bl, float(threshold), t, m,
                  self.num_classes, self._cls_host, self.empty_label, self.dataset_empty_label, self._totals, self._status, ws,
                  nbytes)

    def _count_torch(self, o, t, m, D, flags):
        """The step for CPU tensors: the joint (target, output) counts per z slice by ``torch.bincount``, then the finish
        pass's arithmetic on them."""
        e = self.empty_label
        filt = bool(flags & _lib.GF_MIOU_FILTER_MINMAX)
        D = D if filt else 1
        t = t.to(torch.int64)
        if flags & _lib.GF_MIOU_REMAP:
            t = torch.where(t == self.dataset_empty_label, torch.full_like(t, e), t)
        N = t.numel()
        z = torch.arange(N, device=t.device) % D
        kept = torch.ones_like(t) if m is None else (m != 0).to(torch.int64)
        t_occ, o_occ = (t != e).to(torch.int64), (o != e).to(torch.int64)
        tb = torch.where((t >= 0) & (t < _B - 1), t, torch.full_like(t, _B - 1))
        ob = torch.where((o >= 0) & (o < _B - 1), o, torch.full_like(o, _B - 1))
        joint = torch.bincount(((z * 2 + kept) * _B + tb) * _B + ob, minlength=D * 2 * _B * _B).view(D, 2, _B, _B)[:, 1]
        agg = torch.bincount(((z * 2 + kept) * 2 + t_occ) * 2 + o_occ, minlength=D * 8).view(D, 2, 2, 2)[:, 1]
        any_occ = torch.bincount(z * 2 + t_occ, minlength=D * 2).view(D, 2)[:, 1] > 0     # over all voxels, masked or not
        idx = torch.arange(D, device=t.device)
        lo, hi = torch.where(any_occ, idx, D).min(), torch.where(any_occ, idx, -1).max()
        inside = ((idx >= lo) & (idx <= hi)) if filt else torch.ones_like(any_occ)
        inside = (inside | ~any_occ.any()).to(torch.int64)
        # outside [min_z, max_z] every kept prediction reads empty_label: the slice's counts move to that column
        eb = e if 0 <= e < _B - 1 else _B - 1
        moved = torch.zeros_like(joint)
        moved[:, :, eb] = joint.sum(2)
        table = (joint * inside[:, None, None] + moved * (1 - inside)[:, None, None]).sum(0)
        cls = torch.tensor(self.class_indices, dtype=torch.int64, device=t.device)
        K = self.num_classes
        self._totals[0, :K] += table.sum(1)[cls]
        self._totals[1, :K] += table.diagonal()[cls]
        self._totals[2, :K] += table.sum(0)[cls]
        self._totals[0, K] += agg[:, 1, :].sum()
        self._totals[1, K] += (agg[:, 1, 1] * inside).sum()
        self._totals[2, K] += (agg[:, :, 1].sum(1) * inside).sum()
        self._status[0] += 1
        if filt:
            self._status[1] += (~any_occ.any()).to(torch.int64)

    # ---- epoch

    def _after_epoch(self):
        """All-reduces the totals when a process group is initialised (:69-73), reads them back (the one host read) and
        computes the reference's numbers (:75-111) from the exact integers in float64.  Returns ``(miou * 100, occ_iou *
        100)`` as Python floats."""
        if dist.is_initialized():
            dist.all_reduce(self._state)
            dist.barrier()
        host = self._state.cpu().numpy()
        K1 = self.num_classes + 1
        seen, correct, positive = (host[r * K1:(r + 1) * K1].astype(np.float64) for r in range(3))
        frames, unfiltered = int(host[3 * K1]), int(host[3 * K1 + 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            precs = np.where(positive == 0, 0.0, correct / positive)
            ious = np.where(seen == 0, 1.0, correct / (seen + positive - correct))
            recas = np.where(seen == 0, 1.0, correct / seen)
            occ_iou = correct[-1] / (seen[-1] + positive[-1] - correct[-1])
        miou = float(np.mean(ious[:-1]))
        logger = self.logger
        logger.info(f'Validation per class iou {self.name}:')
        for iou, prec, reca, label_str in zip(ious[:-1], precs[:-1], recas[:-1], self.label_str):
            logger.info('%s : %.2f%%, %.2f, %.2f' % (label_str, iou * 100, prec, reca))
        for r in range(3):
            logger.info(host[r * K1:(r + 1) * K1])
        if unfiltered:
            logger.warning(f'{unfiltered} of {frames} frames had no occupied target voxel: filter_minmax could not be applied, '
                           'they were counted unfiltered (the reference raises on such a frame)')
        return miou * 100, float(occ_iou) * 100
