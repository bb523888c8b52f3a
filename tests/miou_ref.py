"""Int64 numpy restatement of the evaluation metric's contract (gaussianformer_amd/metric.py, include/gf_hip.h "evaluation
metric"): what one ``_after_step`` adds to the three totals, and the numbers ``_after_epoch`` derives from them.  Written
voxel-set by voxel-set from the contract -- select, then count -- the way the reference reads, not the way the kernels
count (they never compact and apply the z filter to a table): agreement is a check of both.
"""
import numpy as np


class MiouRef:
    def __init__(self, class_indices, empty_label, use_mask=False, dataset_empty_label=17, filter_minmax=True):
        self.class_indices = list(class_indices)
        self.empty_label = empty_label
        self.use_mask = use_mask
        self.dataset_empty_label = dataset_empty_label
        self.filter_minmax = filter_minmax
        self.reset()

    def reset(self):
        K1 = len(self.class_indices) + 1
        self.totals = np.zeros((3, K1), dtype=np.int64)   # seen, correct, positive
        self.frames = 0
        self.unfiltered = 0     # frames whose filter found no occupied target voxel (counted without the filter)

    def frame(self, outputs, targets, mask=None):
        """The frame's contribution, int64 [3, K + 1] (also added to ``totals``).  ``targets`` an array, or the dict form."""
        e = self.empty_label
        outputs = np.array(outputs, dtype=np.int64)   # a copy: the caller's array is left alone
        if isinstance(targets, dict):
            assert mask is None
            t = np.array(targets['semantics'], dtype=np.int64)
            t[t == self.dataset_empty_label] = e
            outputs = outputs.reshape(t.shape)
            if self.filter_minmax:
                zs = np.nonzero(t != e)[-1]
                if zs.size:
                    outputs[..., zs.max() + 1:] = e
                    outputs[..., :zs.min()] = e
                else:
                    self.unfiltered += 1
            if self.use_mask:
                mask = np.asarray(targets['mask_camera']).astype(bool)
        else:
            t = np.array(targets, dtype=np.int64)
        o, t = outputs.reshape(-1), t.reshape(-1)
        if mask is not None:
            keep = np.asarray(mask).astype(bool).reshape(-1)
            o, t = o[keep], t[keep]
        add = np.zeros_like(self.totals)
        for i, c in enumerate(self.class_indices):
            add[:, i] = np.sum(t == c), np.sum((t == c) & (o == c)), np.sum(o == c)
        add[:, -1] = np.sum(t != e), np.sum((t != e) & (o != e)), np.sum(o != e)
        self.totals += add
        self.frames += 1
        return add

    def epoch(self, totals=None):
        """``(miou * 100, occ_iou * 100, ious, precisions, recalls)`` from the totals, in float64."""
        seen, correct, positive = (np.asarray(self.totals if totals is None else totals, dtype=np.int64)[r] for r in range(3))
        ious, precs, recas = [], [], []
        for i in range(len(self.class_indices)):
            precs.append(0.0 if positive[i] == 0 else float(correct[i]) / float(positive[i]))
            if seen[i] == 0:
                ious.append(1.0)
                recas.append(1.0)
            else:
                ious.append(float(correct[i]) / float(seen[i] + positive[i] - correct[i]))
                recas.append(float(correct[i]) / float(seen[i]))
        union = float(seen[-1] + positive[-1] - correct[-1])
        occ = float(correct[-1]) / union if union else float("nan")
        return float(np.mean(ious)) * 100, occ * 100, ious, precs, recas
