"""Drop-in for ``misc.metric_util``: the imports at eval.py, train.py and visualize.py (``from misc.metric_util import
MeanIoU``) resolve here when this repo root is on ``sys.path``.  Semantics and the two deliberate differences (int64
totals, ``outputs`` not mutated): gaussianformer_amd/metric.py, DESIGN.md §3.6b."""
from gaussianformer_amd.metric import MeanIoU  # noqa: F401
