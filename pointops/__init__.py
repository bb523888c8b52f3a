"""Drop-in for ``pointops.farthest_point_sampling``: the import at model/lifter/gaussian_lifter_v2.py:9-12
(``from pointops import farthest_point_sampling``) resolves here when this repo root is on ``sys.path``.
Semantics and limits: gaussianformer_amd/sampling.py, DESIGN.md §3.8."""
from gaussianformer_amd.sampling import farthest_point_sampling  # noqa: F401
