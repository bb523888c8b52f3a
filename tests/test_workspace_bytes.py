"""Every ``*_bytes`` entry point of the C ABI against tests/golden/workspace_bytes.json, a table of
(entry point, arguments) -> bytes recorded by tools/make_golden_workspace_bytes.py with the library whose workspace layouts are
to be kept.  The size queries are host code: no GPU needed.  A 0 in the table is a refused shape."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")

_GRID = (640000, 200, 200, 16)                       # the nuScenes occupancy grid: N, H, W, D
_DCN3 = (6, 256, 54, 100, 256, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1)   # ResNet layer3: N, C, H, W, Co, kernel, stride, padding, dilation, groups, dg

# entry point -> argument tuples: the smallest legal shape, production shapes, both sides of every edge of the carve, and the
# refused shapes the other suites use
CASES = {
    "gf_splat_workspace_bytes": [
        (100, 1000, 20, 20, 16), (25601, *_GRID),
        (0, *_GRID), (64, *_GRID), (39552, *_GRID), (39553, *_GRID),           # the kWRow edge: summaries, ten rows per Gaussian
        (144000, *_GRID), (262144, *_GRID), (262145, *_GRID),                  # the kLongWords edge: no matrix-core backward beyond
        (100, 0, 20, 20, 16), (0, 0, 1, 1, 1),                                 # N = 0; the smallest
        (100, 1000, 20, 20, 13), (100, 1000, 21, 27, 16), (50000, 1000, 21, 27, 13), (262145, 1000, 21, 27, 13),
        (-1, 0, 20, 20, 16), (100, -1, 20, 20, 16), (100, 1000, 0, 20, 16),    # refused
    ],
    "gf_subm_tables_bytes": [
        (0, 1, 1, 1, 1, 1), (1000, 1, 50, 50, 8, 3), (25600, 1, 200, 200, 16, 5), (25600, 2, 200, 200, 16, 7),
        (1000, 1, 50, 50, 8, 2), (1000, 1, 50, 50, 8, 9), (-1, 1, 50, 50, 8, 3), (1000, 0, 50, 50, 8, 3),
    ],
    "gf_subm_apply_scratch_bytes": [(1, 1), (1, 32), (1000, 128), (25600, 128), (25601, 64), (0, 128), (1000, 0)],
    "gf_occ_loss_workspace_bytes": [(1, 1, 18, 0), (2, 1000, 18, 0), (1, 640000, 18, 0), (4, 640000, 18, 0), (8, 640000, 18, 0),
                                    (1, 100, 17, 0), (9, 100, 18, 0), (1, 0, 18, 0)],
    "gf_occ_loss_scratch_bytes": [(1, 1, 18, 0), (2, 1000, 18, 0), (1, 640000, 18, 0), (4, 640000, 18, 0), (8, 640000, 18, 0),
                                  (1, 100, 17, 0), (9, 100, 18, 0), (1, 0, 18, 0)],
    "gf_lift_workspace_bytes": [(1, 1, 1), (1, 1000, 2), (1, 129600, 1), (2, 129600, 8), (1, 129600, 9), (0, 100, 1)],
    "gf_pixel_loss_workspace_bytes": [(1, 1), (1000, 64), (129600, 129), (10, 257), (0, 64)],
    "gf_fps_workspace_bytes": [(1,), (7,), (1000,), (129600,), (262144,), (0,), (-1,)],
    "gf_daf_backward_workspace_bytes": [
        (1, 1, 1, 64, 1, 0, 1), (1, 6, 1000, 128, 4, 900, 4), (1, 6, 14960, 128, 4, 332800, 4), (2, 6, 14960, 256, 4, 332800, 8),
        (1, 6, 1000, 128, 4, 900, 3), (1, 6, 1000, 100, 4, 900, 4), (-1, 6, 1000, 128, 4, 900, 4),
    ],
    "gf_daf_fused_backward_workspace_bytes": [(0, 0, 1, 1, 1, 1), (1, 1, 1, 1, 1, 1), (1, 4, 9, 6, 4, 4), (1, 25600, 13, 6, 4, 4), (-1, 4, 9, 6, 4, 4),
                                              (1, 4, 43, 6, 4, 4)],
    "gf_dcn_workspace_bytes": [
        (0, 32, 1, 1, 32, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0), (0, 32, 1, 1, 32, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1),
        (1, 32, 8, 8, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0), (1, 32, 8, 8, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1),
        (*_DCN3, 0), (*_DCN3, 1), (6, 512, 27, 50, 512, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1),
        (1, 32, 8, 8, 32, 3, 3, 1, 1, 1, 1, 1, 1, 2, 1, 0), (1, 32, 8, 8, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1, 3, 1),
        (1, 48, 8, 8, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1),
    ],
}

# read from the library of the commit before the shared carver, by hand
CROSS_CHECK = {
    ("gf_splat_workspace_bytes", (100, 1000, 20, 20, 16)): 484096,
    ("gf_splat_workspace_bytes", (144000, 640000, 200, 200, 16)): 236463104,
    ("gf_subm_tables_bytes", (1000, 1, 50, 50, 8, 3)): 305408,
    ("gf_subm_apply_scratch_bytes", (1000, 128)): 516096,
    ("gf_occ_loss_workspace_bytes", (2, 1000, 18, 0)): 148992,
    ("gf_occ_loss_scratch_bytes", (2, 1000, 18, 0)): 651520,
    ("gf_lift_workspace_bytes", (1, 1000, 2)): 26368,
    ("gf_pixel_loss_workspace_bytes", (1000, 64)): 256,
    ("gf_fps_workspace_bytes", (1000,)): 20224,
    ("gf_daf_backward_workspace_bytes", (1, 6, 1000, 128, 4, 900, 4)): 8833536,
    ("gf_daf_fused_backward_workspace_bytes", (1, 4, 9, 6, 4, 4)): 3456,
    ("gf_dcn_workspace_bytes", (1, 32, 8, 8, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1)): 90112,
}


def compute(lib):
    """The table as the loaded library gives it: {entry point: [[arguments, bytes], ...]} in CASES' order."""
    return {name: [[list(args), int(getattr(lib, name)(*args))] for args in cases] for name, cases in CASES.items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_covers_every_size_entry_point(golden):
    from gaussianformer_amd import _lib
    sized = {n for n in _lib.SIGNATURES if n.endswith("_bytes") and n != "gf_splat_state_bytes"}
    assert set(CASES) == sized == set(golden)
    for name, cases in CASES.items():
        assert [row[0] for row in golden[name]] == [list(a) for a in cases]
        values = [row[1] for row in golden[name]]
        assert 0 in values and any(v > 0 for v in values), name   # a refused shape and a legal one each
    for (name, args), nbytes in CROSS_CHECK.items():
        assert [list(args), nbytes] in golden[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_sizes_are_the_recorded_ones(golden, name):
    from gaussianformer_amd import _lib
    assert compute(_lib.load())[name] == golden[name]
