"""The route of a splat forward -- which kernels a call gets, with which grids and which facts in their argument structs -- asked
of the library's own decision function through the debug hook gf_debug_splat_route, which launches nothing (no GPU needed).
The expectations are the rules of include/gf_hip.h (GF_MFMA_SPLAT, GF_EXACT_FP32, GF_PREPARE_BACKWARD, GF_WORKSPACE_ZEROED,
GF_PATH_*, "splat.mfma_tile_kernel") and DESIGN.md 3.1 / 3.2b / 3.2d / 3.6, written out below -- not the code's output.

Without a device the library takes 256 compute units (an MI355X has 256 as well), so the grid formulas below hold on both."""
import ctypes

import pytest

from gaussianformer_amd import _lib
from gaussianformer_amd._lib import (GF_COMP_EXP, GF_EXACT_FP32, GF_FAST_EXP, GF_LABELS_ARGMAX, GF_LABELS_PROB_GEOSEM,
                                     GF_LABELS_PROB_THRESHOLD, GF_LIBM_EXP, GF_MFMA_SPLAT, GF_PREPARE_BACKWARD, GF_PTS_ASSUME_DENSE,
                                     GF_PTS_GENERAL, GF_SPLAT_BASE, GF_SPLAT_PROB, GF_WORKSPACE_ZEROED)

from splat_cases import ARBITRARY, EXACT_TILE, MFMA_TILE, NO_LABELS, WAVE, WAVE_LONG, splat_route, tensors, units

EXP_LIBM, EXP_COMP, EXP_FAST = range(3)                          # word 3
CUS = 256
GRIDS = [(8, 8, 8), (48, 40, 16), (200, 200, 16)]
H, W, D = GRIDS[1]
V = H * W * D


def route(variant=GF_SPLAT_BASE, flags=0, label_mode=NO_LABELS, P=25601, N=V, grid=(H, W, D)):
    return splat_route(variant, flags, label_mode, P, N, grid)


@pytest.fixture
def tile_option():
    with _lib.option("splat.mfma_tile_kernel", 1):
        yield


def xcd_grid(items, per_cu):
    """Workgroups of a persistent kernel: `per_cu` per compute unit, dealt to 8 XCDs, at most one per item slot."""
    return 8 * min(-(-items // 8), max(1, per_cu * CUS // 8))


def splat_unit_grid(nunits):
    return xcd_grid(nunits, 8)


# 64 Gaussians per bitmask word: row words -> the largest P with that many
def P_of(nwords):
    return 64 * nwords


@pytest.mark.parametrize("nwords, zeroed, kernel", [
    (618, False, WAVE), (618, True, WAVE),             # the last row the wave kernel holds in LDS (P <= 39 552)
    (619, False, MFMA_TILE), (619, True, WAVE_LONG),   # long rows need the one-word verdict: GF_WORKSPACE_ZEROED
    (4096, False, MFMA_TILE), (4096, True, WAVE_LONG),   # the longest row (P <= 262 144)
    (4097, False, MFMA_TILE), (4097, True, MFMA_TILE),
])
def test_wave_long_row_and_tile_kernel_by_row_words(nwords, zeroed, kernel):
    r = route(P=P_of(nwords), flags=GF_WORKSPACE_ZEROED if zeroed else 0)
    assert r["kernel"] == kernel
    assert r["summaries"] == (kernel == WAVE_LONG)
    assert r["one_verdict"] == (zeroed and kernel in (WAVE, WAVE_LONG))
    assert r["range_flags"] == 1 and r["prescale"] == 0 and r["lattice"] == r["verify"] == 1 and r["range_theta_here"] == 0
    nsuper = -(-H // 8) * -(-W // 8)
    grid = splat_unit_grid(units((H, W, D))) if kernel != MFMA_TILE else xcd_grid(2 * nsuper, 2)   # two 8 x 4 tiles per supertile
    assert r["render_grid"] == grid and r["tile_counter_init"] == grid // 8


@pytest.mark.parametrize("nwords, zeroed", [(618, False), (619, True), (4096, True)])
def test_the_option_keeps_the_tile_kernel(tile_option, nwords, zeroed):
    r = route(P=P_of(nwords), flags=GF_WORKSPACE_ZEROED if zeroed else 0)
    assert r["kernel"] == MFMA_TILE and r["summaries"] == 0 and r["one_verdict"] == 0


@pytest.mark.parametrize("flag, exp", [(GF_FAST_EXP, EXP_FAST), (GF_LIBM_EXP, EXP_LIBM), (GF_COMP_EXP, EXP_COMP), (GF_EXACT_FP32, EXP_FAST)])
def test_exp_flags_and_exact_fp32_leave_the_matrix_cores_and_mfma_splat_returns(flag, exp):
    r = route(flags=flag)
    assert r["kernel"] == EXACT_TILE and r["exp"] == exp and r["range_flags"] == 0 and r["tile_counter_init"] == 0
    assert r["prescale"] == (exp == EXP_FAST)   # the prescaled records belong to the bare v_exp_f32
    assert r["render_grid"] == 8 * -(-(-(-H // 8) * -(-W // 8)) // 8) * 2   # two tiles per supertile, supertiles dealt to 8 XCDs
    assert route(flags=flag | GF_MFMA_SPLAT)["kernel"] == WAVE


def test_exp_flavour_precedence_and_defaults():
    assert route(flags=GF_EXACT_FP32 | GF_LIBM_EXP | GF_COMP_EXP | GF_FAST_EXP)["exp"] == EXP_LIBM
    assert route(flags=GF_EXACT_FP32 | GF_COMP_EXP | GF_FAST_EXP)["exp"] == EXP_COMP
    assert route(variant=GF_SPLAT_PROB)["exp"] == EXP_COMP and route(variant=GF_SPLAT_PROB)["prescale"] == 0
    assert route(variant=GF_SPLAT_PROB, flags=GF_FAST_EXP)["prescale"] == 1


@pytest.mark.parametrize("flags", [0, GF_MFMA_SPLAT, GF_MFMA_SPLAT | GF_WORKSPACE_ZEROED | GF_PREPARE_BACKWARD])
def test_the_prob_variant_never_takes_the_matrix_cores(flags):
    for P in (25601, P_of(619), P_of(4097)):
        r = route(variant=GF_SPLAT_PROB, flags=flags, P=P)
        assert r["kernel"] == EXACT_TILE and r["range_flags"] == r["row_layout"] == r["prep_backward"] == r["one_verdict"] == 0


@pytest.mark.parametrize("flags", [0, GF_MFMA_SPLAT])
def test_other_point_counts_and_pts_general_go_to_arbitrary_points(flags):
    for variant in (GF_SPLAT_BASE, GF_SPLAT_PROB):
        for r in (route(variant, flags, N=V - 1), route(variant, flags | GF_PTS_GENERAL)):
            assert r["kernel"] == ARBITRARY and r["verify"] == r["lattice"] == r["range_flags"] == 0
        assert route(variant, flags, N=V - 1)["render_grid"] == min(4096, -(-(V - 1) // 256))
    assert route(N=0)["kernel"] == ARBITRARY and route(N=0)["render_grid"] == 0
    assert route(P=0)["kernel"] == EXACT_TILE and route(P=0)["prep_grid"] == 4096 // 2   # nothing to render on the matrix cores


def test_assume_dense_drops_the_point_scans():
    r = route(flags=GF_PTS_ASSUME_DENSE)
    assert r["kernel"] == WAVE and r["verify"] == r["lattice"] == 0 and r["range_theta_here"] == 1
    assert r["prep_grid"] == r["prep_blocks"]


def test_label_modes():
    r = route(label_mode=GF_LABELS_ARGMAX)   # the argmax epilogue is built into the wave kernel
    assert r["kernel"] == WAVE and r["labels"] == 1
    assert route(label_mode=GF_LABELS_ARGMAX, P=P_of(619), flags=GF_WORKSPACE_ZEROED)["kernel"] == WAVE_LONG
    assert route(label_mode=GF_LABELS_ARGMAX, P=P_of(619))["kernel"] == EXACT_TILE   # ... and into no tile kernel of the matrix cores
    # (the other two modes need the prob variant, which never takes the matrix cores: no call can tell the mode's own term apart)
    for mode in (GF_LABELS_PROB_THRESHOLD, GF_LABELS_PROB_GEOSEM):
        r = route(variant=GF_SPLAT_PROB, label_mode=mode, flags=GF_MFMA_SPLAT)
        assert r["kernel"] == EXACT_TILE and r["labels"] == 1
    assert route(label_mode=GF_LABELS_ARGMAX, flags=GF_PREPARE_BACKWARD)["row_layout"] == 0


def test_argmax_labels_with_the_tile_option_leave_the_matrix_cores(tile_option):
    assert route(label_mode=GF_LABELS_ARGMAX)["kernel"] == EXACT_TILE


@pytest.mark.parametrize("P, zeroed, waves", [
    (25601, True, 2), (65535, False, 2), (65536, False, 4), (P_of(4097), False, 4),   # by P: four waves from 65 536 on
    (P_of(619), True, 4), (P_of(619), False, 2), (P_of(618), True, 2),   # long rows (with their summaries): four
])
def test_records_pass_waves_and_grid(P, zeroed, waves):
    for variant in (GF_SPLAT_BASE, GF_SPLAT_PROB):
        r = route(variant, GF_WORKSPACE_ZEROED if zeroed else 0, P=P)
        blocks = -(-(-(-P // 64)) // waves)   # a workgroup of w waves owns w consecutive words of every bitmask row
        assert (r["prep_waves"], r["prep_blocks"]) == (waves, blocks)
        assert r["prep_grid"] == blocks + 4096 // waves   # ... and 4 096 waves scan the points
    assert route(P=0, N=V - 1)["prep_grid"] == 0


@pytest.mark.parametrize("grid", GRIDS)
def test_row_layout_needs_the_flag_no_labels_and_64_workgroups(grid):
    n = grid[0] * grid[1] * grid[2]
    wave_grid = splat_unit_grid(units(grid))
    enough = wave_grid >= 64   # workgroups 0..63 of the render launch finish the layout
    assert enough == (grid != GRIDS[0])
    for P, zeroed, kernel in ((25601, False, WAVE), (P_of(619), True, WAVE_LONG)):
        z = GF_WORKSPACE_ZEROED if zeroed else 0
        r = route(flags=GF_PREPARE_BACKWARD | z, P=P, N=n, grid=grid)
        assert r["kernel"] == kernel and r["row_layout"] == r["prep_backward"] == enough
        assert route(flags=z, P=P, N=n, grid=grid)["row_layout"] == 0
        assert route(flags=GF_PREPARE_BACKWARD | GF_EXACT_FP32 | z, P=P, N=n, grid=grid)["row_layout"] == 0
        r = route(flags=GF_PREPARE_BACKWARD | z, label_mode=GF_LABELS_ARGMAX, P=P, N=n, grid=grid)
        assert r["kernel"] == kernel and r["row_layout"] == r["prep_backward"] == 0
    assert route(flags=GF_PREPARE_BACKWARD, P=P_of(4097), N=n, grid=grid)["row_layout"] == 0   # no matrix-core backward past 262 144


@pytest.mark.parametrize("grid", GRIDS)
def test_the_backward_counters_start_from_the_grid_the_backward_launches(grid):
    n = grid[0] * grid[1] * grid[2]
    want = splat_unit_grid(units(grid)) // 8
    for flags in (0, GF_PREPARE_BACKWARD, GF_EXACT_FP32):
        r = route(flags=flags, N=n, grid=grid)
        assert r["bwd_counter_init"] == want
        if r["kernel"] == WAVE:
            assert r["render_grid"] == 8 * want and r["tile_counter_init"] == want
    assert [splat_unit_grid(units(g)) for g in GRIDS] == [8, 240, 2048]


def test_refused_calls_name_the_entry_point_that_was_called():
    lib = _lib.load()
    refused = [GF_SPLAT_BASE, 0, 0, 10, V, 18, H, W, 2000] + [None] * 12   # D out of range: refused before any pointer is read
    assert lib.gf_splat_forward_labels(*refused, GF_LABELS_ARGMAX, 0.0, 0, None, None, None, 0, None) == -1
    assert lib.gf_last_error() == b"gf_splat_forward_labels: grid size out of range"
    assert lib.gf_splat_forward(*refused, None, None, 0, None) == -1
    assert lib.gf_last_error() == b"gf_splat_forward: grid size out of range"
    host = (ctypes.c_char * 64)()   # a non-null pointer for every argument: refused on the size before anything is launched
    p = ctypes.addressof(host)
    small = [GF_SPLAT_BASE, 0, 0, 10, V, 18, H, W, D] + [p] * 12
    for mode in (-1, -2, 3):   # (-1 is "no labels" for the route hook only, never for a call that passes a labels pointer)
        assert lib.gf_splat_forward_labels(*small, mode, 0.0, 0, p, p, p, 64, None) == -1
        assert lib.gf_last_error() == b"gf_splat_forward_labels: unknown label mode"
    assert lib.gf_splat_forward_labels(*small, GF_LABELS_ARGMAX, 0.0, 0, p, p, p, 64, None) == -2
    assert lib.gf_last_error().startswith(b"gf_splat_forward_labels: workspace too small (64 < ")


@pytest.mark.gpu
def test_the_route_is_the_body_the_state_block_reports(gpu):
    """Four calls on a 16 x 16 x 16 grid with 200 Gaussians: what the hook says the call takes is what word 1 of the state block
    says rendered it (GF_PATH_*, include/gf_hip.h).  The bitmask-row regimes are held by test_splat_row_regimes_gpu.py."""
    import torch

    from gaussianformer_amd.local_aggregate import splat_forward
    from gaussianformer_amd.synthetic import make_splat_inputs
    path_of = {EXACT_TILE: _lib.GF_PATH_EXACT_TILE, ARBITRARY: _lib.GF_PATH_ARBITRARY, MFMA_TILE: _lib.GF_PATH_MATRIX_CORE,
               WAVE: _lib.GF_PATH_MATRIX_CORE_WAVE, WAVE_LONG: _lib.GF_PATH_MATRIX_CORE_WAVE}
    g = 16
    si = make_splat_inputs("nuscenes_gs25600_solid", seed=11, P=200, H=g, W=g, D=g)
    P = si.means3D.shape[0]
    t = tensors(gpu, si)

    def both(flags=0, drop=0):
        n = g ** 3 - drop
        tensors = [t[0][:n], t[1][:n]] + t[2:]
        state = splat_forward(GF_SPLAT_BASE, *tensors, g, g, g, flags=flags)[4]
        torch.cuda.synchronize(gpu)
        # (splat_forward hands over a zeroed workspace and says so)
        r = route(flags=flags | GF_WORKSPACE_ZEROED, P=P, N=n, grid=(g, g, g))
        return r["kernel"], _lib.SplatState.of(state).path

    for want, (kernel, path) in ((WAVE, both()), (EXACT_TILE, both(GF_EXACT_FP32)), (ARBITRARY, both(drop=1))):
        assert kernel == want and path == path_of[kernel], (want, kernel, path)
    with _lib.option("splat.mfma_tile_kernel", 1):
        kernel, path = both()
    assert kernel == MFMA_TILE and path == path_of[kernel], (kernel, path)
