"""The wave kernel's output stores: a unit inside the grid leaves through the fast path (a uniform base, per-lane offsets computed
once per wave, 16-byte write-through stores issued from inline asm and counted by hand for the next unit's row wait); a unit that
crosses the grid's edge tests every piece; a depth that is no multiple of 4 leaves element by element.  None of that may change a
bit: the reference is the tile kernel (``splat.mfma_tile_kernel``), whose epilogue is its own, compared as int32.  ``out_logits``
is filled with a NaN pattern before each call and no voxel may keep it: together with the equality, every voxel is written.

Every case goes through the records pass too (the tile kernel reads the same records, boxes and bitmask rows)."""
import numpy as np
import pytest
import torch

from gaussianformer_amd import _lib
from gaussianformer_amd.local_aggregate import SplatForwardPlan, splat_forward_labels

from splat_cases import run_plan, same_bits, tensors, wave_equals_tile, wide_radius_scene

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC0BEEF   # a quiet NaN no kernel produces
LOGITS_ARG = 17        # SplatForwardPlan.args: 9 scalars, 8 inputs, then out_logits
FLAGS_ARG = 2


def _plan(si, t, flags=0, offset_floats=0, unzeroed=False):
    plan = SplatForwardPlan(_lib.GF_SPLAT_BASE, *t, si.H, si.W, si.D, flags=flags)
    if offset_floats:
        n = plan.logits.numel()
        buf = torch.empty(n + 64, dtype=torch.float32, device=plan.device)
        lead = ((-buf.data_ptr()) % 64) // 4 + offset_floats     # floats up to a 64-byte boundary, then past it
        plan.logits = buf[lead:lead + n].view(plan.logits.shape)
        assert plan.logits.data_ptr() % 64 == 4 * offset_floats
        plan.args[LOGITS_ARG] = _lib.ptr(plan.logits)
    if unzeroed:
        plan.args[FLAGS_ARG] &= ~_lib.GF_WORKSPACE_ZEROED
    return plan


def _run(plan, tile=False):
    """(logits, SplatState) of one run over the NaN pattern, every voxel written."""
    plan.logits.view(torch.int32).fill_(PATTERN)
    logits, state = run_plan(plan, tile)
    assert not (logits.view(np.int32) == PATTERN).any(), "a voxel was not written"
    return logits, state


def _stores_equal_the_tile_kernels(gpu, si, runs=1, **plan_kw):
    t = tensors(gpu, si)
    tile = _run(_plan(si, t), tile=True)
    wave = _plan(si, t, **plan_kw)
    for _ in range(runs):
        wave_equals_tile(_run(wave), tile)


@pytest.mark.parametrize("shape", [(8, 8, 16), (10, 13, 16), (16, 16, 12), (16, 16, 8), (16, 16, 4), (16, 16, 6)])
def test_logits_equal_the_tile_kernels_bit_for_bit(gpu, shape):
    """8 x 8 x 16: one supertile, every unit inside the grid -- the fast path alone.  10 x 13 x 16: units cross the edge in x and
    in y.  16 x 16 x 12: a depth that is a multiple of 4 whose upper z unit crosses the edge.  16 x 16 x 8 and x 4: one z unit, whole
    and half.  16 x 16 x 6: the element-wise path."""
    H, W, D = shape
    _stores_equal_the_tile_kernels(gpu, wide_radius_scene(61 + H + W + D, 1200, H, W, D))


@pytest.mark.parametrize("shape", [(8, 8, 16), (10, 13, 16)])
@pytest.mark.parametrize("keep_logits", [False, True])
def test_labels_are_the_argmax_of_the_tile_kernels_logits(gpu, shape, keep_logits):
    """Label mode takes its labels from the staged rows: the first maximum of the very values the tile kernel stores."""
    H, W, D = shape
    si = wide_radius_scene(71 + H, 1200, H, W, D)
    t = tensors(gpu, si)
    ref, state = _run(_plan(si, t), tile=True)
    assert state.path == _lib.GF_PATH_MATRIX_CORE
    want = np.argmax(ref, axis=1)
    out = splat_forward_labels(_lib.GF_SPLAT_BASE, *t, H, W, D, keep_logits=keep_logits)
    labels = (out[0] if keep_logits else out).cpu().numpy()
    assert np.array_equal(labels, want)
    if keep_logits:
        same_bits(out[1].cpu().numpy(), ref, "labels instantiation's logits vs tile kernel")


def test_prepared_forward_stores_the_same_logits(gpu):
    """GF_PREPARE_BACKWARD (its own instantiation of the wave kernel) at 10 x 13 x 16."""
    _stores_equal_the_tile_kernels(gpu, wide_radius_scene(81, 1200, 10, 13, 16), flags=_lib.GF_PREPARE_BACKWARD)


def test_long_rows(gpu):
    """P just above 39 552: the long-row instantiation, on 16 x 16 x 16."""
    _stores_equal_the_tile_kernels(gpu, wide_radius_scene(82, 39_600, 16, 16, 16))


def test_second_units_and_the_counted_row_wait(gpu):
    """The smallest square grid of depth 16 with more units than the 8 x CUs resident waves (136 x 136 x 16 = 2 312 units on 256
    CUs): waves take a second unit, whose prefetched bitmask row is waited for by COUNT -- `at most kUnitStores operations
    outstanding` -- behind the first unit's stores.  Three runs on one workspace, each equal to the tile kernel.  A wait count that
    does not match the number of stores issued would show here only with some probability (the row usually lands long before it is
    used); the guard is that the kernel writes the count, where it sets it and in the wait instruction, from one named constant."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    side = 8 * (int(np.floor(np.sqrt(cus))) + 1)
    assert (side // 8) ** 2 * 8 > 8 * cus >= (side // 8 - 1) ** 2 * 8
    _stores_equal_the_tile_kernels(gpu, wide_radius_scene(83, 2000, side, side, 16), runs=3)


def test_output_16_bytes_past_a_64_byte_boundary(gpu):
    """An out_logits view that is only 16-byte aligned: the stores' segments no longer start on 64-byte boundaries; same bits."""
    _stores_equal_the_tile_kernels(gpu, wide_radius_scene(84, 1200, 10, 13, 16), offset_floats=4)


def test_workspace_not_flagged_zeroed(gpu):
    """Without GF_WORKSPACE_ZEROED every wave reads the per-wave verdict words of the flag section, which the records pass writes
    with plain stores."""
    _stores_equal_the_tile_kernels(gpu, wide_radius_scene(85, 1200, 10, 13, 16), unzeroed=True)
