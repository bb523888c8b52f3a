"""The wave-autonomous matrix-core render kernel's group operand phase (S' rows split between the half-lanes, the box rows as
packed 16-bit compares, the S' residuals by v_fma_mix) against the tile kernel, which forms the same operands its own way: equal
bits on the shapes where the one-hot rows meet ragged edges, partial groups and long rows."""
import pytest

from gaussianformer_amd import _lib
from gaussianformer_amd.synthetic import make_splat_inputs

from splat_cases import run_route, tensors, wave_equals_tile

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("config,kw", [
    ("nuscenes_gs144000", dict(P=6000, H=20, W=20, D=16)),            # crowded: many full groups
    ("nuscenes_gs25600_solid", dict(P=700, H=9, W=7, D=4)),          # ragged: partial brick, boxes cut by the grid edges
    ("nuscenes_gs25600_solid", dict(P=90, H=13, W=11, D=12)),        # sparse: mostly partial groups (dead lanes)
    ("nuscenes_gs144000", dict(P=40000, H=64, W=40, D=8)),            # long rows
])
def test_wave_and_tile_kernels_agree_on_the_operand_phase(gpu, config, kw):
    si = make_splat_inputs(config, seed=7, **kw)
    t = tensors(gpu, si)
    wave_equals_tile(run_route(t, si, _lib.GF_MFMA_SPLAT), run_route(t, si, _lib.GF_MFMA_SPLAT, tile=True))
