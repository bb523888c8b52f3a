"""The wave-autonomous matrix-core render kernel's group operand phase (S' rows split between the half-lanes, the box rows as
packed 16-bit compares, the S' residuals by v_fma_mix) against the tile kernel, which forms the same operands its own way: equal
bits on the shapes where the one-hot rows meet ragged edges, partial groups and long rows."""
import numpy as np
import pytest
import torch

from gaussianformer_amd.synthetic import make_splat_inputs

from util import hip_splat_forward, prep

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("config,kw", [
    ("nuscenes_gs144000", dict(P=6000, H=20, W=20, D=16)),            # crowded: many full groups
    ("nuscenes_gs25600_solid", dict(P=700, H=9, W=7, D=4)),          # ragged: partial brick, boxes cut by the grid edges
    ("nuscenes_gs25600_solid", dict(P=90, H=13, W=11, D=12)),        # sparse: mostly partial groups (dead lanes)
    ("nuscenes_gs144000", dict(P=40000, H=64, W=40, D=8)),            # long rows
])
def test_wave_and_tile_kernels_agree_on_the_operand_phase(gpu, config, kw):
    from gaussianformer_amd import _lib
    si = make_splat_inputs(config, seed=7, **kw)
    pi, mi, radii, cov6 = prep(si)
    wave, _, wstate, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
    with _lib.option("splat.mfma_tile_kernel", 1):
        tile, _, tstate, _ = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=_lib.GF_MFMA_SPLAT)
    assert _lib.SplatState.of(wstate).path == _lib.GF_PATH_MATRIX_CORE_WAVE
    assert _lib.SplatState.of(tstate).path == _lib.GF_PATH_MATRIX_CORE
    assert np.isfinite(wave["logits"]).all()
    assert np.array_equal(wave["logits"], tile["logits"])
