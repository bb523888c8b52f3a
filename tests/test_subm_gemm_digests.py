"""The sparse convolution's gather-GEMM, output bit for output bit: every route of ``Rulebook.apply`` -- the three operand formats
(two f16 terms, three bf16 terms, f32 MFMA), runs of tiles and single tiles, a rulebook sized by a capacity -- against SHA-256
digests of the outputs recorded in tests/golden/subm_gemm_digests.json (tools/make_golden_subm_digests.py).  The other tests
hold the routes to the fp64 definition and to each other; only this one notices a change of the arithmetic that stays inside
those bounds (a reordered chain, another term order), which a restructuring of the kernels must not bring.

The inputs come from integer draws alone (numpy's generator, no torch generator): 24-bit mantissas times powers of two, features
of magnitude O(1), weights O(0.1).  Batch 1, grid (10, 10, 6), K = 3:
    N = 3000: 311 574 pairs = 2434 times 128, >= 27 * 32, so the run walk; segments of 9 671 ... 18 328 pairs, none a multiple
              of 128, so every last tile is ragged; their last runs hold 1, 4, 5, 6, 7 or 8 tiles (ceil(pairs / 128) mod 8 over the 27
              segments is {0, 1, 4, 5, 6, 7}: short runs and full ones);
    N = 300:  3 326 pairs = 25 times 128, the tile walk only; segments of 86 ... 478 pairs, some shorter than one tile (waves
              wholly past the segment end, padded index lanes).
Channels: (128, 128) = all 128 output channels per workgroup; (64, 32) = one 32-column group; (32, 128) = two 64-channel slices."""
import contextlib
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from test_subm_conv import _points

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "subm_gemm_digests.json")
SHAPE, K = (10, 10, 6), 3
PAIRS = {3000: 311574, 300: 3326}
CHANNELS = [(128, 128), (64, 32), (32, 128)]
FORMATS = {"f16x2": (), "bf16x3": ("subm.bf16x3",), "f32_mfma": ("subm.f32_mfma",)}


def case_name(N, cin, cout):
    return f"N{N}.{cin}x{cout}"


def compute(N, cin, cout):
    """(pair count, {route: digest}) of one case on the GPU."""
    from gaussianformer_amd import _lib
    from gaussianformer_amd.sparse_conv import Rulebook
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(21)
    idx = _points(rng, N, 1, SHAPE).to(dev)
    feat = rng.integers(-2 ** 23, 2 ** 23, (N, cin)) * 2.0 ** rng.integers(-30, -17, (N, cin))
    weight = rng.integers(-2 ** 23, 2 ** 23, (K ** 3, cin, cout)) * 2.0 ** rng.integers(-34, -23, (K ** 3, cin, cout))
    feat, weight = torch.from_numpy(feat.astype(np.float32)).to(dev), torch.from_numpy(weight.astype(np.float32)).to(dev)
    rb = Rulebook(idx, 1, SHAPE, K)
    runs_apply = rb.total // 128 >= K ** 3 * 32
    routes = {name: (rb, opts) for name, opts in FORMATS.items()}
    if runs_apply:   # the same again with one tile per workgroup (f32 MFMA has no run form)
        routes.update({name + ".tile_gemm": (rb, opts + ("subm.tile_gemm",)) for name, opts in FORMATS.items() if name != "f32_mfma"})
    routes["f16x2.capacity"] = (Rulebook(idx, 1, SHAPE, K, pair_capacity=128 * N), ())
    out = {}
    for name, (book, opts) in routes.items():
        with contextlib.ExitStack() as stack:
            for o in opts:
                stack.enter_context(_lib.option(o, 1))
            out[name] = hashlib.sha256(book.apply(feat, weight).cpu().numpy().tobytes()).hexdigest()
    return rb.total, out


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("N", list(PAIRS))
def test_subm_gemm_output_bits_are_the_recorded_ones(gpu, N, cin, cout):
    total, got = compute(N, cin, cout)
    assert total == PAIRS[N]
    assert (total // 128 >= 864) == (N == 3000)          # 27 offsets * 4 runs of 8 tiles: where the run walk starts
    with open(GOLDEN) as f:
        want = json.load(f)[case_name(N, cin, cout)]
    assert sorted(got) == sorted(want)
    differ = [r for r in got if got[r] != want[r]]
    assert not differ, (f"{case_name(N, cin, cout)}: the output bits of {differ} are not the recorded ones.  The gather-GEMM's arithmetic changed.  "
                        "Regenerate tests/golden/subm_gemm_digests.json (tools/make_golden_subm_digests.py) ONLY if that change is intended.")
