"""tests/splat_cases.py on the CPU: its constants against the source lines they name, its scenes against recorded SHA-256 digests
(tests/golden/splat_scene_digests.json, recorded by tools/make_golden_splat_scene_digests.py with the builders the splat tests had
each for themselves, so the shared scenes are those inputs bit for bit), ``same_bits`` on hand-made arrays, and the geometry
helpers and the route hook at hand-computed cases."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import splat_cases as sc
from gaussianformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "splat_scene_digests.json")

# every (arguments, seeds) combination a test builds a shared scene with
WAVE_INVARIANTS = [(P, H, W, D, 100 + P, 7 * P + H, False) for H, W, D in [(16, 16, 16), (12, 20, 8), (8, 8, 4)] for P in (1, 31, 33, 200, 64)]
RECORD_FETCH = [(P, H, W, D, 300 + P % 1000, 11 * P + H, True)
                for P, H, W, D in [(P, H, W, D) for H, W, D in [(12, 20, 8), (16, 16, 16)] for P in (1, 31, 33, 64)] + [(sc.SHORT_ROW_P, 16, 16, 16)]]
CROWDED = [(53, 54), (63, 64)]
SIDE = 136   # test_second_units_and_the_counted_row_wait's grid on the 256 compute units of an MI355X
WIDE = ([(61 + H + W + D, 1200, H, W, D) for H, W, D in [(8, 8, 16), (10, 13, 16), (16, 16, 12), (16, 16, 8), (16, 16, 4), (16, 16, 6)]]
        + [(71 + H, 1200, H, W, D) for H, W, D in [(8, 8, 16), (10, 13, 16)]]
        + [(81, 1200, 10, 13, 16), (82, 39_600, 16, 16, 16), (83, 2000, SIDE, SIDE, 16), (84, 1200, 10, 13, 16), (85, 1200, 10, 13, 16)])


def _digest(si, prepped):
    _, mi, radii, cov6 = prepped
    h = hashlib.sha256()
    for a in (si.means3D, si.scales, si.cov3D, si.opacities, si.semantics, mi, radii, cov6):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def compute(scenes=sc):
    """``{scene(arguments): digest}`` of ``scenes``' three builders; the crowded scene's entry holds its two counts as well."""
    from util import prep
    out = {}
    for a in WAVE_INVARIANTS + RECORD_FETCH:
        out[f"covering_scene{a}"] = _digest(*scenes.covering_scene(*a))
    for a in CROWDED:
        si, claimed, may_take = scenes.crowded_supertile_scene(*a)
        out[f"crowded_supertile_scene{a}"] = dict(sha256=_digest(si, prep(si)), claimed=claimed, may_take=may_take)
    for a in WIDE:
        si = scenes.wide_radius_scene(*a)
        out[f"wide_radius_scene{a}"] = _digest(si, prep(si))
    return out


def test_scenes_are_the_recorded_ones():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = compute()
    assert sorted(got) == sorted(want)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, (f"{differ}: not the recorded inputs.  The digests were taken from the builders the splat tests had before they "
                        "shared tests/splat_cases.py; regenerate the file ONLY if a scene is meant to change.")


def test_constants_are_their_source_lines():
    for name, table in sc.CONSTANTS.items():
        with open(os.path.join(ROOT, "gaussianformer_amd", "csrc", name)) as f:
            text = f.read()
        for k, v in table.items():
            found = re.findall(rf"^constexpr int {k} = (\d+);", text, flags=re.M)
            assert found == [str(v)], (name, k, v, found)
            assert getattr(sc.K, k) == v
    assert sc.SHORT_ROW_P == 64 * sc.K.kWRow == 39552


def test_route_words_are_the_structs_fields_in_order():
    with open(os.path.join(ROOT, "gaussianformer_amd", "csrc", "splat_fwd.hip")) as f:
        text = f.read()
    body = re.search(r"struct ForwardRoute \{(.*?)\};", text, flags=re.S).group(1)
    fields = [w for decl in re.findall(r"(?:int|uint32_t) ([^;]+);", body) for w in re.split(r",\s*", decl.strip())]
    assert tuple(fields) == sc.WORDS
    kernels = re.search(r"enum RenderKernel \{([^}]*)\}", text).group(1)
    assert [k.split("=")[0].strip() for k in kernels.split(",")] == ["kRenderExactTile", "kRenderArbitrary", "kRenderMfmaTile", "kRenderMfmaWave", "kRenderMfmaWaveLong"]
    assert (sc.EXACT_TILE, sc.ARBITRARY, sc.MFMA_TILE, sc.WAVE, sc.WAVE_LONG) == (0, 1, 2, 3, 4)
    # ... and the order tests/test_splat_route.py has held its expectations against since the hook exists
    assert sc.WORDS == (
        "kernel", "labels", "prep_backward", "exp", "prep_waves", "prep_blocks", "prep_grid", "verify", "lattice", "prescale",
        "range_theta_here", "range_flags", "one_verdict", "summaries", "row_layout", "tile_counter_init", "bwd_counter_init", "render_grid")


def test_same_bits():
    a = np.array([[1.0, -2.5, 0.0], [3.0, 0.0, 7.0]], dtype=np.float32)
    sc.same_bits(a, a.copy(), "equal")
    sc.same_bits(a.view(np.int32), a.copy(), "an int32 view against floats")
    b = a.copy()
    b[1, 1] = -0.0
    assert np.array_equal(a, b)
    with pytest.raises(AssertionError, match=r"first at \(1, 1\): 0x00000000 vs 0x80000000"):
        sc.same_bits(a, b, "+0 against -0")
    sc.same_bits(a, b, "+0 against -0", signed_zero_ok=True)
    b[0, 1] = np.nextafter(np.float32(-2.5), np.float32(0))
    with pytest.raises(AssertionError, match=r"1 values of 6 differ, the first at \(0, 1\): 0xc0200000 vs 0xc01fffff"):
        sc.same_bits(a, b, "one ulp, next to a signed zero", signed_zero_ok=True)
    nan = np.array([0x7FC00000, 0x7FC0BEEF], dtype=np.int32).view(np.float32)
    assert not np.array_equal(nan, nan.copy())
    sc.same_bits(nan, nan.copy(), "identical NaN payloads")
    with pytest.raises(AssertionError, match=r"first at \(1,\): 0x7fc0beef vs 0x7fc00000"):
        sc.same_bits(nan, nan[[0, 0]], "different NaN payloads")
    with pytest.raises(AssertionError, match="shape"):
        sc.same_bits(a, a[:1], "shape")
    with pytest.raises(AssertionError):
        sc.same_bits(a, a.astype(np.float64), "another type")


def test_units():
    assert sc.units((96, 96, 32)) == 2304 and sc.units((40, 36, 16)) == 200 and sc.units((100, 92, 64)) == 4992
    assert sc.units((8, 8, 8)) == 4 and sc.units((9, 8, 9)) == 16


def test_range_bounds():
    """Sigma^-1 = diag(4, 1, 0.25) with xy = 0.5, radius 2 on a grid that does not clip it, steps of 0.5: the overflow bound is
    log2(e) / 2 x trace x (2.5^2 + 2.5^2 + 3.5^2); the accuracy bound's Q is the form at (0.75, 0.75, 1.75) with every entry
    positive = 2.25 + 0.5625 + 0.765625 + 2 x 0.28125."""
    cov6 = np.array([[4.0, 1.0, 0.25, -0.5, 0.0, 0.0]], dtype=np.float32)
    bound, near = sc.range_bounds(cov6, np.array([2]), 16, 16, 16)
    assert bound[0] == pytest.approx(0.7213475204444817 * 5.25 * 24.75, rel=1e-12)
    assert near[0] == pytest.approx(0.7213475204444817 * (4.3 + np.sqrt(4.140625)) ** 2, rel=1e-12)
    # a radius beyond the grid counts as the grid's extent
    assert sc.range_bounds(cov6, np.array([100]), 4, 6, 8)[0][0] == pytest.approx(0.7213475204444817 * 5.25 * (3.5 ** 2 + 4.5 ** 2 + 6.5 ** 2), rel=1e-12)


def test_integer_boxes():
    mi = np.array([[0, 5, 3], [7, 7, 7], [2, 2, 2]], dtype=np.int32)
    lo, hi = sc.integer_boxes(mi, np.array([1, 100, 2], dtype=np.int32), 8, 8, 4)
    assert lo.tolist() == [[0, 4, 2], [0, 0, 0], [0, 0, 0]] and hi.tolist() == [[2, 7, 4], [8, 8, 4], [5, 5, 4]]


def test_splat_route_at_the_short_rows_end():
    for P, kernel in ((sc.SHORT_ROW_P, sc.WAVE), (sc.SHORT_ROW_P + 1, sc.WAVE_LONG)):
        r = sc.splat_route(_lib.GF_SPLAT_BASE, _lib.GF_WORKSPACE_ZEROED, sc.NO_LABELS, P, 16 ** 3, (16, 16, 16))
        assert list(r) == list(sc.WORDS) and r["kernel"] == kernel and r["summaries"] == (kernel == sc.WAVE_LONG)
