"""Records tests/golden/splat_scene_digests.json: the SHA-256 of every shared splat scene (means3D, scales, cov3D, opacities,
semantics and the prepared means3D_int, radii, cov6) at each (arguments, seeds) combination a test uses, as
tests/test_splat_cases.py computes them (CPU only); the crowded scene's entry also holds ``claimed`` and ``may_take``:

    python tools/make_golden_splat_scene_digests.py [--scenes MODULE] [--out FILE]

The digests say what the tests' inputs ARE, so they are recorded with the builders whose values are to be kept.  The committed
file was recorded at the commit before tests/splat_cases.py, with ``--scenes`` naming a module that passed the three calls on to
the builders the test files then had each for themselves (``_inputs`` / ``_covering_inputs``, the crowded scene written out in
tests/test_splat_shared_list_gpu.py and ``_crowded_inputs``, the epilogue test's ``_inputs``).  The covering scene of
64 * kWRow Gaussians is included: it takes under a second.  Data only."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_splat_cases as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="splat_cases", help="module with covering_scene, crowded_supertile_scene and wide_radius_scene")
    ap.add_argument("--out", default=T.GOLDEN)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        json.dump(T.compute(importlib.import_module(a.scenes)), f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out, "recorded")


if __name__ == "__main__":
    main()
