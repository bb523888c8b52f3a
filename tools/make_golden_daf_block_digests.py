"""Records tests/golden/daf_block_digests.json: the SHA-256 of the output bytes of the deformable block's fused and prepare
kernels, forward and backward, for the cases and inputs of tests/test_daf_block_digests_gpu.py (needs a GPU):

    [GF_LIB=<library>] python tools/make_golden_daf_block_digests.py [--out FILE]

The digests say what the arithmetic IS, so they are recorded with the library whose arithmetic is to be kept: before a
restructuring of the kernels, build the commit it starts from under another name (``build.build(lib_name=...)``) and select it
with ``GF_LIB``.  Record them with the current library only for an intended change of arithmetic.  Every case runs twice, and an
output whose two digests differ is refused: only outputs that are reproducible on one library can pin another.  Data only."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_daf_block_digests_gpu as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN)
    a = ap.parse_args()
    from gaussianformer_amd import _lib
    data = {}
    for prefix, cases, compute in (("fused.", T.FUSED, T.compute_fused), ("prepare.", T.PREPARE, T.compute_prepare)):
        for name in sorted(cases):
            first, second = compute(name), compute(name)
            unstable = [k for k in sorted(first) if first[k] != second[k]]
            if unstable:
                sys.exit(f"{prefix}{name}: {unstable} differ between two runs of the same library: not recorded, nothing written")
            data[prefix + name] = first
    with open(a.out, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out, "recorded with", _lib.LIB_PATH, "--", sum(len(v) for v in data.values()), "digests")


if __name__ == "__main__":
    main()
