"""Records tests/golden/subm_gemm_digests.json: the SHA-256 of ``Rulebook.apply``'s output bytes on every route of the sparse
convolution's gather-GEMM, for the cases and inputs of tests/test_subm_gemm_digests.py (needs a GPU):

    [GF_LIB=<library>] python tools/make_golden_subm_digests.py [--out FILE]

The digests say what the arithmetic IS, so they are recorded with the library whose arithmetic is to be kept: before a
restructuring of the kernels, build the commit it starts from under another name (``build.build(lib_name=...)``) and select it
with ``GF_LIB``.  Record them with the current library only for an intended change of arithmetic.  Data only."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_subm_gemm_digests as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN)
    a = ap.parse_args()
    from gaussianformer_amd import _lib
    data = {}
    for N, pairs in T.PAIRS.items():
        for cin, cout in T.CHANNELS:
            total, digests = T.compute(N, cin, cout)
            assert total == pairs, (N, total)
            data[T.case_name(N, cin, cout)] = digests
    with open(a.out, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out, "recorded with", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
