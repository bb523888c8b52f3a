"""Records tests/golden/row_support_digests.json: the SHA-256 of the row ops' seeded weights, inputs, masks and kink-filter
survivors, as tests/test_row_support_digests.py computes them (CPU only):

    python tools/make_golden_row_support_digests.py [--out FILE]

The digests say what the tests' inputs ARE, so they are recorded with the helpers whose values are to be kept: before a
restructuring of the test support, run this in a checkout of the commit it starts from and copy the file over.  Data only."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_row_support_digests as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        json.dump(T.compute(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out, "recorded")


if __name__ == "__main__":
    main()
