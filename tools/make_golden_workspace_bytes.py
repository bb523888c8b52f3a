"""Records tests/golden/workspace_bytes.json: what every ``*_bytes`` entry point returns for the cases of
tests/test_workspace_bytes.py (host code: no GPU needed):

    [GF_LIB=<library>] python tools/make_golden_workspace_bytes.py [--out FILE]

The table says what the workspace layouts' sizes ARE, so it is recorded with the library whose layouts are to be kept: before a
restructuring of the host-side carve-up, build the commit it starts from under another name (``build.build(lib_name=...)``) and
select it with ``GF_LIB``.  Record it with the current library only for an intended change of a layout.  Data only."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_workspace_bytes as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN)
    a = ap.parse_args()
    from gaussianformer_amd import _lib
    data = T.compute(_lib.load())
    for (name, args), nbytes in T.CROSS_CHECK.items():
        assert [list(args), nbytes] in data[name], (name, args, nbytes)
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{name}": [\n' + ",\n".join("  " + json.dumps(row) for row in rows) + "\n ]"
                                   for name, rows in sorted(data.items())) + "\n}\n")
    print(a.out, "recorded with", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
