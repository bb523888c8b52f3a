"""Records tests/golden/encoder_orders.json: the ``encoder`` settings (``operation_order`` and every module's config dict) of
the reference's shipped config files, as data.

    python tools/make_golden_encoder.py /path/to/GaussianFormer

The config files are plain Python that assigns dicts; a file's ``_base_`` list names the files it inherits from.  This tool
only ``exec``s them and merges the dicts the way the reference's config loader does (a child dict is merged into its base's
key by key; a child dict with ``_delete_=True`` replaces it), then dumps ``model["encoder"]``.  Nothing of the reference is
imported and no module is built."""
import json
import os
import sys

CONFIGS = {
    "nuscenes_gs144000": "config/nuscenes_gs144000.py",
    "nuscenes_gs25600_solid": "config/nuscenes_gs25600_solid.py",
    "prob/nuscenes_gs6400": "config/prob/nuscenes_gs6400.py",
    "prob/nuscenes_gs12800": "config/prob/nuscenes_gs12800.py",
    "prob/nuscenes_gs25600": "config/prob/nuscenes_gs25600.py",
}
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "encoder_orders.json")


def merge(base, child):
    """``child`` over ``base``: dicts key by key, ``_delete_=True`` replaces, everything else overwrites."""
    if not isinstance(child, dict):
        return child
    out = dict(base) if isinstance(base, dict) and not child.get("_delete_") else {}
    for k, v in child.items():
        if k != "_delete_":
            out[k] = merge(out.get(k), v)
    return out


def load(path):
    scope = {}
    with open(path) as f:
        exec(compile(f.read(), path, "exec"), scope)
    own = {k: v for k, v in scope.items() if not k.startswith("__") and k != "_base_"}
    merged = {}
    for rel in scope.get("_base_", []):
        merged = merge(merged, load(os.path.normpath(os.path.join(os.path.dirname(path), rel))))
    return merge(merged, own)


def main(root):
    out = {}
    for name, rel in CONFIGS.items():
        enc = load(os.path.join(root, rel))["model"]["encoder"]
        out[name] = {k: v for k, v in enc.items() if k != "type"}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, enc in out.items():
        print(name, len(enc["operation_order"]), "ops,", "spconv:", (enc["spconv_layer"] or {}).get("use_multi_layer", False))


if __name__ == "__main__":
    main(sys.argv[1])
