"""Generates tests/golden/ffn.npz by executing the REFERENCE's ``AsymmetricFFN``, unmodified, on the CPU
(model/encoder/gaussian_encoder/ffn_module.py; needs the reference tree, no GPU):

    python tools/make_golden_ffn.py [--reference ROOT]      (default: $GF_REFERENCE_ROOT)

``mmengine`` is replaced by the stand-ins of tests/ref_shim.py; the three ``mmcv`` names the file imports
(``mmcv.cnn.build_activation_layer``, ``mmcv.cnn.build_norm_layer``, ``mmcv.cnn.bricks.drop.build_dropout``) get stand-ins
here, next to them, that build the torch layers mmcv would.  The reference's package ``__init__`` files are not executed.

Per family of tests/ffn_ref.py's FAMILIES the module is built with the family's constructor arguments,
``ffn_ref.fixed_weights`` is loaded with ``strict=True``, and the fixture records, from ``eval()`` mode: the input (64 rows
with the planted ones), the seed, the float32 output and the output of the same module after ``.double()`` on the same input
-- of the FFN alone and of the FFN followed by what follows it in the family's ``operation_order`` (``"add"`` of the block's
input for ``prob``, then an ``nn.LayerNorm(128)`` with the seeded post-norm weights) -- and the state_dict's keys with their
shapes.  Data only; no weights (they are regenerated from ``fixed_weights``)."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ffn_ref as ref  # noqa: E402
import ref_shim  # noqa: E402


def install_mmcv_stubs():
    """The three builders, for the layer types the shipped configs name."""
    def build_activation_layer(cfg):
        cfg = dict(cfg)
        return {"ReLU": nn.ReLU, "GELU": nn.GELU}[cfg.pop("type")](**cfg)

    def build_norm_layer(cfg, num_features, postfix=""):
        cfg = dict(cfg)
        assert cfg.pop("type") == "LN"
        cfg.pop("requires_grad", None)
        return "ln" + str(postfix), nn.LayerNorm(num_features, **cfg)

    def build_dropout(cfg, default_args=None):
        cfg = dict(cfg)
        assert cfg.pop("type") == "Dropout"
        return nn.Dropout(p=cfg.pop("drop_prob", 0.5), **cfg)

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m._gf_stub = True
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m
    if "mmcv" in sys.modules and not getattr(sys.modules["mmcv"], "_gf_stub", False):
        raise RuntimeError("a real mmcv is installed: the stubs are not needed")
    drop = mod("mmcv.cnn.bricks.drop", build_dropout=build_dropout)
    bricks = mod("mmcv.cnn.bricks", drop=drop)
    cnn = mod("mmcv.cnn", build_activation_layer=build_activation_layer, build_norm_layer=build_norm_layer, bricks=bricks)
    mod("mmcv", cnn=cnn)


def load_reference(root):
    """The reference's class, from its file as it is."""
    ref_shim.install_stubs()
    install_mmcv_stubs()

    def namespace(name, path):
        m = types.ModuleType(name)
        m.__path__ = [path]
        m.__package__ = name
        sys.modules[name] = m

    pkg = "gf_reference_ffn"
    namespace(pkg, os.path.join(root, "model"))
    namespace(pkg + ".encoder", os.path.join(root, "model", "encoder"))
    namespace(pkg + ".encoder.gaussian_encoder", os.path.join(root, "model", "encoder", "gaussian_encoder"))
    return importlib.import_module(pkg + ".encoder.gaussian_encoder.ffn_module").AsymmetricFFN


def family(cls, name, seed):
    shapes = ref.family_shapes(name)
    cin = shapes["layers.0.0.weight"][1]
    weights = ref.fixed_weights(cin, "pre_norm.weight" in shapes, "identity_fc.weight" in shapes, seed=seed)
    module = cls(**ref.FAMILIES[name])
    module.load_state_dict(ref.module_state(weights), strict=True)
    module.eval()
    norm = nn.LayerNorm(ref.E)
    norm.load_state_dict({"weight": weights["norm.weight"], "bias": weights["norm.bias"]}, strict=True)
    x = ref.planted(ref.fixed_input(ref.GOLDEN_ROWS, cin, seed))
    add = ref.FOLLOWED_BY_ADD[name]

    def run(x):
        out = module(x)
        return out, norm(out + x if add else out)
    with torch.no_grad():
        ffn32, block32 = run(x)
        module.double()
        norm.double()
        ffn64, block64 = run(x.double())
    sd = module.state_dict()
    d = {"keys": np.array(list(sd.keys())), "shapes": np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], dtype=np.int64),
         "seed": np.int64(seed), "input": x.numpy(), "ffn32": ffn32.numpy(), "ffn64": ffn64.numpy(), "block32": block32.numpy(),
         "block64": block64.numpy()}
    return {f"{name}.{k}": v for k, v in d.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GF_REFERENCE_ROOT"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ffn.npz"))
    a = ap.parse_args()
    if not a.reference or not os.path.isfile(os.path.join(a.reference, "model", "encoder", "gaussian_encoder", "ffn_module.py")):
        sys.exit("the reference tree is needed: --reference ROOT or GF_REFERENCE_ROOT")
    cls = load_reference(a.reference)
    data = {}
    for seed, name in enumerate(ref.FAMILIES):
        data.update(family(cls, name, 300 + seed))
    np.savez_compressed(a.out, **data)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
