"""Generates tests/golden/anchor_embed.npz by executing the REFERENCE's ``SparseGaussian3DEncoder``, unmodified, on the CPU
(model/encoder/gaussian_encoder/anchor_encoder_module.py with the utils.py / model/utils/safe_ops.py it imports; needs the
reference tree, no GPU):

    python tools/make_golden_anchor_embed.py [--reference ROOT]      (default: $GF_REFERENCE_ROOT)

``mmengine`` is replaced by the stand-ins of tests/ref_shim.py, and the reference's package ``__init__`` files are not
executed: its packages are entered into ``sys.modules`` as bare namespaces over the reference's directories.

Per family of tests/anchor_embed_ref.py's FAMILIES (embed_dims 128, 96 rows each) the module is built with the family's
constructor keys, ``anchor_embed_ref.fixed_weights`` is loaded with ``strict=True``, and the fixture records the input, the
float32 output, the output of the same module after ``.double()`` on the same input, the state_dict's keys with their
shapes, and the reference's own float32 gradients of a fixed weighted sum of the output (``anchor_embed_ref.output_weights``)
with respect to the input and to every parameter but the seven square weights (those alone would be 1.4 MB).  Data only; no
weights (they are regenerated from ``fixed_weights``)."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import anchor_embed_ref as ref  # noqa: E402
import ref_shim  # noqa: E402


def load_reference(root):
    """The reference's class, from its file as it is."""
    ref_shim.install_stubs()

    def namespace(name, path):
        m = types.ModuleType(name)
        m.__path__ = [path]
        m.__package__ = name
        sys.modules[name] = m

    pkg = "gf_reference_anchor"
    namespace(pkg, os.path.join(root, "model"))
    namespace(pkg + ".utils", os.path.join(root, "model", "utils"))
    namespace(pkg + ".encoder", os.path.join(root, "model", "encoder"))
    namespace(pkg + ".encoder.gaussian_encoder", os.path.join(root, "model", "encoder", "gaussian_encoder"))
    return importlib.import_module(pkg + ".encoder.gaussian_encoder.anchor_encoder_module").SparseGaussian3DEncoder


def planted(x, opa, S):
    """Rows that a random draw does not reach: zeros, tiny, saturated semantics, far-away means."""
    x = x.clone()
    x[0] = 0.0
    x[1] = 1e-30
    if S:
        x[2, 10 + opa:10 + opa + S] = 80.0
        x[3, 10 + opa:10 + opa + S] = -80.0
    x[4, 0:3] = 1e4
    x[5, 0:3] = -1e4
    return x


def family(cls, name, cfg, seed):
    opa, S = int(cfg["include_opa"]), cfg["semantic_dim"] or 0
    module = cls(embed_dims=128, **cfg)
    module.load_state_dict(ref.fixed_weights(bool(opa), S, seed=seed), strict=True)
    x = planted(ref.fixed_input(ref.GOLDEN_ROWS, 10 + opa + S, seed), opa, S)
    xg = x.clone().requires_grad_(True)
    out32 = module(xg)
    (out32 * ref.output_weights(out32.shape, torch.float32)).sum().backward()
    grads = {"grad32.input": xg.grad.numpy()}
    for k, p in module.named_parameters():
        if tuple(p.shape) != (128, 128):
            grads["grad32." + k] = p.grad.numpy().copy()
    with torch.no_grad():
        out64 = module.double()(x.double())
    sd = module.state_dict()
    d = {"keys": np.array(list(sd.keys())), "shapes": np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], dtype=np.int64),
         "seed": np.int64(seed), "input": x.numpy(), "out32": out32.detach().numpy(), "out64": out64.numpy(), **grads}
    return {f"{name}.{k}": v for k, v in d.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GF_REFERENCE_ROOT"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "anchor_embed.npz"))
    a = ap.parse_args()
    if not a.reference or not os.path.isfile(os.path.join(a.reference, "model", "encoder", "gaussian_encoder", "anchor_encoder_module.py")):
        sys.exit("the reference tree is needed: --reference ROOT or GF_REFERENCE_ROOT")
    cls = load_reference(a.reference)
    data = {}
    for seed, (name, cfg) in enumerate(ref.FAMILIES.items()):
        data.update(family(cls, name, cfg, 200 + seed))
    np.savez_compressed(a.out, **data)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
