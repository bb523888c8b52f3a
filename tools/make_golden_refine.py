"""Generates tests/golden/refine.npz by executing the REFERENCE's two refinement modules, unmodified, on the CPU
(model/encoder/gaussian_encoder/refine_module.py and refine_module_v2.py with the utils.py / model/utils/safe_ops.py they
import; needs the reference tree, no GPU):

    python tools/make_golden_refine.py [--reference ROOT]      (default: $GF_REFERENCE_ROOT)

``mmengine`` (registry, BaseModule) and ``mmcv.cnn.Scale`` are replaced by stand-ins of this tool's own, and the reference's
package ``__init__`` files are not executed: its packages are entered into ``sys.modules`` as bare namespaces over the
reference's directories, so only the four files named above run.

Per family of tests/refine_ref.py's FAMILIES (solid, gs144000, prob; embed_dims 32, bs 2, 96 anchors each) the fixture holds the
state_dict and its key list, the three inputs, every output, and the gradients of a fixed weighted sum of the outputs
(refine_ref.fixed_weights) with respect to instance_feature, anchor and every parameter (anchor_embed's gradient equals instance_feature's).  Data only."""
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
import refine_ref  # noqa: E402

EMBED, BS, ANCHORS = 32, 2, 96


def load_reference(root):
    """The reference's two module classes, from its files as they are."""
    def namespace(name, path=None):
        m = types.ModuleType(name)
        if path is not None:
            m.__path__ = [path]
        sys.modules[name] = m
        return m

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    class BaseModule(nn.Module):
        def __init__(self, init_cfg=None):
            super().__init__()

    class Scale(nn.Module):   # mmcv.cnn.Scale: a learnable factor
        def __init__(self, scale=1.0):
            super().__init__()
            self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float))

        def forward(self, x):
            return x * self.scale

    namespace("mmengine", "")
    namespace("mmengine.registry").MODELS = _Registry()
    namespace("mmengine.model").BaseModule = BaseModule
    namespace("mmcv", "")
    namespace("mmcv.cnn").Scale = Scale
    pkg = "gf_reference_model"
    namespace(pkg, os.path.join(root, "model"))
    namespace(pkg + ".utils", os.path.join(root, "model", "utils"))
    namespace(pkg + ".encoder", os.path.join(root, "model", "encoder"))
    namespace(pkg + ".encoder.gaussian_encoder", os.path.join(root, "model", "encoder", "gaussian_encoder"))
    v1 = importlib.import_module(pkg + ".encoder.gaussian_encoder.refine_module")
    v2 = importlib.import_module(pkg + ".encoder.gaussian_encoder.refine_module_v2")
    return {1: v1.SparseGaussian3DRefinementModule, 2: v2.SparseGaussian3DRefinementModuleV2}


def family(classes, name, cfg, seed):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    kwargs = {k: v for k, v in cfg.items() if k != "version"}
    # the extra keys the configs pass, which both modules swallow
    module = classes[cfg["version"]](embed_dims=EMBED, phi_activation="sigmoid", xyz_coordinate="cartesian", **kwargs)
    with torch.no_grad():   # away from the initial state: LayerNorm and Scale would otherwise be the identity
        for p in module.parameters():
            p.add_(torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)) * 0.1)
    D = module.output_dim
    leaf = lambda a: torch.tensor(a.astype(np.float32), requires_grad=True)
    feat = leaf(rng.standard_normal((BS, ANCHORS, EMBED)))
    embed = leaf(rng.standard_normal((BS, ANCHORS, EMBED)))
    anchor = leaf(np.concatenate([rng.uniform(-3.0, 3.0, (BS, ANCHORS, 3)), rng.standard_normal((BS, ANCHORS, D - 3))], axis=-1))
    anchor_out, g = module(feat, anchor, embed)
    outs = dict(anchor_out=anchor_out, **{k: v for k, v in g._asdict().items() if v is not None})
    refine_ref.weighted_sum(outs, refine_ref.fixed_weights(outs)).backward()
    d = {"keys": np.array(list(module.state_dict().keys())), "instance_feature": feat.detach().numpy(),
         "anchor": anchor.detach().numpy(), "anchor_embed": embed.detach().numpy(),
         "grad.instance_feature": feat.grad.numpy(), "grad.anchor": anchor.grad.numpy()}
    for k, v in module.state_dict().items():
        d["state." + k] = v.numpy()
    for k, p in module.named_parameters():
        d["grad.param." + k] = p.grad.numpy()
    for k, v in outs.items():
        d["out." + k] = v.detach().numpy()
    return {f"{name}.{k}": v for k, v in d.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GF_REFERENCE_ROOT"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "refine.npz"))
    a = ap.parse_args()
    if not a.reference or not os.path.isfile(os.path.join(a.reference, "model", "encoder", "gaussian_encoder", "refine_module.py")):
        sys.exit("the reference tree is needed: --reference ROOT or GF_REFERENCE_ROOT")
    classes = load_reference(a.reference)
    data = {}
    for seed, (name, cfg) in enumerate(refine_ref.FAMILIES.items()):
        data.update(family(classes, name, cfg, 100 + seed))
    np.savez_compressed(a.out, **data)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
