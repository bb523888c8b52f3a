"""Record the farthest-point-sampling calls the reference's own GaussianLifterV2 makes -> tests/golden/lifter_fps.npz.

Imports model/lifter/gaussian_lifter_v2.py from the reference tree UNMODIFIED, under a synthetic package whose __init__
files are not executed, with this tool's own minimal stand-ins for the third-party names it and its imports need
(``mmseg.registry.MODELS``, ``mmengine.model.BaseModule``, ``jaxtyping``).  The module's ``farthest_point_sampling``
(bound by ``from pointops import ...`` at :9-12) is replaced by a capturing function that records ``scan``, ``offset`` and
``new_offset`` (values and dtypes) and answers with the numpy oracle (tests/fps_ref.py).  Runs on the CPU at reduced size
(6 x 27 x 50 feature maps, num_anchor 1 500, 128 depth bins, random_sampling=False as in config/prob/nuscenes_gs*.py)
through both the default path and the benchmarking=True three-segment path (:233-251).

    python tools/make_golden_lifter_fps.py [reference_root]
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fps_ref  # noqa: E402

REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GF_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "lifter_fps.npz")


def install_stubs():
    class Registry:
        def register_module(self, *a, **k):
            return (lambda cls: cls) if not a or not isinstance(a[0], type) else a[0]

        def build(self, cfg):
            raise RuntimeError("not needed: the lifter is built without an initializer")

    class BaseModule(nn.Module):
        def __init__(self, init_cfg=None):
            super().__init__()

    class Annot:
        def __getitem__(self, item):
            return torch.Tensor

    mods = {"mmseg": None, "mmseg.registry": {"MODELS": Registry()}, "mmengine": None,
            "mmengine.model": {"BaseModule": BaseModule},
            "jaxtyping": {"Float": Annot(), "Int64": Annot(), "Shaped": Annot()}}
    for name, attrs in mods.items():
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in (attrs or {}).items():
            setattr(m, k, v)
        sys.modules[name] = m


def load_lifter_module():
    for pkg, sub in (("gf_reflifter", ""), ("gf_reflifter.lifter", "lifter"), ("gf_reflifter.utils", "utils")):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(REFERENCE, "model", sub)]
        sys.modules[pkg] = m
    return importlib.import_module("gf_reflifter.lifter.gaussian_lifter_v2")


def lidar2img(W_img, H_img):
    """The six cameras of gaussianformer_amd.synthetic.make_lifter_points as 4x4 lidar-to-image matrices."""
    f = 0.79 * W_img
    K = np.array([[f, 0, W_img / 2, 0], [0, f, H_img / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    mats = []
    for yaw in np.deg2rad([0.0, -55.0, -110.0, 180.0, 110.0, 55.0]):
        right = np.array([np.sin(yaw), -np.cos(yaw), 0.0])
        down = np.array([0.0, 0.0, -1.0])
        fwd = np.array([np.cos(yaw), np.sin(yaw), 0.0])
        c2l = np.eye(4)
        c2l[:3, 0], c2l[:3, 1], c2l[:3, 2], c2l[:3, 3] = right, down, fwd, [0.0, 0.0, 1.5]
        mats.append(K @ np.linalg.inv(c2l))
    return np.stack(mats)


def main():
    install_stubs()
    mod = load_lifter_module()
    calls = []

    def capture(scan, offset, new_offset):
        rec = dict(scan=scan.detach().cpu().numpy().astype(np.float32), offset=offset.detach().cpu().numpy(),
                   new_offset=new_offset.detach().cpu().numpy(), offset_dtype=str(offset.dtype),
                   new_offset_dtype=str(new_offset.dtype))
        rec["idx"] = fps_ref.fps(rec["scan"], rec["offset"], rec["new_offset"])
        calls.append(rec)
        return torch.from_numpy(rec["idx"]).to(scan.device)

    mod.farthest_point_sampling = capture
    torch.manual_seed(0)
    np.random.seed(0)
    embed, h, w, n_cam, W_img, H_img = 32, 27, 50, 6, 1600, 864
    lifter = mod.GaussianLifterV2(num_anchor=1500, embed_dims=embed, semantics=True, semantic_dim=17, include_opa=True,
                                  num_samples=128, anchors_per_pixel=1, random_sampling=False, deterministic=False)
    lifter.eval()
    feats = torch.randn(1, n_cam, embed * 4, h, w) * 2.0
    metas = {"projection_mat": torch.from_numpy(lidar2img(W_img, H_img)).float()[None],
             "image_wh": torch.tensor([[W_img, H_img]] * n_cam, dtype=torch.float32)[None],
             "occ_label": torch.randint(0, 18, (1, 200, 200, 16)),
             "occ_cam_mask": torch.ones(1, 200, 200, 16, dtype=torch.bool)}
    names = []
    with torch.no_grad():
        for name, kw in (("default", {}), ("bench3", {"benchmarking": True})):
            before = len(calls)
            try:
                lifter(metas, secondfpn_out=feats, **kw)
            except Exception as e:   # the rest of forward is not what is recorded; the call must have been made
                print(f"{name}: forward stopped after the sampling call: {type(e).__name__}: {e}")
            assert len(calls) == before + 1, f"{name}: the lifter did not call farthest_point_sampling"
            names.append(name)
    out = {}
    for name, rec in zip(names, calls):
        assert rec["offset_dtype"] == "torch.int32" and rec["new_offset_dtype"] == "torch.int32", rec
        out[name + "_scan"] = rec["scan"]
        out[name + "_offset"] = rec["offset"].astype(np.int32)
        out[name + "_new_offset"] = rec["new_offset"].astype(np.int32)
        out[name + "_idx"] = rec["idx"]
        print(name, rec["scan"].shape, rec["offset"].tolist(), rec["new_offset"].tolist(), rec["offset_dtype"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
