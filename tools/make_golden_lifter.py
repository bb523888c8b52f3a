"""Record what the reference's own GaussianLifterV2 and PixelDistributionLoss compute -> tests/golden/lifter.npz.

Imports model/lifter/gaussian_lifter_v2.py and loss/bce_loss.py from the reference tree UNMODIFIED, with the stub loading
of tools/make_golden_lifter_fps.py (synthetic packages whose __init__ files are not executed, minimal stand-ins for
mmseg / mmengine / jaxtyping and for the tensorboard wrapper loss/base_loss.py imports).  The lifter's
``farthest_point_sampling`` is replaced by a capturing function (the pre-FPS ``scan``; answered with the numpy FPS oracle),
and the sampler module's ``torch`` by a proxy that records the uniforms ``torch.rand`` draws.  Runs on the CPU at a
reduced size -- 6 cameras x 6 x 10 pixels, S = 128 depth bins, num_anchor 200 -- so that the logits and both gradients
fit the fixture size limit; the projection's bias on the "no surface" bin is raised so that about a fifth of the pixels
are disabled, and the occupancy is mostly empty with blocks of classes.  Both sampling modes run on the same logits.

    python tools/make_golden_lifter.py [reference_root]
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests import fps_ref  # noqa: E402
import make_golden_lifter_fps as fps_tool  # noqa: E402

REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GF_REFERENCE_ROOT", "/root/reference")
fps_tool.REFERENCE = REFERENCE
OUT = os.path.join(ROOT, "tests", "golden", "lifter.npz")
N_CAM, H, W, S, EMBED, NUM_ANCHOR, RANDOM_SAMPLES = 6, 6, 10, 128, 32, 200, 50
W_IMG, H_IMG = 1600, 864


def load_loss_module():
    class Registry:
        def register_module(self, *a, **k):
            return (lambda cls: cls) if not a or not isinstance(a[0], type) else a[0]

    class WrappedTBWriter:
        _instance_dict = {}

    for name, attrs in (("misc", {}), ("misc.tb_wrapper", {"WrappedTBWriter": WrappedTBWriter})):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
    pkg = types.ModuleType("gf_refloss")
    pkg.__path__ = [os.path.join(REFERENCE, "loss")]
    pkg.OPENOCC_LOSS = Registry()
    sys.modules["gf_refloss"] = pkg
    return importlib.import_module("gf_refloss.bce_loss")


class RandRecorder:
    """Stands in for ``torch`` in the sampler module: ``rand`` draws from torch and keeps what it drew."""

    def __init__(self):
        self.drawn = []

    def rand(self, *a, **k):
        t = torch.rand(*a, **k)
        self.drawn.append(t.detach().cpu().numpy().copy())
        return t

    def __getattr__(self, name):
        return getattr(torch, name)


def structured_occupancy(rng):
    occ = np.full((200, 200, 16), 17, np.int64)
    for _ in range(60):
        x, y = rng.integers(20, 180, 2)
        z = rng.integers(0, 10)
        dx, dy, dz = rng.integers(4, 20, 3)
        occ[x:x + dx, y:y + dy, z:z + dz] = rng.integers(0, 17)
    occ[:, :, 0:2] = 11   # a ground plane
    mask = np.ones((200, 200, 16), bool)
    mask[:40, :, :] = False
    mask[:, 150:170, :] = False
    return occ, mask


def main():
    fps_tool.install_stubs()
    mod = fps_tool.load_lifter_module()
    sampler_mod = sys.modules["gf_reflifter.utils.sampler"]
    recorder = RandRecorder()
    sampler_mod.torch = recorder
    scans = []

    def capture(scan, offset, new_offset):
        s = scan.detach().cpu().numpy().astype(np.float32)
        scans.append(s)
        idx = fps_ref.fps(s, offset.cpu().numpy(), new_offset.cpu().numpy())
        return torch.from_numpy(idx).long()

    mod.farthest_point_sampling = capture
    torch.manual_seed(0)
    np.random.seed(0)
    rng = np.random.default_rng(0)
    lifter = mod.GaussianLifterV2(num_anchor=NUM_ANCHOR, embed_dims=EMBED, semantics=True, semantic_dim=17,
                                  include_opa=True, num_samples=S, anchors_per_pixel=1, random_sampling=False,
                                  deterministic=False, random_samples=RANDOM_SAMPLES)
    lifter.eval()
    with torch.no_grad():
        lifter.projection[1].bias[S] += 1.5
    feats = torch.randn(1, N_CAM, EMBED * 4, H, W) * 2.0
    occ, mask = structured_occupancy(rng)
    metas = {"projection_mat": torch.from_numpy(fps_tool.lidar2img(W_IMG, H_IMG)).float()[None],
             "image_wh": torch.tensor([[W_IMG, H_IMG]] * N_CAM, dtype=torch.float32)[None],
             "occ_label": torch.from_numpy(occ)[None], "occ_cam_mask": torch.from_numpy(mask)[None]}
    out = {}
    logits = gt = None
    for mode in ("deterministic", "stochastic"):
        lifter.deterministic = mode == "deterministic"
        before, drawn = len(scans), len(recorder.drawn)
        with torch.no_grad():
            res = lifter(metas, secondfpn_out=feats)
        assert len(scans) == before + 1
        if logits is None:
            logits, gt = res["pixel_logits"].clone(), res["pixel_gt"].clone()
        else:
            assert torch.equal(logits, res["pixel_logits"]) and torch.equal(gt, res["pixel_gt"])
        out[f"{mode}_scan"] = scans[-1]
        if mode == "stochastic":
            assert len(recorder.drawn) == drawn + 1
            out["uniforms"] = recorder.drawn[-1].astype(np.float32)
        else:
            assert len(recorder.drawn) == drawn
        print(mode, "scan", scans[-1].shape)
    pdf = torch.softmax(logits, -1)
    print("disabled fraction", float((pdf.argmax(-1) == S).float().mean()), "gt positives", int(gt[..., :S].sum()))
    loss_mod = load_loss_module()
    for use_sigmoid in (False, True):
        x = logits.clone().requires_grad_(True)
        loss = loss_mod.PixelDistributionLoss(weight=1.0, use_sigmoid=use_sigmoid)({"pixel_logits": x, "pixel_gt": gt})
        loss.backward()
        key = "sigmoid" if use_sigmoid else "softmax"
        out[f"{key}_loss"] = np.float32(loss.item())
        out[f"{key}_grad"] = x.grad.numpy().astype(np.float32)
        print(key, "loss", loss.item())
    sd = lifter.state_dict()
    out.update(
        logits=logits.numpy().astype(np.float32),
        projection_mat=metas["projection_mat"].numpy(),
        img2lidar=metas["projection_mat"].inverse().numpy(),
        image_wh=metas["image_wh"].numpy(),
        depth_bins=lifter.depth_bins.numpy(),
        occ_packed=((occ != 17) & mask).astype(np.uint8)[None],
        pixel_gt=gt.numpy(),
        pc_range=np.asarray(lifter.pc_range, np.float32),
        voxel_size=np.float32(lifter.voxel_size),
        num_anchor=np.int32(NUM_ANCHOR),
        state_dict_keys=np.array(list(sd.keys())),
        state_dict_shapes=np.array([",".join(str(s) for s in v.shape) for v in sd.values()]),
    )
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
