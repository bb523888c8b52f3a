"""CPU checks of the pixel lifting and pixel loss (gf_lift_pixels, gf_pixel_loss_*, gaussianformer_amd.lifter): the float64
restatement its GPU tests compare against (tests/lifter_ref.py) reproduces what the reference's own GaussianLifterV2 and
PixelDistributionLoss recorded (tests/golden/lifter.npz, written by tools/make_golden_lifter.py) in both sampling modes and
both loss settings; the C entry points refuse bad arguments before any HIP call; CPU tensors are refused."""
import ctypes
import math
import os

import numpy as np
import pytest

import lifter_ref as ref
from gaussianformer_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lifter.npz")


def _lift(d, mode):
    return ref.lift(d["logits"], d["img2lidar"], d["image_wh"], d["depth_bins"], d["pc_range"].tolist(),
                    float(d["voxel_size"]), (200, 200, 16), 1, uniforms=d["uniforms"] if mode == "stochastic" else None,
                    occ=d["occ_packed"])


@pytest.mark.parametrize("mode", ["deterministic", "stochastic"])
def test_restatement_matches_reference_scan(mode):
    d = np.load(GOLDEN)
    r = _lift(d, mode)
    scan, want = r["scans"][0], d[f"{mode}_scan"]
    c, m = scan.shape[0], int(d["num_anchor"])
    # the reference repeats a short scan ceil(m / c) - 1 times behind it (with jitter) before FPS
    assert want.shape[0] == (c if c >= m else c * math.ceil(m / c))
    # the reference's candidates (the head of its pre-FPS scan) in the oracle's slots: none may differ, even where exempted
    ex, _ = ref.check_lift(r, [want[:c]], r["src"], what=f"reference {mode} scan", bound=0)
    assert ex == 0


def test_restatement_matches_reference_pixel_gt():
    d = np.load(GOLDEN)
    r = _lift(d, "deterministic")
    ref.check_lift(r, r["scans"], r["src"], pixel_gt=d["pixel_gt"], what="reference pixel_gt")
    want = d["pixel_gt"]
    assert want[..., :-1].sum() > 1000 and (~want[..., -1]).sum() > 50


@pytest.mark.parametrize("use_sigmoid", [False, True])
def test_restatement_matches_reference_loss(use_sigmoid):
    d = np.load(GOLDEN)
    key = "sigmoid" if use_sigmoid else "softmax"
    loss, grad = ref.pixel_loss(d["logits"], d["pixel_gt"], use_sigmoid)
    want = float(d[f"{key}_loss"])
    assert abs(loss - want) <= 1e-5 * abs(want), (loss, want)
    w = d[f"{key}_grad"]
    assert np.abs(grad - w).max() <= 1e-5 * np.abs(w).max()


def test_restatement_constructed_cases():
    S = 8
    M = np.eye(4, dtype=np.float32)[None, None]
    wh = np.array([[[3.0, 1.0]]], np.float32)          # u = j + 0.5, v = 0.5
    depth = np.linspace(1, 8, S).astype(np.float32)
    pc = [-100, -100, -100, 100, 100, 100]
    x = np.zeros((1, 1, 1, 3, S + 1), np.float32)
    x[0, 0, 0, 0, S] = 5.0                       # argmax = S: disabled
    x[0, 0, 0, 1, 2] = 5.0                       # argmax 2, but a uniform of 0.9999 samples S -> bin S - 1
    x[0, 0, 0, 1, S] = 4.0
    x[0, 0, 0, 2, [3, 5]] = 6.0                  # exact tie: the lower index
    r = ref.lift(x, M, wh, depth, pc, 0.5, (4, 4, 4), 1, uniforms=np.array([0.5, 0.99999, 0.5], np.float32).reshape(1, 1, 1, 3, 1))
    assert r["keep"][0].tolist() == [False, True, True]
    np.testing.assert_allclose(r["scans"][0][0], [1.5 * 8, 0.5 * 8, 8])
    det = ref.lift(x, M, wh, depth, pc, 0.5, (4, 4, 4), 1)
    assert det["src"][0].tolist() == [1, 2]
    np.testing.assert_allclose(det["scans"][0][1], [2.5 * depth[3], 0.5 * depth[3], depth[3]])


def _lift_call(lib, b=1, n=6, h=4, w=5, S=128, a=1, logits=8, M=8, wh=8, d=8, pc=None, vs=0.5, X=200, Y=200, Z=16, occ=8,
               u=None, points=8, counts=8, src=None, gt=8, ws=8, nbytes=1 << 40):
    if pc is None:
        pc = (ctypes.c_float * 6)(-50, -50, -5, 50, 50, 3)
    return lib.gf_lift_pixels(b, n, h, w, S, a, logits, M, wh, d, pc, vs, X, Y, Z, occ, u, points, counts, src, gt, ws,
                              nbytes, None)


def test_abi_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    assert lib.gf_lift_workspace_bytes(1, 129600, 1) > 0
    assert lib.gf_lift_workspace_bytes(1, 129600, 9) == 0
    assert lib.gf_lift_workspace_bytes(0, 100, 1) == 0
    assert lib.gf_pixel_loss_workspace_bytes(129600, 129) > 0
    assert lib.gf_pixel_loss_workspace_bytes(10, 257) == 0

    def refused(rc, text):
        assert rc == -1, rc
        assert text in lib.gf_last_error().decode(), lib.gf_last_error()

    refused(_lift_call(lib, S=256), "S + 1 <= 256")
    refused(_lift_call(lib, S=0), "S + 1 <= 256")
    refused(_lift_call(lib, a=9), "anchors_per_pixel")
    refused(_lift_call(lib, a=0), "anchors_per_pixel")
    refused(_lift_call(lib, b=0), "b = 0")
    refused(_lift_call(lib, h=0), "h = 0")
    refused(_lift_call(lib, logits=None), "null input")
    refused(_lift_call(lib, counts=None), "points and counts")
    refused(_lift_call(lib, points=None, counts=None, gt=None), "nothing to compute")
    refused(_lift_call(lib, points=None, counts=None, src=8), "src needs points")
    refused(_lift_call(lib, occ=None), "occupancy table")
    refused(_lift_call(lib, vs=0.0), "voxel_size")
    refused(_lift_call(lib, pc=(ctypes.c_float * 6)(50, -50, -5, -50, 50, 3)), "pc_range axis 0")
    refused(_lift_call(lib, ws=None), "null workspace")
    assert _lift_call(lib, nbytes=16) == -2
    assert "workspace" in lib.gf_last_error().decode()
    assert _lift_call(lib, S=254, points=None, counts=None, gt=None) == -1   # the largest S, refused for another reason

    S, L = _lib.GF_PIXEL_LOSS_SOFTMAX, _lib.GF_PIXEL_LOSS_SIGMOID
    refused(lib.gf_pixel_loss_forward(100, 129, 0, 8, 8, 8, 8, 1 << 40, None), "exactly one")
    refused(lib.gf_pixel_loss_forward(100, 129, S | L, 8, 8, 8, 8, 1 << 40, None), "exactly one")
    refused(lib.gf_pixel_loss_forward(100, 257, S, 8, 8, 8, 8, 1 << 40, None), "bins = 257")
    refused(lib.gf_pixel_loss_forward(0, 129, S, 8, 8, 8, 8, 1 << 40, None), "rows = 0")
    refused(lib.gf_pixel_loss_forward(100, 129, S, None, 8, 8, 8, 1 << 40, None), "null pointer")
    assert lib.gf_pixel_loss_forward(100, 129, S, 8, 8, 8, 8, 8, None) == -2
    refused(lib.gf_pixel_loss_backward(100, 129, L, 8, 8, None, 8, None), "null gradient")
    refused(lib.gf_pixel_loss_backward(100, 0, L, 8, 8, 8, 8, None), "bins = 0")


def test_cpu_tensors_are_refused():
    import torch
    from gaussianformer_amd import lifter
    x = torch.zeros(1, 1, 2, 2, 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lifter.lift_pixels(x, torch.eye(4)[None, None], torch.ones(1, 1, 2), depth_bins=torch.linspace(1, 72, 8),
                           pc_range=[-50, -50, -5, 50, 50, 3], voxel_size=0.5, occ_resolution=[200, 200, 16],
                           anchors_per_pixel=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lifter.pixel_distribution_loss(x, torch.zeros(x.shape, dtype=torch.bool), use_sigmoid=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lifter.PixelDistributionLoss(use_sigmoid=False)({"pixel_logits": x, "pixel_gt": x > 0})


def test_module_refuses_a_config_initializer():
    from gaussianformer_amd.lifter import GaussianLifterV2
    with pytest.raises(ValueError, match="mmseg"):
        GaussianLifterV2(num_anchor=10, embed_dims=8, initializer=dict(type="ResNetSecondFPN"))


def test_module_state_dict_matches_the_reference_keys():
    import torch
    from gaussianformer_amd.lifter import GaussianLifterV2
    d = np.load(GOLDEN)
    m = GaussianLifterV2(num_anchor=int(d["num_anchor"]), embed_dims=32, semantics=True, semantic_dim=17, num_samples=128,
                         anchors_per_pixel=1, random_sampling=False, deterministic=False, random_samples=50)
    sd = m.state_dict()
    assert list(sd.keys()) == d["state_dict_keys"].tolist()
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == d["state_dict_shapes"].tolist()
    assert "depth_bins" not in sd and "pc_start" not in sd
    torch.testing.assert_close(m.depth_bins, torch.from_numpy(d["depth_bins"]), rtol=0, atol=0)
