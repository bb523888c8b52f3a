"""gf_lift_pixels and gf_pixel_loss_* on the MI355X against the float64 restatement (tests/lifter_ref.py) and the fixture
recorded from the reference (tests/golden/lifter.npz).  Candidates, their slot order and pixel_gt match exactly except at
entries whose answer depends on rounding (lifter_ref.check_lift prints and bounds how many); points within 1e-4 m; the loss
within 1e-5 relative and gradients within 1e-5 x max|grad|.  The oracle is fed the img2lidar the op used (torch's inverse
on the device)."""
import os

import numpy as np
import pytest

import lifter_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lifter.npz")
PC = [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0]
RES = (200, 200, 16)


def lidar2img(n_cam, W_img, H_img):
    f = 0.79 * W_img
    K = np.array([[f, 0, W_img / 2, 0], [0, f, H_img / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    mats = []
    for yaw in np.deg2rad(np.linspace(0.0, 360.0, n_cam, endpoint=False)):
        c2l = np.eye(4)
        c2l[:3, 0] = [np.sin(yaw), -np.cos(yaw), 0.0]
        c2l[:3, 1] = [0.0, 0.0, -1.0]
        c2l[:3, 2] = [np.cos(yaw), np.sin(yaw), 0.0]
        c2l[:3, 3] = [0.0, 0.0, 1.5]
        mats.append(K @ np.linalg.inv(c2l))
    return np.stack(mats).astype(np.float32)


def make_inputs(gpu, b=1, n=6, h=108, w=200, S=128, a=1, seed=0, stochastic=True):
    import torch
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(b, n, h, w, S + 1, generator=g) * 2.0
    logits[..., S] += 1.5
    proj = torch.from_numpy(np.stack([lidar2img(n, 1600, 864)] * b))
    wh = torch.tensor([[1600.0, 864.0]] * n).expand(b, n, 2).contiguous()
    rng = np.random.default_rng(seed)
    occ = np.zeros((b,) + RES, np.uint8)
    for i in range(b):
        occ[i, :, :, :2] = 1
        for _ in range(300):
            x, y = rng.integers(0, 190, 2)
            z = rng.integers(0, 12)
            dx, dy, dz = rng.integers(2, 15, 3)
            occ[i, x:x + dx, y:y + dy, z:z + dz] = rng.integers(0, 2)
    u = torch.rand(b, n, h, w, a, generator=g) if stochastic else None
    dev = lambda t: None if t is None else t.to(gpu)
    return dict(logits=dev(logits), proj=dev(proj), wh=dev(wh), depth=dev(torch.linspace(1.0, 72.0, S)), u=dev(u),
                occ=dev(torch.from_numpy(occ)), a=a)


def run(inp, with_gt=True):
    import torch
    from gaussianformer_amd.lifter import lift_pixels
    occ = inp["occ"]
    # occ is already the packed table: label 1 = occupied against empty_label 0, every voxel valid
    return lift_pixels(inp["logits"], inp["proj"], inp["wh"], depth_bins=inp["depth"], pc_range=PC, voxel_size=0.5,
                       occ_resolution=RES, anchors_per_pixel=inp["a"], uniforms=inp["u"],
                       occ_label=occ if with_gt else None, occ_cam_mask=torch.ones_like(occ, dtype=torch.bool) if with_gt else None,
                       empty_label=0, return_src=True)


def oracle(inp, with_gt=True):
    c = lambda t: None if t is None else t.detach().cpu().numpy()
    return ref.lift(c(inp["logits"]), c(inp["proj"].inverse()), c(inp["wh"]), c(inp["depth"]), PC, 0.5, RES, inp["a"],
                    uniforms=c(inp["u"]), occ=c(inp["occ"]) if with_gt else None)


def check(inp, what, with_gt=True):
    scans, gt, srcs = run(inp, with_gt)
    r = oracle(inp, with_gt)
    ref.check_lift(r, [s.cpu().numpy() for s in scans], [s.cpu().numpy() for s in srcs],
                   None if gt is None else gt.cpu().numpy(), what=what)
    return scans, gt, srcs


@pytest.mark.parametrize("mode", ["deterministic", "stochastic"])
def test_fixture(gpu, mode):
    import torch
    from gaussianformer_amd.lifter import lift_pixels
    d = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(d[k]).to(gpu)
    occ = t("occ_packed")
    scans, gt, srcs = lift_pixels(t("logits"), t("projection_mat"), t("image_wh"), depth_bins=t("depth_bins"),
                                  pc_range=d["pc_range"].tolist(), voxel_size=float(d["voxel_size"]), occ_resolution=RES,
                                  anchors_per_pixel=1, uniforms=t("uniforms") if mode == "stochastic" else None,
                                  occ_label=occ, occ_cam_mask=None, empty_label=0, return_src=True)
    # against the reference's own outputs
    c = scans[0].shape[0]
    want = d[f"{mode}_scan"]
    np.testing.assert_allclose(scans[0].cpu().numpy(), want[:c], rtol=0, atol=1e-4)
    assert want.shape[0] >= c and (c >= int(d["num_anchor"]) or want.shape[0] > c)
    r = ref.lift(d["logits"], t("projection_mat").inverse().cpu().numpy(), d["image_wh"], d["depth_bins"],
                 d["pc_range"].tolist(), float(d["voxel_size"]), RES, 1,
                 uniforms=d["uniforms"] if mode == "stochastic" else None, occ=d["occ_packed"])
    ref.check_lift(r, [scans[0].cpu().numpy()], [srcs[0].cpu().numpy()], gt.cpu().numpy(), what=f"fixture {mode}")
    np.testing.assert_array_equal(gt.cpu().numpy(), d["pixel_gt"])


@pytest.mark.parametrize("use_sigmoid", [False, True])
def test_fixture_loss(gpu, use_sigmoid):
    import torch
    from gaussianformer_amd.lifter import PixelDistributionLoss
    d = np.load(GOLDEN)
    key = "sigmoid" if use_sigmoid else "softmax"
    x = torch.from_numpy(d["logits"]).to(gpu).requires_grad_(True)
    gt = torch.from_numpy(d["pixel_gt"]).to(gpu)
    loss = PixelDistributionLoss(weight=1.0, use_sigmoid=use_sigmoid)({"pixel_logits": x, "pixel_gt": gt})
    loss.backward()
    want = float(d[f"{key}_loss"])
    assert abs(loss.item() - want) <= 1e-5 * abs(want), (loss.item(), want)
    w = d[f"{key}_grad"]
    assert np.abs(x.grad.cpu().numpy() - w).max() <= 1e-5 * np.abs(w).max()


@pytest.mark.parametrize("stochastic", [False, True])
def test_full_size(gpu, stochastic):
    inp = make_inputs(gpu, stochastic=stochastic, seed=1 + stochastic)
    scans, gt, _ = check(inp, f"full size, stochastic={stochastic}")
    assert scans[0].shape[0] > 10000 and gt[..., :-1].any()


@pytest.mark.parametrize("a", [2, 4])
@pytest.mark.parametrize("stochastic", [False, True])
def test_anchors_per_pixel(gpu, a, stochastic):
    check(make_inputs(gpu, h=27, w=50, a=a, stochastic=stochastic, seed=10 + a), f"a={a}, stochastic={stochastic}")


def test_constructed_cases(gpu):
    import torch
    from gaussianformer_amd.lifter import lift_pixels
    S = 8
    x = torch.zeros(1, 1, 1, 3, S + 1)
    x[0, 0, 0, 0, S] = 5.0                       # argmax = S: disabled
    x[0, 0, 0, 1, 2] = 5.0                       # argmax 2; a uniform near 1 samples S -> kept at bin S - 1
    x[0, 0, 0, 1, S] = 4.0
    x[0, 0, 0, 2, [3, 5]] = 6.0                  # exact tie: the lower index
    depth = torch.linspace(1, 8, S)
    kw = dict(depth_bins=depth.to(gpu), pc_range=[-100, -100, -100, 100, 100, 100], voxel_size=0.5, occ_resolution=(4, 4, 4),
              anchors_per_pixel=1, return_src=True)
    M, wh = torch.eye(4)[None, None].to(gpu), torch.tensor([[[3.0, 1.0]]]).to(gpu)
    u = torch.tensor([0.5, 0.99999, 0.5]).reshape(1, 1, 1, 3, 1).to(gpu)
    scans, _, srcs = lift_pixels(x.to(gpu), M, wh, uniforms=u, **kw)
    assert srcs[0].tolist() == [1, 2]
    np.testing.assert_allclose(scans[0][0].cpu().numpy(), [1.5 * 8, 0.5 * 8, 8], rtol=1e-6)
    scans, _, srcs = lift_pixels(x.to(gpu), M, wh, **kw)     # deterministic: the tie goes to bin 3
    d3 = float(depth[3])
    np.testing.assert_allclose(scans[0][1].cpu().numpy(), [2.5 * d3, 0.5 * d3, d3], rtol=1e-6)
    # every point out of range: count 0, the padding holds zeros and src -1
    scans, gt, srcs = lift_pixels(x.to(gpu), M, wh, uniforms=u, **{**kw, "pc_range": [500, 500, 500, 600, 600, 600]})
    assert scans[0].shape == (0, 3) and srcs[0].numel() == 0


def test_padding_and_counts_per_element(gpu):
    import torch
    inp = make_inputs(gpu, b=2, h=27, w=50, seed=5)
    inp["logits"][1, :3, ..., -1] += 20.0     # element 1: three cameras disabled
    scans, gt, srcs = check(inp, "b=2")
    assert scans[0].shape[0] > scans[1].shape[0] > 0
    # the padded buffer behind each element's candidates: zeros and src -1
    base = scans[1]._base if scans[1]._base is not None else scans[1]
    full_src = srcs[1]._base if srcs[1]._base is not None else srcs[1]
    c1 = scans[1].shape[0]
    assert torch.all(base[1, c1:] == 0) and torch.all(full_src[1, c1:] == -1)


def test_bitwise_reproducible(gpu):
    import torch
    from gaussianformer_amd.lifter import pixel_distribution_loss
    inp = make_inputs(gpu, seed=3)
    a, b = run(inp), run(inp)
    for x, y in zip(a[0] + a[2] + [a[1]], b[0] + b[2] + [b[1]]):
        assert torch.equal(x, y)
    out = []
    for _ in range(2):
        x = inp["logits"].clone().requires_grad_(True)
        loss = pixel_distribution_loss(x, a[1], use_sigmoid=False)
        loss.backward()
        out.append((loss.detach(), x.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("use_sigmoid", [False, True])
def test_loss_full_size(gpu, use_sigmoid):
    import torch
    from gaussianformer_amd.lifter import pixel_distribution_loss
    inp = make_inputs(gpu, seed=4, stochastic=False)
    _, gt, _ = run(inp)
    x = inp["logits"].clone().requires_grad_(True)
    loss = pixel_distribution_loss(x, gt, use_sigmoid=use_sigmoid)
    loss.backward()
    # fp64 torch restatement on the fp32 p (torch's BCE: log clamped at -100; backward floor 1e-12 on p (1 - p))
    x32 = inp["logits"]
    p = (torch.sigmoid(x32) if use_sigmoid else torch.softmax(x32, -1)).double()
    t = gt.double()
    want = -(t * torch.log(p).clamp(min=-100) + (1 - t) * torch.log1p(-p).clamp(min=-100)).mean()
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())
    gp = (p - t) / torch.clamp((1 - p) * p, min=float(np.float32(1e-12))) / t.numel()
    g = gp * (1 - p) * p if use_sigmoid else p * (gp - (gp * p).sum(-1, keepdim=True))
    assert (x.grad.double() - g).abs().max().item() <= 1e-5 * g.abs().max().item()


def _module(gpu, **kw):
    import torch
    from gaussianformer_amd.lifter import GaussianLifterV2
    d = np.load(GOLDEN)
    torch.manual_seed(0)
    m = GaussianLifterV2(num_anchor=int(d["num_anchor"]), embed_dims=32, semantics=True, semantic_dim=17, num_samples=128,
                         anchors_per_pixel=1, random_sampling=False, deterministic=False, random_samples=50, **kw)
    return m.to(gpu), d


def test_module_loads_the_reference_state_dict_and_runs(gpu):
    import torch
    m, d = _module(gpu)
    shapes = [tuple(int(v) for v in s.split(",") if v) for s in d["state_dict_shapes"]]
    sd = {k: torch.randn(s) for k, s in zip(d["state_dict_keys"].tolist(), shapes)}
    m.load_state_dict(sd, strict=True)
    with torch.no_grad():
        m.projection[1].bias[128] = 1.5
    feats = torch.randn(1, 6, 128, 27, 50).to(gpu)
    metas = {"projection_mat": torch.from_numpy(lidar2img(6, 1600, 864))[None].to(gpu),
             "image_wh": torch.tensor([[[1600.0, 864.0]] * 6]).to(gpu),
             "occ_label": torch.randint(0, 18, (1,) + RES).to(gpu), "occ_cam_mask": torch.ones((1,) + RES, dtype=torch.bool).to(gpu)}
    out = m(metas, secondfpn_out=feats)
    assert set(out) == {"rep_features", "representation", "anchor_init", "pixel_logits", "pixel_gt"}
    assert out["representation"].shape == (1, 200 + 50, 3 + 3 + 4 + 1 + 17)
    assert out["pixel_gt"].shape == (1, 6, 27, 50, 129) and out["pixel_gt"].dtype == torch.bool
    assert torch.isfinite(out["representation"]).all()
    xyz = torch.sigmoid(out["representation"][0, :200, :3])
    assert (xyz > 0).all() and (xyz < 1).all()


def test_module_benchmarking_takes_three_segments(gpu, monkeypatch):
    import torch
    from gaussianformer_amd import lifter
    m, d = _module(gpu)
    calls = []
    real = lifter.farthest_point_sampling

    def spy(xyz, offset, new_offset):
        calls.append((offset.tolist(), new_offset.tolist()))
        return real(xyz, offset, new_offset)

    monkeypatch.setattr(lifter, "farthest_point_sampling", spy)
    feats = torch.randn(1, 6, 128, 27, 50).to(gpu)
    metas = {"projection_mat": torch.from_numpy(lidar2img(6, 1600, 864))[None].to(gpu),
             "image_wh": torch.tensor([[[1600.0, 864.0]] * 6]).to(gpu)}
    out = m(metas, secondfpn_out=feats, benchmarking=True)
    assert out["pixel_gt"] is None
    assert len(calls) == 1 and len(calls[0][0]) == 3 and calls[0][1][-1] == 200
    assert out["representation"].shape[1] == 250
