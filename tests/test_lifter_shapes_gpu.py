"""gf_lift_pixels and gf_pixel_loss_* on the MI355X at every entries-per-lane instantiation R = ceil(bins / 64), at both sides
of every 64-entry chunk edge, on ragged rows and tail workgroups, with a camera, an image size and an occupancy table per batch
element, upstream gradients other than 1, and the loss's -100 clamp and 1e-12 floor (the cases of tests/lifter_cases.py, whose
conditioning tests/test_lifter_cases.py proves on the CPU).  Truth is the float64 restatement (tests/lifter_ref.py): candidates,
slot order and pixel_gt equal outside the entries it marks as rounding-dependent (whose share bounds what may differ), points
within 1e-4 m, top-a ties exactly lower index first, the loss within 1e-5 relative, every gradient element within 1e-5 of the
size y of the terms it is formed from and exactly 0 where there are none."""
import numpy as np
import pytest

import lifter_cases as lc
import lifter_ref as ref

pytestmark = pytest.mark.gpu


def _dev(gpu, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _lift(gpu, inp, with_gt=True):
    """``(scans, pixel_gt, srcs, img2lidar)`` as numpy: the op's outputs and the inverse it used (torch's, on the device)."""
    from gaussianformer_amd.lifter import lift_pixels
    g = inp["grid"]
    proj = _dev(gpu, inp["proj"])
    scans, gt, srcs = lift_pixels(
        _dev(gpu, inp["logits"]), proj, _dev(gpu, inp["wh"]), depth_bins=_dev(gpu, inp["depth"]), pc_range=g["pc_range"],
        voxel_size=g["voxel_size"], occ_resolution=g["occ_resolution"], anchors_per_pixel=inp["a"], uniforms=_dev(gpu, inp["u"]),
        occ_label=_dev(gpu, inp["occ_label"]) if with_gt else None, occ_cam_mask=_dev(gpu, inp["occ_cam_mask"]) if with_gt else None,
        empty_label=lc.EMPTY, return_src=True)
    return ([s.cpu().numpy() for s in scans], None if gt is None else gt.cpu().numpy(), [s.cpu().numpy() for s in srcs],
            proj.inverse().cpu().numpy())


def _check(gpu, inp, what, with_gt=True):
    scans, gt, srcs, inv = _lift(gpu, inp, with_gt)
    assert (gt is None) == (not with_gt)
    r = lc.oracle(inp, img2lidar=inv, with_gt=with_gt)
    marked, compared = lc.exempt_share(r)
    assert marked <= lc.MAX_EXEMPT_SHARE * compared, (what, marked, compared)
    # differences only at marked entries, and no more of them than are marked
    ref.check_lift(r, scans, srcs, gt, what=f"{what} ({marked} marked)", bound=marked / compared)
    return r, scans, gt, srcs


@pytest.mark.parametrize("S,a,stochastic", lc.LIFT_CASES)
def test_lift_at_every_entries_per_lane(gpu, S, a, stochastic):
    r, scans, gt, _ = _check(gpu, lc.lift_inputs(S, a, stochastic), f"S={S} a={a} stochastic={stochastic}")
    assert all(s.shape[0] > 0 for s in scans) and gt[..., :-1].any() and gt[..., -1].any()


@pytest.mark.parametrize("S,a,stochastic", lc.NO_GT_CASES)
def test_lift_without_an_occupancy_table(gpu, S, a, stochastic):
    _check(gpu, lc.lift_inputs(S, a, stochastic), f"no table, S={S} a={a} stochastic={stochastic}", with_gt=False)


def test_lift_on_another_grid(gpu):
    S, a, stochastic = lc.OTHER_GRID_CASE
    _check(gpu, lc.lift_inputs(S, a, stochastic, grid=lc.OTHER_GRID), "pc_range not symmetric, voxel 0.4, 201 x 200 x 20")


def test_lift_uniforms_at_both_ends(gpu):
    inp = lc.edge_uniform_inputs()
    r, scans, _, srcs = _check(gpu, inp, "uniforms 0.0 and 1 - 2^-24")
    # The largest uniform below 1 is within the cdf tolerance of the last step's end, so the rule above leaves its slots out.
    # Where p_S is not tiny the answer does not depend on rounding all the same, and is held to the restatement's here.
    sure = lc.sure_top_uniform_slots(inp, r)
    assert len(sure) >= 6
    for i, s in sure:
        kept = s in srcs[i]
        assert kept == bool(r["keep"][i][s]), (i, s)
        if kept:
            np.testing.assert_allclose(scans[i][np.nonzero(srcs[i] == s)[0][0]], r["cand"][i][s], rtol=0, atol=1e-4)


def test_ties_go_to_the_lower_index_across_chunks(gpu):
    inp, expected = lc.tie_inputs()
    scans, _, srcs, inv = _lift(gpu, inp, with_gt=False)
    r = lc.tie_oracle(inp, img2lidar=inv)
    assert not r["slot_exempt"].any()
    ref.check_lift(r, scans, srcs, what="ties, S=191 a=4", bound=0)
    # and against the hand-computed entries: z names the bin
    want_src = [q * lc.TIE_A + j for q, e in enumerate(expected) if e is not None for j in range(lc.TIE_A)]
    want_bins = [min(k, lc.TIE_S - 1) for e in expected if e is not None for k in e]
    assert srcs[0].tolist() == want_src
    np.testing.assert_array_equal(lc.bins_of(scans[0][:, 2], inp["depth"]), want_bins)


def _loss_and_grad(gpu, x, gt, use_sigmoid, upstream=None, weight=None):
    """The op's loss and logits gradient; ``upstream``: ``(upstream * loss).backward()``; ``weight``: through the module."""
    import torch
    from gaussianformer_amd.lifter import PixelDistributionLoss, pixel_distribution_loss
    xt = _dev(gpu, x).requires_grad_(True)
    gtt = _dev(gpu, gt)
    if weight is not None:
        out = PixelDistributionLoss(weight=weight, use_sigmoid=use_sigmoid)({"pixel_logits": xt, "pixel_gt": gtt})
        out.backward()
        return out.item() / weight, xt.grad.cpu().numpy()
    loss = pixel_distribution_loss(xt, gtt, use_sigmoid=use_sigmoid)
    (loss if upstream is None else upstream * loss).backward()
    return loss.item(), xt.grad.cpu().numpy()


def _check_loss(got, want, what):
    print(f"{what}: loss {got!r} against {want!r}")
    assert abs(got - want) <= lc.LOSS_RTOL * abs(want), (what, got, want)


@pytest.mark.parametrize("use_sigmoid", [False, True])
@pytest.mark.parametrize("bins", lc.LOSS_BINS)
def test_pixel_loss_at_every_entries_per_lane_and_ragged_rows(gpu, bins, use_sigmoid):
    for rows in lc.LOSS_ROWS:
        x, gt = lc.loss_inputs(rows, bins, use_sigmoid)
        want, g, y = ref.pixel_loss_terms(x, gt, use_sigmoid)
        what = f"{'sigmoid' if use_sigmoid else 'softmax'} bins={bins} rows={rows}"
        loss, grad = _loss_and_grad(gpu, x, gt, use_sigmoid, upstream=lc.UPSTREAM)
        _check_loss(loss, want, what)
        lc.check_grad(grad, g, y, what, scale=lc.UPSTREAM)


@pytest.mark.parametrize("use_sigmoid", [False, True])
def test_pixel_loss_through_the_module_with_a_weight(gpu, use_sigmoid):
    x, gt = lc.loss_inputs(70, 65, use_sigmoid)
    want, g, y = ref.pixel_loss_terms(x, gt, use_sigmoid)
    loss, grad = _loss_and_grad(gpu, x.reshape(2, 5, 7, 65), gt.reshape(2, 5, 7, 65), use_sigmoid, weight=lc.MODULE_WEIGHT)
    _check_loss(loss, want, "module, weight 0.25")
    lc.check_grad(grad.reshape(70, 65), g, y, "module, weight 0.25", scale=lc.MODULE_WEIGHT)


@pytest.mark.parametrize("use_sigmoid", [False, True])
def test_pixel_loss_clamp_and_floor(gpu, use_sigmoid):
    import torch
    import torch.nn.functional as F
    x, gt = lc.saturated_inputs(use_sigmoid)
    want, g, y = ref.pixel_loss_terms(x, gt, use_sigmoid)
    what = f"saturated {'sigmoid' if use_sigmoid else 'softmax'}"
    loss, grad = _loss_and_grad(gpu, x, gt, use_sigmoid, upstream=lc.UPSTREAM)
    _check_loss(loss, want, what)
    lc.check_grad(grad, g, y, what, scale=lc.UPSTREAM)
    # the second witness: torch's own binary_cross_entropy on the device, held to the same bounds; with p exactly 0 or 1 the two
    # cannot differ by conditioning
    xt = _dev(gpu, x).requires_grad_(True)
    p = torch.sigmoid(xt) if use_sigmoid else torch.softmax(xt, -1)
    tl = F.binary_cross_entropy(p, _dev(gpu, gt).float())
    (lc.UPSTREAM * tl).backward()
    tg = xt.grad.cpu().numpy()
    _check_loss(tl.item(), want, what + ", torch")
    lc.check_grad(tg, g, y, what + ", torch", scale=lc.UPSTREAM)
    _check_loss(loss, tl.item(), what + ", against torch")
    lc.check_grad(grad, tg.astype(np.float64) / lc.UPSTREAM, y, what + ", against torch", scale=lc.UPSTREAM)


def test_module_at_its_default_num_samples(gpu, monkeypatch):
    import torch
    from gaussianformer_amd import lifter
    torch.manual_seed(0)
    np.random.seed(0)
    m = lifter.GaussianLifterV2(num_anchor=40, embed_dims=lc.MODULE_C // 4, anchors_per_pixel=2, deterministic=False).to(gpu)
    assert m.num_samples == 64
    proj, wh = lc.cameras()
    label, mask = lc.occupancy()
    metas = {"projection_mat": _dev(gpu, proj), "image_wh": _dev(gpu, wh), "occ_label": _dev(gpu, label),
             "occ_cam_mask": _dev(gpu, mask)}
    calls = []
    real = lifter.lift_pixels

    def spy(*args, **kw):
        calls.append((args, kw))
        return real(*args, **kw)

    monkeypatch.setattr(lifter, "lift_pixels", spy)
    out = m(metas, secondfpn_out=_dev(gpu, lc.module_feats()))
    assert len(calls) == 1
    logits, gt = out["pixel_logits"], out["pixel_gt"]
    assert logits.shape == (lc.B, lc.N, lc.H, lc.W, 65) and gt.shape == logits.shape and gt.dtype == torch.bool
    assert out["representation"].shape[:2] == (lc.B, 40) and torch.isfinite(out["representation"]).all()
    # the module's pixel_gt is lift_pixels' on these logits and uniforms, and that is the restatement's
    args, kw = calls[0]
    assert args[0] is logits and kw["uniforms"].shape == (lc.B, lc.N, lc.H, lc.W, 2)
    scans, gt2, srcs = real(*args, **kw, return_src=True)
    assert torch.equal(gt, gt2)
    c = lambda t: t.detach().cpu().numpy()
    r = ref.lift(c(logits), c(metas["projection_mat"].inverse()), wh, c(m.depth_bins), lc.PC, lc.VS, lc.RES, 2,
                 uniforms=c(kw["uniforms"]), occ=lc.packed(label, mask))
    marked, compared = lc.exempt_share(r)
    assert marked <= lc.MAX_EXEMPT_SHARE * compared, (marked, compared)
    ref.check_lift(r, [c(s) for s in scans], [c(s) for s in srcs], c(gt), what=f"module default ({marked} marked)",
                   bound=marked / compared)
    for use_sigmoid in (True, False):
        want, g, y = ref.pixel_loss_terms(c(logits), c(gt), use_sigmoid)
        loss = lifter.PixelDistributionLoss(weight=lc.MODULE_WEIGHT, use_sigmoid=use_sigmoid)(out)
        grad, = torch.autograd.grad(loss, logits, retain_graph=True)
        _check_loss(loss.item() / lc.MODULE_WEIGHT, want, f"module default, sigmoid={use_sigmoid}")
        lc.check_grad(c(grad), g, y, f"module default, sigmoid={use_sigmoid}", scale=lc.MODULE_WEIGHT)
