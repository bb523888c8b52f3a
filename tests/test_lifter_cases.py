"""tests/lifter_cases.py on the CPU: every case under the float64 restatement alone (tests/lifter_ref.py) meets the conditions
that make it a fair test of the fp32 kernels, and prints what it measured.  Lifting: the entries the restatement marks as
rounding-dependent are at most 1 % of those compared.  Ties: nothing is marked and the expected order is the stable argsort.
Pixel loss: moving every ``0 < p < 1`` by 4 fp32 ulp moves the loss by at most 1e-6 relative and no gradient element by more than
1e-6 of its term size y, a tenth of the GPU tests' tolerance.  Saturated cases: enough exact zeros, exact ones and floored
entries, and no denormal.  A case that breaks a condition gets other inputs, never a wider bound."""
import numpy as np
import pytest

import lifter_cases as lc
import lifter_ref as ref


def _share(r, what):
    marked, compared = lc.exempt_share(r)
    print(f"{what}: {marked} marked of {compared} compared ({100.0 * marked / compared:.2f} %)")
    assert marked <= lc.MAX_EXEMPT_SHARE * compared, (what, marked, compared)
    return marked, compared


def test_cameras_are_all_distinct_and_the_ring_is_the_old_one():
    from test_lifter_gpu import lidar2img
    np.testing.assert_array_equal(lc.ring([(1600.0, 864.0)] * 6), lidar2img(6, 1600, 864))
    proj, wh = lc.cameras()
    assert proj.shape == (lc.B, lc.N, 4, 4) and wh.shape == (lc.B, lc.N, 2)
    flat = proj.reshape(-1, 16)
    assert len({m.tobytes() for m in flat}) == lc.B * lc.N
    assert len({tuple(v) for v in wh[0]}) == lc.N and not (wh[0] == wh[1]).all(-1).any()
    label, mask = lc.occupancy()
    occ = lc.packed(label, mask)
    assert 0.2 < occ.mean() < 0.28 and not mask.all() and not (occ[0] == occ[1]).all()


def test_lift_cases_cover_every_instantiation_and_chunk_edge():
    bins = sorted({S + 1 for S, _, _ in lc.LIFT_CASES})
    assert bins == [2, 63, 64, 65, 128, 192, 193, 256]
    assert {(b + 63) // 64 for b in bins} == {1, 2, 3, 4}
    assert all(a <= S + 1 for S, a, _ in lc.LIFT_CASES) and len(lc.LIFT_CASES) == 2 * (2 + 7 * 3)
    assert lc.B * lc.N * lc.H * lc.W // lc.B == 72 and lc.H % 2 == 0 and lc.W % 2 == 0


@pytest.mark.parametrize("S,a,stochastic", lc.LIFT_CASES)
def test_lift_case_exempt_share(S, a, stochastic):
    inp = lc.lift_inputs(S, a, stochastic)
    r = lc.oracle(inp)
    _share(r, f"S={S} a={a} stochastic={stochastic}")
    assert all(0 < s.shape[0] < r["keep"][0].size for s in r["scans"])      # every element keeps some slots and drops some
    assert r["pixel_gt"][..., :-1].any() and r["pixel_gt"][..., -1].any()
    ref.check_lift(r, r["scans"], r["src"], r["pixel_gt"], what="the restatement against itself", bound=0)


def test_further_lift_cases_exempt_share():
    for S, a, st in lc.NO_GT_CASES:
        r = lc.oracle(lc.lift_inputs(S, a, st), with_gt=False)
        assert r["pixel_gt"] is None and r["gt_exempt"] is None
        _share(r, f"no occupancy table, S={S} a={a} stochastic={st}")
    S, a, st = lc.OTHER_GRID_CASE
    r = lc.oracle(lc.lift_inputs(S, a, st, grid=lc.OTHER_GRID))
    _share(r, f"other grid, S={S} a={a}")
    assert r["pixel_gt"][..., :-1].any() and sum(s.shape[0] for s in r["scans"]) > 0
    inp = lc.edge_uniform_inputs()
    assert (inp["u"] == 0.0).sum() == 8 and (inp["u"] == lc.ONE_BELOW_1).sum() == 8 and lc.ONE_BELOW_1 < 1
    r = lc.oracle(inp)
    _share(r, "uniforms 0.0 and 1 - 2^-24")
    sure = lc.sure_top_uniform_slots(inp, r)
    kept = sum(bool(r["keep"][i][s]) for i, s in sure)
    print(f"uniforms 1 - 2^-24: {len(sure)} of 8 slots are decided whatever the rounding, {kept} of them kept")
    assert len(sure) >= 6 and 0 < kept
    assert all(r["slot_exempt"][i][s] for i, s in sure), "the rule marks them; the GPU test checks them apart"


def test_tie_case_is_exact_under_the_restatement():
    inp, expected = lc.tie_inputs()
    x = inp["logits"].reshape(-1, lc.TIE_S + 1)
    assert np.array_equal(x * 2, np.round(x * 2))
    r = lc.tie_oracle(inp)
    assert not r["slot_exempt"].any(), "a negative tie_tol and a far pc_range: nothing is exempt"
    # the expected entries are the stable argsort of the float64 pdf, and the kept points name their bins
    order = np.argsort(-ref.softmax64(x), axis=-1, kind="stable")
    want_bins = []
    for q, e in enumerate(expected):
        assert r["disabled"].reshape(-1)[q] == (e is None)
        if e is not None:
            assert order[q, :lc.TIE_A].tolist() == e, (q, order[q, :lc.TIE_A], e)
            want_bins += [min(k, lc.TIE_S - 1) for k in e]
    assert expected[5] is None and expected[9] == [190, 191, 0, 1]
    np.testing.assert_array_equal(lc.bins_of(r["scans"][0][:, 2], inp["depth"]), want_bins)
    # fp32 agrees on every comparison: equal logits give equal pdf entries, different ones different (or both exactly 0)
    p32 = ref.softmax64(x).astype(np.float32)
    for q in range(x.shape[0]):
        same_x = x[q][:, None] == x[q][None]
        same_p = p32[q][:, None] == p32[q][None]
        both_0 = (p32[q][:, None] == 0) & (p32[q][None] == 0)
        assert same_p[same_x].all() and (~same_p | both_0)[~same_x].all()
    ties = sum(len(set(x[q][e].tolist())) < lc.TIE_A for q, e in enumerate(expected) if e is not None)
    print(f"ties: {ties} of {len(expected)} pixels have an exact tie among their top {lc.TIE_A}")
    assert ties >= 12


@pytest.mark.parametrize("use_sigmoid", [False, True])
@pytest.mark.parametrize("bins", lc.LOSS_BINS)
def test_loss_cases_are_well_conditioned(bins, use_sigmoid):
    for rows in lc.LOSS_ROWS:
        x, gt = lc.loss_inputs(rows, bins, use_sigmoid)
        p = ref.pixel_probs(x, use_sigmoid)
        assert p.max() <= (0.9 if bins > 1 or use_sigmoid else 1.0)
        dl, dg = lc.probe(x, gt, use_sigmoid)
        print(f"{'sigmoid' if use_sigmoid else 'softmax'} bins={bins} rows={rows}: 4-ulp probe moves the loss {dl:.1e}, "
              f"the worst gradient element {dg:.1e} of y")
        assert dl <= lc.PROBE_RTOL and dg <= lc.PROBE_RTOL, (rows, bins, dl, dg)


def test_loss_terms_are_the_loss_and_bound_the_gradient():
    x, gt = lc.loss_inputs(17, 65, False)
    loss, g = ref.pixel_loss(x, gt, False)
    l2, g2, y = ref.pixel_loss_terms(x, gt, False)
    assert l2 == loss and np.array_equal(g, g2) and (np.abs(g) <= y).all()
    _, g, y = ref.pixel_loss_terms(x, gt, True)
    assert np.array_equal(np.abs(g), y)
    # one bin: p = 1, the gradient is 1 x (gp - gp)
    x, gt = lc.loss_inputs(17, 1, False)
    _, g, y = ref.pixel_loss_terms(x, gt, False)
    assert (g == 0).all() and ((y == 0) == gt).all()


@pytest.mark.parametrize("use_sigmoid", [False, True])
def test_saturated_case(use_sigmoid):
    x, gt = lc.saturated_inputs(use_sigmoid)
    p = ref.pixel_probs(x, use_sigmoid)
    tiny = float(np.finfo(np.float32).tiny)
    assert not ((p > 0) & (p < tiny)).any(), "a denormal p"
    floor = (p > 0) & (p < 1) & ((1.0 - p.astype(np.float64)) * p < float(np.float32(1e-12)))
    zeros, ones, floored = int((p == 0).sum()), int((p == 1).sum()), int(floor.sum())
    dl, dg = lc.probe(x, gt, use_sigmoid)
    loss, g, y = ref.pixel_loss_terms(x, gt, use_sigmoid)
    print(f"{'sigmoid' if use_sigmoid else 'softmax'}: {zeros} exact zeros, {ones} exact ones, {floored} floored; 4-ulp probe "
          f"moves the loss {dl:.1e}, the worst element {dg:.1e} of y; loss {loss:.4f}")
    assert zeros >= 1000 and ones >= 40 and floored >= 1000
    assert (g[floor] != 0).all()
    # nothing near the unstable band: every other p is far from both ends
    rest = p[(p > 0) & (p < 1) & ~floor]
    assert rest.min() > 1e-3 and rest.max() < 0.9
    assert dl <= lc.PROBE_RTOL and dg <= lc.PROBE_RTOL
    if not use_sigmoid:
        dom = x.argmax(-1)
        on = p[np.arange(x.shape[0]), dom] == 1
        clamp = on & ~gt[np.arange(x.shape[0]), dom] & (np.arange(x.shape[0]) % 3 == 0)
        assert clamp.sum() >= 10 and (on & gt[np.arange(x.shape[0]), dom]).sum() >= 10
    else:
        assert ((p == 1) & ~gt).sum() >= 1000 and ((p == 0) & gt).sum() >= 100      # both logs clamp at -100
