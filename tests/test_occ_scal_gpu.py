"""GPU checks of the occupancy loss's scene-class affinity terms (occupancy_loss(..., sem_scal_weight=, geo_scal_weight=),
csrc/occ_loss.hip): the reference's own loss with the terms (tests/golden/occ_scal.npz), the float64 restatement
(tests/occ_scal_ref.py) at sizes around one voxel block, additivity with the loss without the terms, the exact edges of the
shift loops in prob mode, bitwise reproducibility, the absence of host synchronisation, graph capture and the drop-in module.

Where no other bound is named: loss to 1e-5 relative, each gradient row to 1e-5 of the layer's largest entry."""
import os

import numpy as np
import pytest
import torch

import occ_loss_ref
import occ_scal_ref as ref
from gaussianformer_amd.occupancy_loss import OccupancyLoss, occupancy_loss
from test_occ_loss_gpu import CW, _close, _run

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "occ_scal.npz")
WEIGHTS = dict(ce_weight=10.0, lovasz_weight=1.0, sem_scal_weight=0.7, geo_scal_weight=1.3)
ALONE = dict(ce_weight=0.0, use_lovasz=False, sem_scal_weight=0.7, geo_scal_weight=1.3)
C = 18


def _inputs(N, L, seed, prob=False, masked=False):
    """Labels over all 18 classes (40 % empty, 3 % ignore_index), logits or probabilities [L, N, C], a mask of 80 %."""
    rng = np.random.default_rng(seed)
    label = rng.integers(0, C, N)
    label[rng.random(N) < 0.4] = 17
    label[rng.random(N) < 0.03] = 255
    x = (2.0 * rng.standard_normal((L, N, C))).astype(np.float32)
    if prob:
        x = np.exp(x - x.max(-1, keepdims=True))
        x = (x / x.sum(-1, keepdims=True)).astype(np.float32)
    return x, label.astype(np.int64), (rng.random(N) < 0.8) if masked else None


def _loss_close(got, want, rel=1e-5):
    assert np.isfinite(want) and abs(got - want) <= rel * abs(want), (got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["softmax", "prob"])
def test_matches_reference_golden(gpu, mode):
    d = np.load(GOLDEN)
    loss, grads = _run(gpu, d[f"{mode}_pred"], d["label"], d["mask"], class_weights=torch.from_numpy(d[f"{mode}_class_weights"]).to(gpu),
                       lovasz_ignore=17, use_softmax=mode == "softmax", **WEIGHTS)
    _loss_close(loss, float(d[f"{mode}_loss"]))
    _close(grads, [g.T for g in d[f"{mode}_grad"]], 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("N", [255, 257, 1500])
def test_scal_alone_matches_restatement(gpu, N, L, masked):
    """The two terms alone (ce_weight = 0, no Lovász): a partial block, one block plus one voxel, a ragged last block."""
    for prob in (False, True):
        x, label, mask = _inputs(N, L, seed=N + L + 7 * masked, prob=prob, masked=masked)
        loss, grads = _run(gpu, x, label, mask, use_softmax=not prob, **ALONE)
        want, wgrads, _, _ = ref.occ_scal_ref([r.T for r in x], label, mask, sem_scal_weight=0.7, geo_scal_weight=1.3,
                                              use_softmax=not prob)
        _loss_close(loss, want)
        _close(grads, wgrads, 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["view", "contiguous"])
@pytest.mark.parametrize("ignore_empty", [False, True])
def test_scal_alone_layouts_and_ignore_empty(gpu, layout, ignore_empty):
    x, label, mask = _inputs(1500, 3, seed=21, masked=True)
    loss, grads = _run(gpu, x, label, mask, layout=layout, ignore_empty=ignore_empty, **ALONE)
    want, wgrads, _, _ = ref.occ_scal_ref([r.T for r in x], label, mask, sem_scal_weight=0.7, geo_scal_weight=1.3,
                                          ignore_empty=ignore_empty)
    _loss_close(loss, want)
    _close(grads, wgrads, 1e-5)
    if ignore_empty:
        assert all(not g[:, label == 17].any() for g in grads)        # no voxel of the empty class is in V


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["softmax", "prob"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("N", [255, 257, 1500])
def test_all_terms_match_restatement(gpu, mode, N, L):
    """CE + Lovász + both terms on the fixture's inputs, whose errors are separated within every class (a subset of them
    is too), so that no near-tie rule is needed; lovasz_ignore = 17: the empty voxels are in V but not in the Lovász term."""
    d = np.load(GOLDEN)
    x = d[f"{mode}_pred"][[0, 1, 0][:L], :N]
    label, mask = d["label"][:N], d["mask"][:N]
    for m in (mask, None):
        kw = dict(lovasz_ignore=17, use_softmax=mode == "softmax", **WEIGHTS)
        loss, grads = _run(gpu, x, label, m, **kw)
        want, wgrads = ref.occ_loss_with_scal_ref([r.T for r in x], label, m, class_weights=CW, **kw)
        _loss_close(loss, want)
        _close(grads, wgrads, 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["softmax", "prob"])
def test_additive_with_the_loss_without_the_terms(gpu, mode):
    d = np.load(GOLDEN)
    x, label, mask = d[f"{mode}_pred"], d["label"], d["mask"]
    kw = dict(lovasz_ignore=17, use_softmax=mode == "softmax")
    both = _run(gpu, x, label, mask, **kw, **WEIGHTS)
    old = _run(gpu, x, label, mask, ce_weight=10.0, lovasz_weight=1.0, **kw)
    alone = _run(gpu, x, label, mask, use_softmax=mode == "softmax", **ALONE)
    _loss_close(both[0], old[0] + alone[0], 1e-6)
    _close(both[1], [a + b for a, b in zip(old[1], alone[1])], 1e-6)
    # one weight given: the other counts as 0
    sem = _run(gpu, x, label, mask, ce_weight=0.0, use_lovasz=False, sem_scal_weight=0.7, use_softmax=mode == "softmax")
    geo = _run(gpu, x, label, mask, ce_weight=0.0, use_lovasz=False, geo_scal_weight=1.3, use_softmax=mode == "softmax")
    _loss_close(alone[0], sem[0] + geo[0], 1e-6)
    _close(alone[1], [a + b for a, b in zip(sem[1], geo[1])], 1e-6)


def _one_hot(label, shift=0):
    hot = np.zeros((1, len(label), C), np.float32)
    hot[0, np.arange(len(label)), (label + shift) % C] = 1
    return hot


@pytest.mark.gpu
def test_prob_mode_edges(gpu):
    label = np.repeat([0, 5, 17], [600, 600, 1200]).astype(np.int64)
    kw = dict(ce_weight=0.0, use_lovasz=False, sem_scal_weight=1.0, geo_scal_weight=1.0, use_softmax=False)
    rkw = dict(use_softmax=False)
    # rows one-hot at the label: every ratio is exactly 1.0f (a count of 256 or more + 1e-5 rounds back to the count) and
    # takes two shift steps
    hot = _one_hot(label)
    loss, grads = _run(gpu, hot, label, **kw)
    want, wgrads, _, _ = ref.occ_scal_ref([hot[0].T], label, **rkw)
    _loss_close(want, 1.2016174e-4, 1e-6)
    _loss_close(loss, want)
    _close(grads, wgrads, 1e-5)
    # rows one-hot at the next class: recall 0, S_i = 0 skips the precision
    off = _one_hot(label, 1)
    loss, grads = _run(gpu, off, label, **kw)
    want, wgrads, _, _ = ref.occ_scal_ref([off[0].T], label, **rkw)
    _loss_close(want, 30.02480, 1e-6)
    assert abs(np.abs(wgrads[0]).max() - 125.0) < 1e-3
    _loss_close(loss, want)
    _close(grads, wgrads, 1e-5)
    # a class present in the labels whose column is all zeros
    x, lab, _ = _inputs(1500, 1, seed=33, prob=True)
    assert (lab == 6).any()
    x[:, :, 6] = 0
    loss, grads = _run(gpu, x, lab, **kw)
    want, wgrads, _, _ = ref.occ_scal_ref([x[0].T], lab, **rkw)
    _loss_close(loss, want)
    _close(grads, wgrads, 1e-5)
    # inputs that are no probabilities: a recall of 2 is still out of range after the 8 shift steps the op allows (the
    # reference would take 100 001 host round trips) -- NaN; 1 + 5e-5 needs 6 steps and is taken as the reference takes it
    for value, finite in ((2.0, False), (1.0 + 5e-5, True)):
        big = hot.copy()
        big[0, label == 5, 5] = value
        loss, grads = _run(gpu, big, label, **kw)
        want, wgrads, _, _ = ref.occ_scal_ref([big[0].T], label, **rkw)
        assert np.isfinite(want) == finite
        if finite:
            _loss_close(loss, want)
            _close(grads, wgrads, 1e-5)
        else:
            assert np.isnan(loss)
    # no class of 0 .. C-2 among the voxels of V: the reference divides by zero in Python; the op gives NaN
    none = np.where(np.arange(len(label)) % 3 == 0, 255, 17).astype(np.int64)
    loss, _ = _run(gpu, hot, none, **kw)
    assert np.isnan(loss)
    assert np.isnan(ref.occ_scal_ref([hot[0].T], none, **rkw)[0])


@pytest.mark.gpu
def test_nan_rules_apply_to_the_voxels_of_v(gpu):
    x, label, _ = _inputs(1500, 1, seed=34)
    bad = label.copy()
    bad[123] = 40
    assert np.isnan(_run(gpu, x, bad, **ALONE)[0])
    k = int(np.nonzero(label == 4)[0][0])
    xn = x.copy()
    xn[0, k, 3] = np.inf
    assert np.isnan(_run(gpu, xn, label, **ALONE)[0])
    # ... and not to a voxel outside V (label 255)
    k = int(np.nonzero(label == 255)[0][0])
    xn = x.copy()
    xn[0, k, 3] = np.inf
    assert _run(gpu, xn, label, **ALONE)[0] == _run(gpu, x, label, **ALONE)[0]


@pytest.mark.gpu
def test_bitwise_reproducible(gpu):
    d = np.load(GOLDEN)
    kw = dict(lovasz_ignore=17, **WEIGHTS)
    a = _run(gpu, d["softmax_pred"], d["label"], d["mask"], **kw)
    b = _run(gpu, d["softmax_pred"], d["label"], d["mask"], **kw)
    assert a[0] == b[0]
    for ga, gb in zip(a[1], b[1]):
        assert np.array_equal(ga, gb)


def _device_inputs(gpu):
    d = np.load(GOLDEN)
    leaves = [torch.from_numpy(r).to(gpu)[None].requires_grad_(True) for r in d["softmax_pred"]]
    return d, leaves, torch.from_numpy(d["label"]).to(gpu)[None], torch.from_numpy(d["mask"]).to(gpu)[None], torch.from_numpy(CW).to(gpu)


@pytest.mark.gpu
def test_forward_and_backward_do_not_synchronise(gpu):
    d, leaves, lab, m, cw = _device_inputs(gpu)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = occupancy_loss([t.transpose(1, 2) for t in leaves], lab, m, class_weights=cw, lovasz_ignore=17, **WEIGHTS)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    want, wgrads = _run(gpu, d["softmax_pred"], d["label"], d["mask"], class_weights=cw, lovasz_ignore=17, **WEIGHTS)
    assert loss.item() == want
    for t, w in zip(leaves, wgrads):
        assert np.array_equal(t.grad[0].cpu().numpy().T, w)


@pytest.mark.gpu
def test_graph_capture_replays_eager_bits(gpu):
    """As test_occ_loss_gpu: the eager run's autograd graph is gone before the capture (results detached)."""
    _, leaves, lab, m, cw = _device_inputs(gpu)

    def step():
        for t in leaves:
            t.grad = None
        loss = occupancy_loss([t.transpose(1, 2) for t in leaves], lab, m, class_weights=cw, lovasz_ignore=17, **WEIGHTS)
        loss.backward()
        return loss

    eager = step().detach().clone()
    eager_grads = [t.grad.detach().clone() for t in leaves]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    for t in leaves:
        t.grad = None
    with torch.cuda.graph(g):
        loss = step()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, eager)
        for t, e in zip(leaves, eager_grads):
            assert torch.equal(t.grad, e)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["softmax", "prob"])
def test_module_equals_functional(gpu, mode, monkeypatch):
    monkeypatch.setattr(OccupancyLoss, "native_scal", True)
    cfg = dict(occ_loss_ref.SOLID_CFG if mode == "softmax" else occ_loss_ref.PROB_CFG, use_sem_geo_scal_loss=True,
               multi_loss_weights=dict(loss_voxel_ce_weight=10.0, loss_voxel_lovasz_weight=1.0, loss_voxel_sem_scal_weight=0.7,
                                       loss_voxel_geo_scal_weight=1.3))
    d = np.load(GOLDEN)
    x, label, mask = d[f"{mode}_pred"], d["label"], d["mask"]
    module = OccupancyLoss(**cfg).to(gpu)
    leaves = [torch.from_numpy(r).to(gpu)[None].requires_grad_(True) for r in x]
    inputs = {"pred_occ": [t.transpose(1, 2) for t in leaves], "sampled_xyz": None,
              "sampled_label": torch.from_numpy(label).to(gpu)[None], "occ_mask": torch.from_numpy(mask).to(gpu)[None]}
    got = module(inputs)
    got.backward()
    want, wgrads = _run(gpu, x, label, mask, class_weights=module.class_weights, lovasz_ignore=17, use_softmax=mode == "softmax",
                        **WEIGHTS)
    assert got.item() == want
    _loss_close(want, float(d[f"{mode}_loss"]))
    for t, w in zip(leaves, wgrads):
        assert np.array_equal(t.grad[0].cpu().numpy().T, w)
