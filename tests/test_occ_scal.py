"""CPU checks of the occupancy loss's scene-class affinity terms (gf_occ_loss_scal_*, GF_OCC_SCAL): the float64 restatement
(tests/occ_scal_ref.py) is pinned to the reference's own loss with use_sem_geo_scal_loss=True (tests/golden/occ_scal.npz,
written by tools/make_golden_occ_scal.py), the new entry points refuse bad arguments before any HIP call, the old ones still
refuse the flag, the size queries honour it, and the drop-in module takes the option only with native_scal."""
import ctypes
import os

import numpy as np
import pytest

import occ_loss_ref
import occ_scal_ref as ref
from gaussianformer_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "occ_scal.npz")
WEIGHTS = dict(ce_weight=10.0, lovasz_weight=1.0, sem_scal_weight=0.7, geo_scal_weight=1.3)


@pytest.mark.parametrize("mode", ["softmax", "prob"])
def test_restatement_matches_reference_golden(mode):
    d = np.load(GOLDEN)
    pred = d[f"{mode}_pred"]                                       # [L, N, C]
    loss, grads = ref.occ_loss_with_scal_ref([p.T for p in pred], d["label"], d["mask"], class_weights=d[f"{mode}_class_weights"],
                                             lovasz_ignore=17, use_softmax=mode == "softmax", **WEIGHTS)
    want = float(d[f"{mode}_loss"])
    assert abs(loss - want) <= 1e-6 * abs(want), (loss, want)
    for g, w in zip(grads, d[f"{mode}_grad"]):
        w = w.T                                                    # [C, N]
        scale = np.abs(w).max()
        assert scale > 0
        assert np.abs(g - w).max() <= 1e-6 * scale, np.abs(g - w).max() / scale


def test_fixture_is_not_the_loss_without_the_terms():
    """The two terms are a visible share of the recorded loss and gradient: a restatement that dropped them would fail."""
    d = np.load(GOLDEN)
    for mode in ("softmax", "prob"):
        pred = [p.T for p in d[f"{mode}_pred"]]
        base, bgrads = occ_loss_ref.occ_loss_ref(pred, d["label"], d["mask"], class_weights=d[f"{mode}_class_weights"],
                                                 ce_weight=10.0, lovasz_weight=1.0, lovasz_ignore=17, use_softmax=mode == "softmax")
        want = float(d[f"{mode}_loss"])
        assert want - base > 0.05 * want
        w = d[f"{mode}_grad"][0].T
        assert np.abs(bgrads[0] - w).max() > 10 * 1e-6 * np.abs(w).max()      # ten times the bound of the test above


def test_restatement_shift_steps_and_edges():
    C = 18
    label = np.repeat([0, 5, 17], [600, 600, 1200])
    hot = np.zeros((C, len(label)), np.float32)
    hot[label, np.arange(len(label))] = 1
    # exact rows: precision, recall and specificity are exactly 1.0f and take two shift steps each -> six f(0.99998f) of sem
    # / 2 classes, three of geo
    loss, grads, sems, geos = ref.occ_scal_ref([hot], label, use_softmax=False)
    assert abs(loss - 1.2016174e-4) <= 1e-6 * 1.2016174e-4, loss
    assert sems[0] == geos[0]
    # rows one-hot at the next class: recall 0 (one step up), S_i = 0 skips precision
    off = np.zeros_like(hot)
    off[(label + 1) % C, np.arange(len(label))] = 1
    loss, grads, _, _ = ref.occ_scal_ref([off], label, use_softmax=False)
    assert abs(loss - 30.02480) <= 1e-6 * 30.02480, loss
    assert abs(np.abs(grads[0]).max() - 125.0) <= 1e-3
    # a ratio that 8 shift steps do not bring into range (inputs that are no probabilities): NaN; 6 steps are taken
    big = hot.copy()
    big[5, label == 5] = 2.0
    assert np.isnan(ref.occ_scal_ref([big], label, use_softmax=False)[0])
    big[5, label == 5] = 1.0 + 5e-5
    assert np.isfinite(ref.occ_scal_ref([big], label, use_softmax=False)[0])
    assert ref.scal_f(np.float32(1.0 + 5e-5))[2] and not ref.scal_f(np.float32(1.0 + 9e-5))[2] and not ref.scal_f(np.float32(-1e-4))[2]
    # no class of 0 .. C-2 among V: NaN; so for labels out of range
    assert np.isnan(ref.occ_scal_ref([hot], np.where(label == 17, 17, 255), use_softmax=False)[0])
    bad = label.copy()
    bad[3] = 40
    assert np.isnan(ref.occ_scal_ref([hot], bad, use_softmax=False)[0])


def _args(flags=_lib.GF_OCC_SCAL, L=1, N=100, empty=17, preds=True, label=1, loss=1, ws=1, nbytes=1 << 40, scratch=1,
          sbytes=1 << 40):
    arr = (ctypes.c_void_p * L)(*([8] * L)) if preds else None
    return (L, N, 18, flags, arr, 1, 18, label, None, 1, 10.0, 1.0, 0.7, 1.3, 17, 255, empty), (loss, ws, nbytes, scratch, sbytes, None)


def test_scal_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    S = _lib.GF_OCC_SCAL
    cases = [
        (dict(flags=0), b"GF_OCC_SCAL"),
        (dict(flags=_lib.GF_OCC_PROB | _lib.GF_OCC_NO_LOVASZ), b"GF_OCC_SCAL"),
        (dict(flags=S | 64), b"unknown flags"),
        (dict(empty=18), b"empty_label = 18"),
        (dict(empty=-1), b"empty_label = -1"),
        (dict(preds=False), b"null pointer"),
        (dict(label=None), b"null pointer"),
        (dict(ws=None), b"null pointer"),
        (dict(loss=None), b"null loss"),
        (dict(scratch=None), b"null scratch"),
    ]
    for kw, msg in cases:
        head, tail = _args(**kw)
        rc = lib.gf_occ_loss_scal_forward(*head, *tail)
        assert rc == -1, kw
        assert msg in lib.gf_last_error() and b"gf_occ_loss_scal_forward" in lib.gf_last_error(), (kw, lib.gf_last_error())
    # a workspace or a scratch of the size the queries give WITHOUT the flag is too small
    for L, N in ((1, 100), (4, 640000)):
        head, tail = _args(L=L, N=N, nbytes=lib.gf_occ_loss_workspace_bytes(L, N, 18, 0))
        assert lib.gf_occ_loss_scal_forward(*head, *tail) == -2 and b"workspace" in lib.gf_last_error()
        head, tail = _args(L=L, N=N, sbytes=lib.gf_occ_loss_scratch_bytes(L, N, 18, 0))
        assert lib.gf_occ_loss_scal_forward(*head, *tail) == -2 and b"scratch" in lib.gf_last_error()
        head, _ = _args(L=L, N=N)
        garr = (ctypes.c_void_p * L)(*([8] * L))
        rc = lib.gf_occ_loss_scal_backward(*head, 1, garr, 1, lib.gf_occ_loss_workspace_bytes(L, N, 18, 0), None)
        assert rc == -2 and b"workspace" in lib.gf_last_error()
    head, _ = _args()
    garr = (ctypes.c_void_p * 1)(8)
    assert lib.gf_occ_loss_scal_backward(*head, None, garr, 1, 1 << 40, None) == -1 and b"null gradient" in lib.gf_last_error()
    head, _ = _args(flags=0)
    assert lib.gf_occ_loss_scal_backward(*head, 1, garr, 1, 1 << 40, None) == -1 and b"GF_OCC_SCAL" in lib.gf_last_error()
    head, _ = _args(empty=18)
    assert lib.gf_occ_loss_scal_backward(*head, 1, garr, 1, 1 << 40, None) == -1 and b"empty_label" in lib.gf_last_error()


def test_old_entry_points_refuse_the_flag():
    lib = _lib.load()
    arr = (ctypes.c_void_p * 1)(8)
    for flags in (_lib.GF_OCC_SCAL, _lib.GF_OCC_SCAL | _lib.GF_OCC_PROB):
        rc = lib.gf_occ_loss_forward(1, 100, 18, flags, arr, 1, 18, 1, None, 1, 10.0, 1.0, 17, 255, 17, 1, 1, 1 << 40, 1, 1 << 40, None)
        assert rc == -1 and b"unknown flags" in lib.gf_last_error()
        rc = lib.gf_occ_loss_backward(1, 100, 18, flags, arr, 1, 18, 1, None, 1, 10.0, 1.0, 17, 255, 17, 1, arr, 1, 1 << 40, None)
        assert rc == -1 and b"unknown flags" in lib.gf_last_error()


def test_size_queries_honour_the_flag():
    """Without the flag: the sizes of the layout as it was (256-byte sections, written out here); with it: more, by the
    sections of the two terms (a, b in the workspace; the S, N and T partials and their sums in the scratch)."""
    lib = _lib.load()
    S = _lib.GF_OCC_SCAL

    def up(n):
        return (n + 255) // 256 * 256

    for L, N in ((1, 100), (2, 1500), (1, 640000), (4, 640000), (8, 257)):
        NB, T, C = (N + 255) // 256, (N + 2047) // 2048, 18
        ws0 = up(64 * 4) + up(N * 4) + up(L * N * C * 4) + up((2 * L + L * C) * 8)
        sc0 = (up(NB * 4) + up(NB * C * 4) + up(L * NB * 2 * 8) + 2 * up(L * C * N * 8) + up(L * C * 256 * T * 4) + up(L * C * 256 * 4)
               + up(L * C * T * 4) + up(L * C * T * 8))
        for other in (0, _lib.GF_OCC_PROB | _lib.GF_OCC_MASK, _lib.GF_OCC_NO_LOVASZ):
            assert lib.gf_occ_loss_workspace_bytes(L, N, C, other) == ws0
            assert lib.gf_occ_loss_scratch_bytes(L, N, C, other) == sc0
            assert lib.gf_occ_loss_workspace_bytes(L, N, C, other | S) == ws0 + up(2 * L * C * 4)
            assert lib.gf_occ_loss_scratch_bytes(L, N, C, other | S) == sc0 + up(2 * L * C * NB * 8) + up(C * NB * 4) + up((2 * L * C + C) * 8)
    assert lib.gf_occ_loss_workspace_bytes(9, 100, 18, S) == 0 and lib.gf_occ_loss_scratch_bytes(1, 100, 17, S) == 0


def test_module_takes_the_option_only_with_native_scal(monkeypatch):
    import torch
    from gaussianformer_amd.occupancy_loss import OccupancyLoss
    assert OccupancyLoss.native_scal is False
    with pytest.raises(ValueError, match="use_sem_geo_scal_loss.*native_scal = True"):
        OccupancyLoss(lovasz_ignore=17)                       # the reference's default: use_sem_geo_scal_loss=True
    monkeypatch.setattr(OccupancyLoss, "native_scal", True)
    m = OccupancyLoss(lovasz_ignore=17)
    assert m.use_sem_geo_scal_loss and m.loss_voxel_sem_scal_weight == 1.0 and m.loss_voxel_geo_scal_weight == 1.0
    m = OccupancyLoss(lovasz_ignore=17, multi_loss_weights=dict(loss_voxel_sem_scal_weight=0.7, loss_voxel_geo_scal_weight=1.3))
    assert (m.loss_voxel_sem_scal_weight, m.loss_voxel_geo_scal_weight) == (0.7, 1.3)
    assert not OccupancyLoss(lovasz_ignore=17, use_sem_geo_scal_loss=False).use_sem_geo_scal_loss
    # what the module hands to the functional op
    import gaussianformer_amd.occupancy_loss as mod
    seen = {}
    monkeypatch.setattr(mod, "occupancy_loss", lambda *a, **k: seen.update(k) or 0.0)
    m.loss_voxel([torch.zeros(1)], None, None)
    assert (seen["sem_scal_weight"], seen["geo_scal_weight"]) == (0.7, 1.3)
    OccupancyLoss(lovasz_ignore=17, use_sem_geo_scal_loss=False).loss_voxel([torch.zeros(1)], None, None)
    assert seen["sem_scal_weight"] is None and seen["geo_scal_weight"] is None

