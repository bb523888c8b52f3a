"""The evaluation metric without a GPU: the numpy restatement (miou_ref.py) against the fixture recorded from the
reference's own ``MeanIoU`` (tests/golden/miou.npz), ``gaussianformer_amd.metric.MeanIoU`` on CPU tensors against both,
exact totals past 2^24, the epoch's all-reduce over two gloo ranks, and the C entry points' argument refusals."""
import ctypes
import logging
import multiprocessing as mp
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gaussianformer_amd import _lib  # noqa: E402
from gaussianformer_amd.metric import MeanIoU  # noqa: E402
from miou_cases import CASES, GOLDEN, PERMUTED, WITH_EMPTY, load_case, random_frame  # noqa: E402
from miou_ref import MiouRef  # noqa: E402

CPU = torch.device("cpu")
# percent scale: the reference divides exactly represented fp32 integers once (relative error 2^-24 on values <= 1), times 100
EPOCH_TOL = 1e-5


@pytest.fixture(scope="module")
def fix():
    return np.load(GOLDEN)


def make(settings, device=CPU, **kw):
    s = dict(settings)
    classes, empty = s.pop("class_indices"), s.pop("empty_label")
    return MeanIoU(classes, empty, [f"class{c}" for c in classes], device=device, **s, **kw)


def totals_of(m):
    return torch.stack([m.total_seen, m.total_correct, m.total_positive]).cpu().numpy()


@pytest.mark.parametrize("case", CASES)
def test_ref_matches_the_reference_fixture(fix, case):
    settings, frames, totals, (miou, occ) = load_case(fix, case)
    ref = MiouRef(**settings)
    for f, frame in enumerate(frames):
        ref.frame(*frame)
        assert np.array_equal(ref.totals, totals[f]), (case, f)
    got = ref.epoch()
    assert abs(got[0] - miou) <= EPOCH_TOL and abs(got[1] - occ) <= EPOCH_TOL
    assert ref.unfiltered == 0


def test_fixture_holds_the_cases_it_is_meant_to(fix):
    _, frames, totals, _ = load_case(fix, "dict_band")
    sem = frames[0][1]["semantics"]
    assert sem.dtype == np.uint8 and (sem == 0).any() and (sem == 255).any()
    z = np.nonzero((sem != 0).reshape(-1, sem.shape[-1]).any(0))[0]
    assert z.min() > 0 and z.max() < sem.shape[-1] - 1                       # a middle band: the filter removes predictions
    assert (frames[0][0][..., :z.min()] != 17).any()
    z1 = np.nonzero((frames[1][1]["semantics"] != 0).reshape(-1, 16).any(0))[0]
    assert z1.min() == z1.max()                                              # min_z == max_z
    assert load_case(fix, "dict_d5")[1][0][1]["semantics"].shape[-1] == 5
    s, fr, tot, _ = load_case(fix, "absent")
    assert tot[-1][0][s["class_indices"].index(9)] == 0 and (fr[0][1] == 255).any() and (fr[0][1] == 0).any()
    # the two dict cases differ (the mask matters), and so do the two flat ones
    assert not np.array_equal(totals, load_case(fix, "dict_nomask")[2])
    assert not np.array_equal(load_case(fix, "eval_mask")[2], load_case(fix, "eval_nomask")[2])


@pytest.mark.parametrize("case", CASES)
def test_class_on_cpu_matches_the_fixture(fix, case):
    settings, frames, totals, (miou, occ) = load_case(fix, case)
    m = make(settings)
    for f, (out, tgt, mask) in enumerate(frames):
        keep = out.copy()
        m._after_step(torch.from_numpy(out), tgt, None if mask is None else torch.from_numpy(mask.astype(bool)))
        assert np.array_equal(out, keep)                                     # outputs is not written
        assert np.array_equal(totals_of(m), totals[f]), (case, f)
    got = m._after_epoch()
    assert isinstance(got[0], float) and isinstance(got[1], float)
    assert abs(got[0] - miou) <= EPOCH_TOL and abs(got[1] - occ) <= EPOCH_TOL


@pytest.mark.parametrize("shape", [(1, 1, 16), (6, 5, 16), (7, 3, 5)])
@pytest.mark.parametrize("classes", [list(range(1, 17)), PERMUTED, WITH_EMPTY])
def test_class_on_cpu_matches_ref_on_random_frames(shape, classes):
    rng = np.random.default_rng(hash((shape, tuple(classes))) % (1 << 32))
    for dict_form in (False, True):
        for u8 in (False, True):
            for masked in (False, True):
                for filt in ((False, True) if dict_form else (False,)):
                    settings = dict(class_indices=classes, empty_label=17, use_mask=masked, dataset_empty_label=0, filter_minmax=filt)
                    m, ref = make(settings), MiouRef(**settings)
                    for band in (None, (shape[-1] // 3, shape[-1] // 2), (0, 0), (shape[-1] - 1, shape[-1] - 1)):
                        frame = random_frame(rng, shape, dict_form, u8, masked, band)
                        ref.frame(*frame)
                        m._after_step(*frame)
                        assert np.array_equal(totals_of(m), ref.totals), (dict_form, u8, masked, filt, band)
                    a, b = m._after_epoch(), ref.epoch()
                    assert a[0] == pytest.approx(b[0], abs=1e-9) and a[1] == pytest.approx(b[1], abs=1e-9, nan_ok=True)


def test_frame_without_an_occupied_target_is_counted_unfiltered_and_reported(caplog):
    settings = dict(class_indices=list(range(1, 17)), empty_label=17, use_mask=True, dataset_empty_label=0, filter_minmax=True)
    rng = np.random.default_rng(5)
    out = rng.integers(0, 18, (6, 5, 16))
    tgt = {"semantics": np.zeros((6, 5, 16), np.uint8), "mask_camera": (rng.random((6, 5, 16)) < 0.7).astype(np.uint8)}
    m, ref = make(settings, logger=logging.getLogger("miou-test")), MiouRef(**settings)
    m._after_step(out, tgt)
    ref.frame(out, tgt)
    assert ref.unfiltered == 1 and np.array_equal(totals_of(m), ref.totals)
    assert m._status.tolist() == [1, 1]
    with caplog.at_level(logging.INFO, logger="miou-test"):
        m._after_epoch()
    assert any(r.levelno == logging.WARNING and "1 of 1 frames" in r.getMessage() for r in caplog.records)
    assert any("Validation per class iou" in r.getMessage() for r in caplog.records)


def test_logits_form_on_cpu_is_the_label_form_of_the_head_rule():
    rng = np.random.default_rng(11)
    N = 480
    logits = torch.from_numpy(rng.standard_normal((N, 18)).astype(np.float32))
    logits[::7, 3] = logits[::7].max(dim=1).values            # tied maxima: the first wins
    bins = torch.from_numpy(rng.random(N).astype(np.float32))
    tgt = torch.from_numpy(rng.integers(0, 18, N))
    settings = dict(class_indices=list(range(1, 17)), empty_label=17)
    for kw, labels in ((dict(), logits.argmax(1)),
                       (dict(bin_logits=bins, threshold=0.4), torch.where(bins > 0.4, logits.argmax(1), 17)),
                       (dict(bin_logits=bins, combine_geosem=True),
                        torch.cat([logits[:, :-1] * bins[:, None], 1 - bins[:, None]], 1).argmax(1))):
        a, b = make(settings), make(settings)
        a._after_step_logits(logits, tgt, **kw)
        b._after_step(labels, tgt)
        assert np.array_equal(totals_of(a), totals_of(b)) and totals_of(a)[2].sum() > 0


def test_reset_and_attributes():
    m = make(dict(class_indices=[1, 2, 3], empty_label=17))
    assert m.total_seen.dtype == torch.int64 and m.total_seen.shape == (4,) and m.num_classes == 3
    m._after_step(torch.tensor([1, 2, 17, 3]), torch.tensor([1, 3, 17, 3]))
    assert m.total_seen.tolist() == [1, 0, 2, 3] and m.total_correct.tolist() == [1, 0, 1, 3] and m.total_positive.tolist() == [1, 1, 1, 3]
    assert m._status.tolist() == [1, 0]
    m.reset()
    assert not totals_of(m).any() and m._status.tolist() == [0, 0]
    with pytest.raises(ValueError):
        MeanIoU([1, 40], 17, ["a", "b"], device=CPU)
    with pytest.raises(ValueError):
        m._after_step(torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    from misc.metric_util import MeanIoU as DropIn
    assert DropIn is MeanIoU


def test_drop_in_package_does_not_hide_the_reference_tree_misc_modules(tmp_path, monkeypatch):
    """The reference's ``misc`` directory (no ``__init__.py``) also holds ``checkpoint_util`` and ``tb_wrapper``: with both
    trees on the path ``misc.metric_util`` is this repository's and the others still import."""
    import importlib
    (tmp_path / "misc").mkdir()
    (tmp_path / "misc" / "tb_wrapper_stand_in.py").write_text("WHERE = 'the other tree'\n")
    (tmp_path / "misc" / "metric_util.py").write_text("MeanIoU = None\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    for name in [n for n in sys.modules if n == "misc" or n.startswith("misc.")]:
        monkeypatch.delitem(sys.modules, name)
    assert importlib.import_module("misc.tb_wrapper_stand_in").WHERE == "the other tree"
    assert importlib.import_module("misc.metric_util").MeanIoU is MeanIoU


def test_totals_past_2_to_24_stay_exact():
    """The reference's float32 totals stop being exact at 2^24; these are integers."""
    settings = dict(class_indices=list(range(1, 17)), empty_label=17)
    m, ref = make(settings), MiouRef(**settings)
    m._totals += 1 << 40
    rng = np.random.default_rng(3)
    for _ in range(3):
        frame = random_frame(rng, (6, 5, 16), False, False, True)
        m._after_step(*frame)
        ref.frame(*frame)
    assert np.array_equal(totals_of(m) - (1 << 40), ref.totals)
    assert int(np.float32((1 << 40) + int(ref.totals[0, -1]))) != (1 << 40) + int(ref.totals[0, -1])   # float32 could not hold it


# ------------------------------------------------------------------ the epoch's all-reduce, 2-rank gloo
def _rank_frames(rank):
    rng = np.random.default_rng(100 + rank)
    return [random_frame(rng, (6, 5, 16), True, True, True, band) for band in ((2, 9), None)]


_SETTINGS = dict(class_indices=list(range(1, 17)), empty_label=17, use_mask=True, dataset_empty_label=0, filter_minmax=True)


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = make(_SETTINGS)
    for frame in _rank_frames(rank):
        m._after_step(*frame)
    q.put((rank, m._after_epoch(), totals_of(m)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_epoch_equals_single_process_over_both_ranks_frames():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r: (e, t) for r, e, t in (q.get(timeout=180) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    single = make(_SETTINGS)
    for rank in range(2):
        for frame in _rank_frames(rank):
            single._after_step(*frame)
    want = single._after_epoch()
    for r in range(2):
        assert got[r][0] == want and np.array_equal(got[r][1], totals_of(single))


# ------------------------------------------------------------------ the C entry points refuse bad arguments before any HIP call
def test_argument_refusals_through_the_c_abi():
    lib = _lib.load()
    cls = (ctypes.c_int * 16)(*range(1, 17))
    buf = torch.zeros(1 << 16, dtype=torch.int64)      # host memory: every call below is refused before a launch
    p = buf.data_ptr()
    F = _lib.GF_MIOU_FILTER_MINMAX
    need = lib.gf_miou_workspace_size(480, 16, F)
    assert need >= 16 * 102 * 4 and lib.gf_miou_workspace_size(0, 16, F) > 0
    # the recorded sizes (this query is not in tests/golden/workspace_bytes.json, the table of the *_bytes queries): 104 words per
    # slice and slot, whole 256-byte sections; 640 000 voxels are 105 slots of 16 slices, or 313 of one
    assert [lib.gf_miou_workspace_size(*a) for a in ((480, 16, F), (480, 16, 0), (0, 16, F), (640000, 16, F), (640000, 16, 0))] == [
        6656, 512, 6656, 698880, 130304]
    assert lib.gf_miou_workspace_size(480, 16, 0) < need                      # D counts with the filter only
    assert lib.gf_miou_workspace_size(640000, 16, F) > need
    assert lib.gf_miou_workspace_size(-1, 16, 0) == 0 and lib.gf_miou_workspace_size(480, 0, F) == 0
    assert lib.gf_miou_workspace_size(480, 7, F) == 0 and lib.gf_miou_workspace_size(480, 16, 64) == 0

    def step(N=480, D=16, flags=F, outputs=p, targets=p, K=16, classes=cls, totals=p, status=p, ws=p, nbytes=need):
        return lib.gf_miou_step(N, D, flags, outputs, targets, None, K, classes, 17, 0, totals, status, ws, nbytes, None)

    def step_logits(C=18, mode=0, logits=p, bins=None, N=480, D=16, flags=F, K=16, ws=p, nbytes=need):
        return lib.gf_miou_step_logits(N, D, flags, C, mode, logits, bins, 0.5, p, None, K, cls, 17, 0, p, p, ws, nbytes, None)

    def refused(rc, word, code=-1):
        assert rc == code and word in lib.gf_last_error().decode(), (rc, lib.gf_last_error())

    refused(step(outputs=None), "null pointer")
    refused(step(targets=None), "null pointer")
    refused(step(totals=None), "null pointer")
    refused(step(status=None), "null pointer")
    refused(step(classes=None), "null pointer")
    refused(step(N=-1), "bad size")
    refused(step(flags=64), "unknown flag")
    refused(step(K=0), "num_classes")
    refused(step(K=33), "num_classes")
    refused(step(classes=(ctypes.c_int * 16)(*([1] * 15 + [32]))), "class index")
    refused(step(classes=(ctypes.c_int * 16)(*([1] * 15 + [-1]))), "class index")
    refused(step(D=0), "D")
    refused(step(D=65), "D")
    refused(step(D=7), "multiple of D")
    refused(step(ws=None), "workspace", -2)
    refused(step(nbytes=need - 1), "workspace", -2)
    assert b"gf_miou_step:" in lib.gf_last_error()
    refused(step_logits(C=17), "18")
    refused(step_logits(mode=3), "unknown mode")
    refused(step_logits(logits=None), "null pointer")
    refused(step_logits(mode=1), "bin_logits")
    refused(step_logits(nbytes=0), "workspace", -2)
    assert b"gf_miou_step_logits:" in lib.gf_last_error()
    with pytest.raises(RuntimeError, match=r"gf_miou_step failed \(code -1\): .*num_classes"):
        _lib.call("gf_miou_step", CPU, 480, 16, F, buf, buf, None, 0, cls, 17, 0, buf, buf, buf, need)
