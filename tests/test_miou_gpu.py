"""The evaluation metric's kernels (csrc/miou.hip) on the GPU: exact to the last count against the numpy restatement
(miou_ref.py) and the fixture recorded from the reference (tests/golden/miou.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gaussianformer_amd.head import occupancy_labels  # noqa: E402
from gaussianformer_amd.metric import MeanIoU  # noqa: E402
from miou_cases import CASES, GOLDEN, PERMUTED, WITH_EMPTY, load_case, random_frame  # noqa: E402
from miou_ref import MiouRef  # noqa: E402

pytestmark = pytest.mark.gpu
CLASSES = {"1..16": list(range(1, 17)), "permuted": PERMUTED, "with_empty": WITH_EMPTY}


def make(settings, dev):
    s = dict(settings)
    classes, empty = s.pop("class_indices"), s.pop("empty_label")
    return MeanIoU(classes, empty, [f"class{c}" for c in classes], device=dev, **s)


def totals_of(m):
    return torch.stack([m.total_seen, m.total_correct, m.total_positive]).cpu().numpy()


def on(dev, frame):
    """A frame's arrays as device tensors (the dict form keeps its dict)."""
    out, tgt, mask = frame
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if isinstance(tgt, dict):
        return t(out), {k: t(v) for k, v in tgt.items()}, None
    return t(out), t(tgt), t(mask)


@pytest.mark.parametrize("case", CASES)
def test_fixture_replayed_through_the_kernels(gpu, case):
    settings, frames, totals, (miou, occ) = load_case(np.load(GOLDEN), case)
    m = make(settings, gpu)
    for f, (out, tgt, mask) in enumerate(frames):
        o = torch.from_numpy(out).to(gpu)
        keep = o.clone()
        m._after_step(o, tgt, None if mask is None else torch.from_numpy(mask.astype(bool)).to(gpu))   # the dict form as numpy, like the reference's caller
        assert np.array_equal(totals_of(m), totals[f]), (case, f)
        assert torch.equal(o, keep)
    got = m._after_epoch()
    assert abs(got[0] - miou) <= 1e-5 and abs(got[1] - occ) <= 1e-5
    assert m._status.tolist() == [len(frames), 0]


@pytest.mark.parametrize("shape", [(1, 1, 16), (6, 5, 16), (7, 3, 5), (40, 40, 16)])
@pytest.mark.parametrize("classes", list(CLASSES))
def test_random_frames_match_ref_exactly(gpu, shape, classes):
    """int64 and uint8 targets, with and without a mask, flat and dict form, filter on and off, 0 and 255 among the labels."""
    rng = np.random.default_rng(sum(shape) * 31 + len(classes))
    for dict_form in (False, True):
        for u8 in (False, True):
            for masked in (False, True):
                for filt in ((False, True) if dict_form else (False,)):
                    settings = dict(class_indices=CLASSES[classes], empty_label=17, use_mask=masked, dataset_empty_label=0, filter_minmax=filt)
                    m, ref = make(settings, gpu), MiouRef(**settings)
                    for band in (None, (shape[-1] // 3, shape[-1] // 2)):
                        frame = random_frame(rng, shape, dict_form, u8, masked, band)
                        ref.frame(*frame)
                        m._after_step(*on(gpu, frame))
                    assert np.array_equal(totals_of(m), ref.totals), (dict_form, u8, masked, filt)
                    assert m._status.tolist() == [2, ref.unfiltered]      # (16 voxels can come without an occupied one)


def test_full_grid_once(gpu):
    """200 x 200 x 16, the evaluation's own shape: every workgroup slot in use, dict form with remap, filter and mask."""
    rng = np.random.default_rng(640000)
    settings = dict(class_indices=CLASSES["1..16"], empty_label=17, use_mask=True, dataset_empty_label=0, filter_minmax=True)
    frame = random_frame(rng, (200, 200, 16), True, True, True, (2, 12))
    m, ref = make(settings, gpu), MiouRef(**settings)
    ref.frame(*frame)
    m._after_step(*on(gpu, frame))
    assert np.array_equal(totals_of(m), ref.totals)
    # ... and the flat int64 form with a mask on the same voxels, from a pointer that is only 8-byte aligned
    out, tgt, mask = random_frame(rng, (640001,), False, False, True)
    settings = dict(class_indices=PERMUTED, empty_label=17)
    m, ref = make(settings, gpu), MiouRef(**settings)
    ref.frame(out[1:], tgt[1:], mask[1:])
    o, t, k = on(gpu, (out, tgt, mask))
    m._after_step(o[1:], t[1:], k[1:])
    assert np.array_equal(totals_of(m), ref.totals)


def test_non_contiguous_outputs(gpu):
    rng = np.random.default_rng(8)
    settings = dict(class_indices=CLASSES["1..16"], empty_label=17, use_mask=True, dataset_empty_label=0, filter_minmax=True)
    out, tgt, _ = random_frame(rng, (6, 5, 16), True, True, True, (4, 9))
    wide = torch.from_numpy(np.repeat(out, 2, axis=-1)).to(gpu)
    wide[..., 1::2] = 3                                       # what a reader that ignored the strides would count
    view = wide[..., ::2]
    assert not view.is_contiguous() and np.array_equal(view.cpu().numpy(), out)
    m, ref = make(settings, gpu), MiouRef(**settings)
    ref.frame(out, tgt)
    m._after_step(view, tgt)
    assert np.array_equal(totals_of(m), ref.totals)
    tr = torch.from_numpy(np.ascontiguousarray(out.transpose(2, 0, 1))).to(gpu).permute(1, 2, 0)   # [6,5,16] with z outermost in memory
    assert not tr.is_contiguous()
    m.reset()
    m._after_step(tr, tgt)
    assert np.array_equal(totals_of(m), ref.totals)


@pytest.mark.parametrize("D", [16, 5])
def test_filter_edges(gpu, D):
    rng = np.random.default_rng(D)
    shape = (6, 5, D)
    settings = dict(class_indices=CLASSES["1..16"], empty_label=17, use_mask=True, dataset_empty_label=0, filter_minmax=True)
    for name, band in (("slice 0 only", (0, 0)), ("slice D-1 only", (D - 1, D - 1)), ("min_z == max_z", (2, 2)), ("none occupied", (D, D))):
        frame = random_frame(rng, shape, True, True, True, band)
        m, ref = make(settings, gpu), MiouRef(**settings)
        ref.frame(*frame)
        m._after_step(*on(gpu, frame))
        assert np.array_equal(totals_of(m), ref.totals), name
        assert m._status.tolist() == [1, int(band[0] == D)] and ref.unfiltered == int(band[0] == D), name   # counted unfiltered, and said so
    # a mask that hides every occupied voxel: the z range still comes from the unmasked targets
    out, tgt, _ = random_frame(rng, shape, True, True, True, (1, 3))
    tgt["mask_camera"] = (tgt["semantics"] == 0).astype(np.uint8)
    assert (tgt["semantics"] != 0).any() and not (tgt["mask_camera"].astype(bool) & (tgt["semantics"] != 0)).any()
    m, ref = make(settings, gpu), MiouRef(**settings)
    ref.frame(out, tgt)
    m._after_step(*on(gpu, (out, tgt, None)))
    assert np.array_equal(totals_of(m), ref.totals) and ref.totals[0, -1] == 0 and m._status.tolist() == [1, 0]
    unfiltered = MiouRef(**dict(settings, filter_minmax=False))
    unfiltered.frame(out, tgt)
    assert not np.array_equal(unfiltered.totals, ref.totals)          # the filter did something on this frame


@pytest.mark.parametrize("N", [1, 63, 64, 1000, 5000])
def test_logits_form_equals_labels_then_step(gpu, N):
    """All three modes of the head's rule, rows with tied maxima, an unaligned logits view; N = 5000 takes three workgroups
    and the z filter (25 x 25 x 8)."""
    rng = np.random.default_rng(N)
    logits = torch.from_numpy(rng.standard_normal((N, 18)).astype(np.float32)).to(gpu)
    logits[::5, 7] = logits[::5].max(dim=1).values            # tied maxima: the first maximal channel wins
    logits[::9] = 0.25                                        # ... all 18 equal
    bins = torch.from_numpy(rng.random(N).astype(np.float32)).to(gpu)
    flat = torch.zeros(N * 18 + 1, device=gpu)
    unaligned = flat[1:].view(N, 18)
    unaligned.copy_(logits)
    assert unaligned.data_ptr() % 16 != 0
    dict_form = N % 200 == 0
    shape = (N // 200, 25, 8) if dict_form else (N,)
    settings = dict(class_indices=CLASSES["1..16"], empty_label=17, use_mask=True, dataset_empty_label=0, filter_minmax=True)
    _, tgt, mask = on(gpu, random_frame(rng, shape, dict_form, True, True, (2, 5) if dict_form else None))
    for kw in (dict(), dict(bin_logits=bins, threshold=0.4), dict(bin_logits=bins, combine_geosem=True)):
        labels = occupancy_labels(logits, kw.get("bin_logits"), kw.get("threshold", 0.5), 17, kw.get("combine_geosem", False))
        want = make(settings, gpu)
        want._after_step(labels, tgt, mask)
        for lg in (logits, unaligned):
            m = make(settings, gpu)
            m._after_step_logits(lg, tgt, mask, **kw)
            assert np.array_equal(totals_of(m), totals_of(want)), (kw.keys(), lg is unaligned)
        assert totals_of(want)[2].sum() > 0 or N == 1


def test_accumulation_and_reset(gpu):
    rng = np.random.default_rng(21)
    settings = dict(class_indices=PERMUTED, empty_label=17, use_mask=True, dataset_empty_label=0, filter_minmax=True)
    m = make(settings, gpu)
    parts = []
    for band in ((1, 3), None, (7, 12)):
        frame = random_frame(rng, (6, 5, 16), True, True, True, band)
        parts.append(MiouRef(**settings).frame(*frame))
        m._after_step(*on(gpu, frame))
    assert np.array_equal(totals_of(m), sum(parts)) and m._status.tolist() == [3, 0]
    m.reset()
    assert not totals_of(m).any() and m._status.tolist() == [0, 0]
    m._after_step(torch.zeros(0, dtype=torch.int64, device=gpu), torch.zeros(0, dtype=torch.int64, device=gpu))   # N == 0: a frame, no counts
    assert not totals_of(m).any() and m._status.tolist() == [1, 0]


def test_step_is_captured_in_a_graph_and_replayed(gpu):
    """A step that read anything back could not be captured: warm-up, capture on a linear stream, three replays with new
    contents in the static inputs; the totals are the reference's for all four frames."""
    rng = np.random.default_rng(77)
    shape = (40, 40, 16)
    settings = dict(class_indices=CLASSES["1..16"], empty_label=17, use_mask=True, dataset_empty_label=0, filter_minmax=True)
    frames = [random_frame(rng, shape, True, True, True, band) for band in ((3, 9), None, (0, 4), (15, 15))]
    ref = MiouRef(**settings)
    for frame in frames:
        ref.frame(*frame)
    m = make(settings, gpu)
    out, tgt, _ = on(gpu, frames[0])
    stream = torch.cuda.Stream(gpu)
    stream.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(stream):
        m._after_step(out, tgt)                               # warm-up: counts frame 0, sizes the stream's scratch
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        m._after_step(out, tgt)
    for frame in frames[1:]:
        o, t, _ = on(gpu, frame)
        with torch.cuda.stream(stream):
            out.copy_(o)
            tgt["semantics"].copy_(t["semantics"])
            tgt["mask_camera"].copy_(t["mask_camera"])
            graph.replay()
    stream.synchronize()
    assert np.array_equal(totals_of(m), ref.totals) and m._status.tolist() == [4, 0]
