"""The geosem op (``gf_head_geosem_forward`` / ``gf_head_geosem_backward``) and ``GaussianHead``'s native route on the GPU.

* geosem: every element of the forward and of ``grad_logits`` against the torch expression bit for bit, the labels of the same
  launch against ``occupancy_labels``, ``grad_bin`` per row against float64 truth within the bound of an 18-term fp32 sum --
  at row counts around the wave (64) and workgroup (256) sizes, with zero rows, ``-0.0``, bins of 0 and 1, ``inf`` and ``NaN``,
  and with every pointer one float off a 16-byte boundary;
* the module: the four recorded calls (tests/golden/caller_head_*.npz) through ``native = True`` and ``native = False`` in one
  process, and the reference module's supervised layers (tests/golden/head_module.npz) through the native route.
Fixtures, tolerances and the label judge: tests/head_module_ref.py."""
import numpy as np
import pytest
import torch

import head_module_ref as R
from gaussianformer_amd import _lib
from gaussianformer_amd.head import GaussianHead, geosem, geosem_labels, occupancy_labels

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 255, 257, 2085]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(got, want, what):
    """Equal as int32 off the NaN positions, equal NaN masks."""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN masks differ"
    differ = (_bits(got) != _bits(want)) & ~nan
    assert not bool(differ.any()), f"{what}: {int(differ.sum())} elements differ in bits"


def _expression(logits, bins):
    """model/head/gaussian_head.py:166-168."""
    return torch.cat([logits[:, :-1] * bins.unsqueeze(-1), 1 - bins.unsqueeze(-1)], dim=-1)


def _case(N, device):
    """Seeded normal logits and cotangent, uniform bins; every 7th row's logits exact zeros, some of them -0.0; every 5th bin
    0 and the row after it 1; one row with inf, one with NaN."""
    gen = torch.Generator().manual_seed(100 + N)
    logits, bins, grad = torch.randn(N, 18, generator=gen), torch.rand(N, generator=gen), torch.randn(N, 18, generator=gen)
    logits[::7] = 0.0
    logits[::7, ::3] = -0.0
    bins[::5] = 0.0
    bins[1::5] = 1.0
    logits[min(2, N - 1), 4] = float("inf")
    logits[min(3, N - 1), 9] = float("nan")
    return logits.to(device), bins.to(device), grad.to(device)


def _raw_backward(logits, bins, grad):
    gl, gb = torch.empty_like(logits), torch.empty_like(bins)
    _lib.call("gf_head_geosem_backward", logits.device, logits.shape[0], 18, logits, bins, grad, gl, gb)
    return gl, gb


def _check_forward(logits, bins, out, labels, what):
    _same_bits(out, _expression(logits, bins), f"{what} out")
    assert labels.dtype == torch.int64 and torch.equal(labels, occupancy_labels(logits, bins, combine_geosem=True)), f"{what} labels"


def _check_backward(logits, bins, grad, gl, gb, what):
    _same_bits(gl[:, :17], grad[:, :17] * bins.unsqueeze(-1), f"{what} grad_logits")
    assert not bool(_bits(gl[:, 17]).any()), f"{what}: column 17 of grad_logits is not +0.0"
    l64, g64 = logits.double().cpu(), grad.double().cpu()
    terms = g64[:, :17] * l64[:, :17]
    truth = terms.sum(dim=1) - g64[:, 17]
    bound = 18 * 2.0 ** -23 * (terms.abs().sum(dim=1) + g64[:, 17].abs())
    finite = torch.isfinite(truth)
    got = gb.double().cpu()
    assert torch.equal(torch.isfinite(got), finite), f"{what}: grad_bin is finite on other rows than the truth"
    assert np.array_equal(got[~finite].float().numpy(), truth[~finite].float().numpy(), equal_nan=True), f"{what}: non-finite rows"
    ratio = ((got - truth).abs()[finite] / bound[finite].clamp_min(1e-300)).max() if bool(finite.any()) else 0.0
    print(f"{what}: grad_bin at {float(ratio):.3f} of the bound")
    assert bool(((got - truth).abs()[finite] <= bound[finite]).all()), f"{what}: grad_bin off by {float(ratio):.3f} of the bound"


@pytest.mark.parametrize("N", SIZES)
def test_geosem_forward_backward_bits_and_bound(gpu, N):
    logits, bins, grad = _case(N, gpu)
    out, labels = geosem_labels(logits, bins)
    _check_forward(logits, bins, out, labels, f"N={N}")
    _same_bits(geosem(logits, bins), out, f"N={N} geosem against geosem_labels")
    gl, gb = _raw_backward(logits, bins, grad)
    _check_backward(logits, bins, grad, gl, gb, f"N={N}")
    # a second run repeats the first bit for bit
    gl2, gb2 = _raw_backward(logits, bins, grad)
    assert torch.equal(_bits(gl), _bits(gl2)) and torch.equal(_bits(gb), _bits(gb2))
    # autograd through geosem is the raw backward
    lg, bl = logits.clone().requires_grad_(True), bins.clone().requires_grad_(True)
    res = geosem(lg, bl)
    assert res.requires_grad
    res.backward(grad)
    assert torch.equal(_bits(lg.grad), _bits(gl)) and torch.equal(_bits(bl.grad), _bits(gb))
    # the cotangent as the head's consumers send it: of the transposed view, so not contiguous here
    lg.grad = bl.grad = None
    geosem(lg, bl)[None].transpose(1, 2).backward(grad.t().contiguous()[None])
    assert torch.equal(_bits(lg.grad), _bits(gl)) and torch.equal(_bits(bl.grad), _bits(gb))


def test_geosem_with_every_pointer_one_float_off_a_16_byte_boundary(gpu):
    N = 257
    logits, bins, grad = _case(N, gpu)
    guard = 12345.0

    def off(n, src=None):
        """A view of ``n`` floats that starts 4 bytes past a 16-byte boundary, guard values around it."""
        buf = torch.full((n + 8,), guard, device=gpu)
        assert buf.data_ptr() % 16 == 0
        view = buf[1:1 + n]
        if src is not None:
            view.copy_(src.reshape(-1))
        return buf, view

    (_, lg), (_, bl), (_, g) = off(N * 18, logits), off(N, bins), off(N * 18, grad)
    lg, g = lg.view(N, 18), g.view(N, 18)
    (obuf, out), (gbuf, gl), (bbuf, gb) = off(N * 18), off(N * 18), off(N)
    labels = torch.empty(N, dtype=torch.int64, device=gpu)
    assert all(t.data_ptr() % 16 == 4 for t in (lg, bl, g, out, gl, gb))
    _lib.call("gf_head_geosem_forward", gpu, N, 18, lg, bl, out, labels)
    _lib.call("gf_head_geosem_backward", gpu, N, 18, lg, bl, g, gl, gb)
    want_out, want_labels = geosem_labels(logits, bins)
    want_gl, want_gb = _raw_backward(logits, bins, grad)
    assert torch.equal(_bits(out), _bits(want_out.reshape(-1))) and torch.equal(labels, want_labels)
    assert torch.equal(_bits(gl), _bits(want_gl.reshape(-1))) and torch.equal(_bits(gb), _bits(want_gb))
    _check_forward(logits, bins, out.view(N, 18), labels, "offset")
    _check_backward(logits, bins, grad, gl.view(N, 18), gb, "offset")
    for buf, n in ((obuf, N * 18), (gbuf, N * 18), (bbuf, N)):   # nothing written outside the views
        assert float(buf[0]) == guard and bool((buf[1 + n:] == guard).all())


def test_geosem_labels_replays_from_a_captured_graph(gpu):
    logits, bins, _ = _case(2085, gpu)
    eager_out, eager_labels = geosem_labels(logits, bins)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        geosem_labels(logits, bins)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, labels = geosem_labels(logits, bins)
    out.zero_()
    labels.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager_out)) and torch.equal(labels, eager_labels)
    # new contents of the same input buffers
    logits2, bins2, _ = _case(2084, gpu)
    logits[:2084].copy_(logits2)
    bins[:2084].copy_(bins2)
    want_out, want_labels = geosem_labels(logits, bins)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want_out)) and torch.equal(labels, want_labels)


def test_geosem_reproduces_the_recorded_pred_occ_on_the_device(gpu):
    """The pinned fact of tests/test_head_module.py, on the kernel: the recorded aggregator outputs give the recorded
    ``pred_occ`` bit for bit."""
    d = R.caller_fixture("prob_geosem")
    logits, bins = torch.from_numpy(d["call_out_logits"]).to(gpu), torch.from_numpy(d["call_out_bin_logits"]).to(gpu)
    out, labels = geosem_labels(logits, bins)
    assert np.array_equal(out[None].transpose(1, 2).cpu().numpy().view(np.int32), d["pred_occ"].view(np.int32))
    assert np.array_equal(labels.cpu().numpy()[None], d["final_occ"])


class _Recorded:
    """Keeps what the aggregator returned, whichever of its two entries the head called."""

    def __init__(self, agg):
        self.outs = []
        for entry in ("forward_from_rotations", "forward"):
            setattr(agg, entry, self._wrap(getattr(agg, entry), entry))

    def _wrap(self, fn, entry):
        def call(*args):
            res = fn(*args)
            self.outs.append((entry, res))
            return res
        return call


def _own_labels(name, pred_rows, agg_out):
    """``occupancy_labels`` of the module's own outputs."""
    if name == "base":
        return occupancy_labels(pred_rows)
    logits, bins, _ = agg_out
    if name == "prob_geosem":
        assert torch.equal(occupancy_labels(pred_rows), occupancy_labels(logits, bins, combine_geosem=True))
        return occupancy_labels(pred_rows)
    return occupancy_labels(logits, bins, threshold=0.5, empty_label=17)


@pytest.mark.parametrize("name", R.CALLER_CASES)
def test_recorded_caller_through_the_native_route_and_the_reference_sequence(gpu, name):
    prob = name != "base"
    head = GaussianHead(**R.caller_kwargs(name)).to(gpu).train()
    rec = _Recorded(head.aggregator)
    # native
    leaves = R.caller_leaves(name, gpu)
    out, loss = R.caller_call(head, name, leaves, gpu)
    loss.backward()
    assert [e for e, _ in rec.outs] == ["forward_from_rotations"]
    R.check_caller(head, name, out, leaves, f"native {name}")
    agg_out = rec.outs[-1][1]
    pred = out["pred_occ"][-1]
    rows = pred.transpose(1, 2)[0]
    assert pred.shape[:2] == (1, 18) and rows.is_contiguous()
    if prob:   # given the aggregator's outputs, the head's rows are the torch expression's bits
        logits, bins, dens = agg_out
        _same_bits(rows, _expression(logits, bins) if name == "prob_geosem" else logits, f"{name} rows")
        assert torch.equal(_bits(out["bin_logits"][-1][0]), _bits(bins)) and torch.equal(_bits(out["density"][-1][0]), _bits(dens))
    else:
        _same_bits(rows, agg_out, f"{name} rows")
    assert out["final_occ"].dtype == torch.int64 and torch.equal(out["final_occ"][0], _own_labels(name, rows, agg_out))
    # eval mode: the same bits as train mode's last layer, with and without a graph being recorded
    head.eval()
    for grad_mode in (torch.enable_grad, torch.no_grad):
        with grad_mode():
            out_e, _ = R.caller_call(head, name, leaves, gpu)
        assert len(out_e["pred_occ"]) == 1 and torch.equal(_bits(out_e["pred_occ"][-1]), _bits(pred)), grad_mode.__name__
        assert torch.equal(out_e["final_occ"], out["final_occ"])
    # the reference's op sequence in the same process, the same leaves requiring grad
    head.train()
    head.native = False
    head.zero_grad()
    rec.outs.clear()
    leaves2 = R.caller_leaves(name, gpu)
    out2, loss2 = R.caller_call(head, name, leaves2, gpu)
    loss2.backward()
    assert [e for e, _ in rec.outs] == ["forward"]
    R.check_caller(head, name, out2, leaves2, f"sequence {name}")
    R.check(pred.detach().cpu(), out2["pred_occ"][-1].detach().cpu(), f"{name} native against sequence pred_occ", R.out_tol(prob))
    for k in R.LEAVES:
        R.check(leaves[k].grad.cpu(), leaves2[k].grad.cpu(), f"{name} native against sequence grad_{k}", R.grad_tol(prob))
    rows2 = out2["pred_occ"][-1].transpose(1, 2)[0]
    if name == "prob_geosem":
        _same_bits(geosem(*rec.outs[-1][1][:2]), rows2, "geosem against the three torch ops on the sequence's aggregator outputs")
    assert torch.equal(out2["final_occ"][0], _own_labels(name, rows2.contiguous(), rec.outs[-1][1]))


@pytest.mark.parametrize("name", R.CONSTRUCTIONS)
def test_supervised_layers_through_the_native_route(gpu, name):
    rep, metas = R.module_inputs(name, gpu)
    for case, apply_loss_type, seed, train, fwd_kwargs in R.module_cases(name):
        head = GaussianHead(apply_loss_type=apply_loss_type, **R.module_kwargs(name)).to(gpu)
        head.train(train)
        np.random.seed(seed)
        with torch.no_grad():
            out = head(rep, metas, **fwd_kwargs)
        R.check_module_case(head, name, case, out, threshold=fwd_kwargs.get("sigmoid_thresh", 0.5))
