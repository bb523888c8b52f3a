"""``gaussianformer_amd.head.GaussianHead`` and the geosem entry points without a device.

The drop-in on CPU tensors runs the reference's own op sequence on this package's pieces (``GaussianArgs._forward_torch``
with the closed-form Sigma^-1, ``aggregator(..., CovInv)``, the three torch ops, ``argmax``) with the raw splat served by the
CPU oracle (tests/ref_shim.py ``cpu_kernels``) -- the route that tests/test_head_module_gpu.py compares the native one
with.  Here it is held to what the reference's module did (tests/golden/head_module.npz, tools/make_golden_head.py:
state dict, supervised layers, outputs, labels) and to the four recorded calls with their gradients
(tests/golden/caller_head_*.npz).  Tolerances: tests/head_module_ref.py."""
import numpy as np
import pytest
import torch

import head_module_ref as R
import ref_shim
from gaussianformer_amd import _lib
from gaussianformer_amd.head import GaussianHead, geosem, geosem_labels


def test_geosem_entry_points_check_their_arguments_before_any_device_call():
    lib = _lib.load()
    one = 1 << 20   # (a non-null address: never dereferenced, every call below is refused or empty)
    for rc in (lib.gf_head_geosem_forward(4, 17, one, one, one, None, None),
               lib.gf_head_geosem_backward(4, 17, one, one, one, one, one, None)):
        assert rc == -1 and b"18" in lib.gf_last_error()
    for rc in (lib.gf_head_geosem_forward(-1, 18, one, one, one, None, None),
               lib.gf_head_geosem_backward(-1, 18, one, one, one, one, one, None)):
        assert rc == -1 and b"size" in lib.gf_last_error()
    assert lib.gf_head_geosem_forward(4, 18, one, one, None, None, None) == -1 and b"null" in lib.gf_last_error()
    assert lib.gf_head_geosem_backward(4, 18, one, one, one, None, one, None) == -1 and b"null" in lib.gf_last_error()
    assert lib.gf_head_geosem_backward(4, 18, one, one, one, one, None, None) == -1 and b"null" in lib.gf_last_error()
    assert lib.gf_head_geosem_forward(1 << 40, 18, one, one, one, None, None) == -1 and b"large" in lib.gf_last_error()
    assert lib.gf_head_geosem_forward(0, 18, None, None, None, None, None) == 0
    assert lib.gf_head_geosem_backward(0, 18, None, None, None, None, None, None) == 0


def test_geosem_refuses_cpu_tensors():
    for op in (geosem, geosem_labels):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            op(torch.zeros(4, 18), torch.zeros(4))


def test_the_closed_form_covariance_inverse_is_the_reference_sequence():
    """The CPU route's Sigma^-1 (R^T diag(1 / s^2) R) against the reference's five lines (oracle/prepare_ref.py) in float64."""
    from gaussianformer_amd.head import _covariance_inverse_torch
    from oracle import prepare_ref
    gen = torch.Generator().manual_seed(3)
    s = torch.rand(2, 9, 3, generator=gen, dtype=torch.float64) + 0.05
    q = torch.randn(2, 9, 4, generator=gen, dtype=torch.float64)
    want = prepare_ref.covariance_inverse(s, q)
    assert ((_covariance_inverse_torch(s, q) - want).abs() <= 1e-12 * want.abs().max()).all()


@pytest.mark.parametrize("name", R.CONSTRUCTIONS)
def test_construction_has_the_reference_state_dict(name):
    d = R.module_fixture()
    for case, apply_loss_type, _, _, _ in R.module_cases(name):
        head = GaussianHead(apply_loss_type=apply_loss_type, **R.module_kwargs(name))
        state = head.state_dict()
        assert sorted(state) == d[f"{name}_state_names"].tolist(), (case, sorted(state))
        for k, v in state.items():
            want = d[f"{name}_state_{k}"]
            assert tuple(v.shape) == want.shape and v.dtype == torch.float32 and np.array_equal(v.numpy(), want), (case, k)
        assert [k for k, _ in head.named_parameters()] == d[f"{name}_param_names"].tolist()
        assert "native" not in state and GaussianHead.native is True
    assert d["base_param_names"].tolist() == ["empty_scalar"] and d["prob_param_names"].tolist() == []
    assert {"zero_tensor", "aggregator.pc_min"} <= set(d["prob_state_names"].tolist())


def test_attributes_and_aggregators_are_the_reference_heads():
    from gaussianformer_amd.local_aggregate import LocalAggregator, LocalAggregatorProb, LocalAggregatorProbFast
    kw = R.module_kwargs("prob")
    head = GaussianHead(apply_loss_type="random_2", **kw)
    assert type(head.aggregator) is LocalAggregatorProb and head.apply_loss_type == "random" and head.random_apply_loss_layers == 2
    assert (head.with_emtpy, head.combine_geosem, head.use_localaggprob, head.empty_label, head.num_classes, head.dataset_type) == \
        (False, False, True, 17, 18, "nusc")
    fast = GaussianHead(apply_loss_type="fixed_0_2", use_localaggprob_fast=True, **kw)
    assert type(fast.aggregator) is LocalAggregatorProbFast and fast.apply_loss_type == "fixed" and fast.fixed_apply_loss_layers == [0, 2]
    kw = R.module_kwargs("base")
    base = GaussianHead(apply_loss_type="all", **dict(kw, cuda_kwargs=dict(kw["cuda_kwargs"], check_inputs=False, matrix_cores=False)))
    assert type(base.aggregator) is LocalAggregator and base.with_emtpy and base.apply_loss_type == "all"
    assert base.aggregator.check_inputs is False and base.aggregator.matrix_cores is False
    base.init_weights()
    with pytest.raises(NotImplementedError):
        GaussianHead(apply_loss_type="some", **kw)
    xyz, label = base._sampling(torch.zeros(1, 2, 3, 4, 3), torch.zeros(1, 2, 3, 4))
    assert xyz.shape == (1, 24, 3) and label.shape == (1, 24)


@pytest.mark.parametrize("name", R.CONSTRUCTIONS)
def test_supervised_layers_outputs_and_labels_match_the_reference_module(name):
    """Every (apply_loss_type, numpy seed, mode) of the fixture: the same number of ``pred_occ`` entries -- under
    ``'random_2'`` the layers the reference drew --, each within the tolerance, ``final_occ`` on the decisive voxels."""
    rep, metas = R.module_inputs(name, "cpu")
    for case, apply_loss_type, seed, train, fwd_kwargs in R.module_cases(name):
        head = GaussianHead(apply_loss_type=apply_loss_type, **R.module_kwargs(name))
        head.train(train)
        np.random.seed(seed)
        with ref_shim.cpu_kernels(), torch.no_grad():
            out = head(rep, metas, **fwd_kwargs)
        R.check_module_case(head, name, case, out, threshold=fwd_kwargs.get("sigmoid_thresh", 0.5))


def test_prepare_gaussian_args_returns_the_reference_tuple():
    rep, _ = R.module_inputs("base", "cpu")
    head = GaussianHead(apply_loss_type="all", **R.module_kwargs("base"))
    means, origi_opa, opacities, scales, cov_inv = head.prepare_gaussian_args(rep[0]["gaussian"])
    g = rep[0]["gaussian"].means.shape[1] + 1
    assert means.shape == (1, g, 3) and origi_opa.shape == (1, g, 1) and opacities.shape == (1, g, 18) and scales.shape == (1, g, 3)
    assert cov_inv.shape == (1, g, 3, 3)
    assert opacities[0, -1, 17] == 10.0 and opacities[0, :-1, 17].abs().max() == 0


@pytest.mark.parametrize("name", R.CALLER_CASES)
def test_recorded_caller_replayed_through_the_dropin_on_the_cpu_oracle(name):
    """tests/golden/caller_head_<name>.npz: train mode, one layer -- ``pred_occ``, ``bin_logits``, ``density``, ``final_occ`` on
    the decisive voxels and the gradients of the fixture's loss in every leaf and in ``empty_scalar``."""
    head = GaussianHead(**R.caller_kwargs(name)).train()
    leaves = R.caller_leaves(name, "cpu")
    with ref_shim.cpu_kernels():
        out, loss = R.caller_call(head, name, leaves, "cpu")
        loss.backward()
    R.check_caller(head, name, out, leaves, f"cpu {name}")


def test_geosem_formula_reproduces_the_fixture_bit_for_bit():
    """A pinned fact the GPU test repeats on the device: the torch expression on the recorded aggregator outputs of
    caller_head_prob_geosem.npz IS its ``pred_occ`` (20 of its rows have ``bin == 0``)."""
    d = R.caller_fixture("prob_geosem")
    logits, bins = torch.from_numpy(d["call_out_logits"]), torch.from_numpy(d["call_out_bin_logits"])
    assert int((bins == 0).sum()) == 20
    geo = torch.cat([logits[:, :-1] * bins.unsqueeze(-1), 1 - bins.unsqueeze(-1)], dim=-1)
    assert np.array_equal(geo[None].transpose(1, 2).numpy().view(np.int32), d["pred_occ"].view(np.int32))
