"""The HIP path, through the C ABI, against the frozen fixtures of REFERENCE outputs (tests/golden/*.npz, produced by
tools/make_golden.py from oracle/_ref = the reference's own kernels on an MI355X).  Needs only the committed fixtures:
neither /root/reference nor oracle/_ref at run time."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import oracle

from util import (GRAD_RTOL, assert_grad_close, assert_grad_rows_close, assert_logits_close, assert_prob_grad_rows_close,
                  hip_splat_backward, hip_splat_forward, print_grad_rows, splat_truth_grads, to_dev, whole_grid_rows)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", ["splat_base", "splat_base_signed", "splat_prob", "splat_prob_fast"])
def test_splat_matches_reference_fixture(gpu, name):
    import torch
    from gaussianformer_amd import _lib
    from gaussianformer_amd.local_aggregate import splat_box_volumes
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert "oracle/_ref" in str(d["producer"])
    si = SimpleNamespace(variant=str(d["variant"]), pts=d["pts"], means3D=d["means3D"], opacities=d["opacities"],
                         semantics=d["semantics"], H=int(d["H"]), W=int(d["W"]), D=int(d["D"]))
    pi, mi, radii, cov6 = d["points_int"], d["means_int"], d["radii"], d["cov6"]
    prob = si.variant == "prob"
    whole = whole_grid_rows(mi, radii, si.H, si.W, si.D)
    if prob:   # the fixture's own gradients cancel in fp32 like any: float64 truth, the oracle's error on the row as the yardstick
        og = oracle.splat_backward("prob", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6, si.H, si.W, si.D,
                                   d["out_grad"], bin_grad=d["bin_grad"], density_grad=d["density_grad"],
                                   fwd=oracle.splat_forward("prob", si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii,
                                                            cov6, si.H, si.W, si.D))
        truth = splat_truth_grads(si, pi, mi, radii, cov6, d["out_grad"], d["bin_grad"], d["density_grad"])
    print()
    # default flags (base variant on the dense grid: the matrix-core kernel, north_star's 1e-4 bound), the exact-fp32
    # tile kernel and the arbitrary-points kernel (both 1e-5)
    for flags, tol in ((0, 1e-5 if prob else 1e-4), (_lib.GF_EXACT_FP32, 1e-5), (_lib.GF_PTS_GENERAL, 1e-5)):
        got, t, state, fwd_t = hip_splat_forward(gpu, si, pi, mi, radii, cov6, flags=flags)
        for k in (("logits", "bin_logits", "density", "probability") if prob else ("logits",)):
            assert_logits_close(got[k], d[k], what=f"{name}: {k} vs reference fixture (flags {flags})", tol=tol)
        grads = hip_splat_backward(gpu, si, t, state, fwd_t, d["out_grad"], d["bin_grad"] if prob else None,
                                   d["density_grad"] if prob else None, flags=flags)
        for k, g in zip(("means3D_grad", "opacity_grad", "semantics_grad", "cov3D_grad"), grads):
            assert_grad_close(g, d[k], what=f"{name}: {k} vs reference fixture", rtol=1e-4)
        for i, (k, g) in enumerate(zip(("means3D_grad", "opacity_grad", "semantics_grad", "cov3D_grad"), grads)):
            if prob:
                assert_prob_grad_rows_close(g, truth[i], og[i], what=f"{name}: {k} vs float64 (flags {flags})")
            else:
                print_grad_rows(f"{name}: {k} vs fixture (flags {flags})",
                                assert_grad_rows_close(g, d[k], whole, what=f"{name}: {k} vs reference fixture", rtol=GRAD_RTOL))
    vols, R = splat_box_volumes(torch.from_numpy(mi).to(gpu), torch.from_numpy(radii).to(gpu), si.H, si.W, si.D)
    assert R == int(d["num_rendered"]) and np.array_equal(vols.cpu().numpy().astype(np.uint32), d["tiles_touched"])


def test_daf_matches_reference_fixture(gpu):
    import torch
    from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF
    d = np.load(os.path.join(GOLDEN, "daf.npz"))
    assert "oracle/_ref" in str(d["producer"])
    feat, ss, st, loc, w = to_dev(gpu, d["mc_ms_feat"], d["spatial_shape"], d["scale_start_index"],
                                  d["sampling_location"], d["weights"])
    feat.requires_grad_(True); loc.requires_grad_(True); w.requires_grad_(True)
    out = DAF.apply(feat, ss, st, loc, w)
    assert_logits_close(out.detach().cpu().numpy(), d["output"], what="daf output vs reference fixture", tol=1e-5)
    out.backward(torch.from_numpy(d["grad_output"]).to(gpu))
    assert_grad_close(feat.grad.cpu().numpy(), d["grad_mc_ms_feat"], "grad_mc_ms_feat vs reference fixture", rtol=1e-4)
    assert_grad_close(loc.grad.cpu().numpy(), d["grad_sampling_location"], "grad_sampling_location vs reference fixture", rtol=1e-4)
    assert_grad_close(w.grad.cpu().numpy(), d["grad_weights"], "grad_weights vs reference fixture", rtol=1e-4)
