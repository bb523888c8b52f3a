"""``SparseConv3D``'s native tail (``native_tail``, ``forward(residual=, norm=)``): one case per shipped config family --

    single      conv -> "norm"                                                  (nuscenes_gs144000)
    single_proj conv -> output_proj -> "norm"                                   (nuscenes_gs25600_solid)
    multi_proj  3 x (conv + bias -> LayerNorm -> ReLU) -> output_proj, "add", "norm"   (prob/)

at bs = 2, 301 anchors per batch, kernel 3, width 128, about three anchors per occupied cell, with both ``duplicates`` modes.
The float64 truth is the dense definition (oracle/subm_ref.py) and float64 torch layers; the yardstick Y of DESIGN.md §3.13b's
rule is the same module with ``native_tail = False``.  ReLU is continuous, so a forward needs no kink filter."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from gaussianformer_amd.sparse_conv import SparseConv3D, SubMConv3d
from oracle.subm_ref import subm_conv3d_dense
from row_judge import bound, held, max_error, spy  # noqa: F401  (spy is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BS, G, E, K = 2, 301, 128, 3
PC_RANGE, GRID = [-5.0, -5.0, -2.5, 5.0, 5.0, 2.5], [2.0, 2.0, 1.0]      # 5 x 5 x 5 cells per batch
FAMILIES = {"single": dict(use_out_proj=False, use_multi_layer=False, residual=False),
            "single_proj": dict(use_out_proj=True, use_multi_layer=False, residual=False),
            "multi_proj": dict(use_out_proj=True, use_multi_layer=True, residual=True)}
BUILD = ["gf_subm_voxelize", "gf_subm_rulebook_count", "gf_subm_rulebook_fill"]
LAUNCHES = {"single": BUILD + ["gf_subm_conv_apply_epilogue"],
            "single_proj": BUILD + ["gf_subm_conv_apply_scratch", "gf_deform_output_forward"],
            "multi_proj": BUILD + ["gf_subm_conv_apply_epilogue"] * 3 + ["gf_deform_output_forward"]}


class Block:
    def __init__(self, family, duplicates):
        f = FAMILIES[family]
        torch.manual_seed(11)
        self.m = SparseConv3D(E, E, PC_RANGE, GRID, use_out_proj=f["use_out_proj"], kernel_size=K, use_multi_layer=f["use_multi_layer"],
                              duplicates=duplicates).to(DEV).eval()
        self.norm = nn.LayerNorm(E).to(DEV)
        with torch.no_grad():
            for ln in [l for l in self.m.modules() if isinstance(l, nn.LayerNorm)] + [self.norm]:
                ln.weight.copy_(1 + 0.3 * torch.randn(E))
                ln.bias.copy_(0.3 * torch.randn(E))
        self.x = torch.randn(BS, G, E).to(DEV)
        self.anchor = torch.randn(BS, G, 11).to(DEV)
        self.residual = torch.randn(BS, G, E).to(DEV) if f["residual"] else None
        self.duplicates = duplicates

    def call(self, native, **kw):
        self.m.native_tail = native
        try:
            with torch.no_grad():
                return self.m(self.x, self.anchor, residual=self.residual, norm=self.norm, **kw)
        finally:
            del self.m.native_tail          # (back to the class attribute)

    def truth(self):
        m, d = self.m, lambda t: t.detach().cpu().double()
        idx = m.voxel_indices(self.anchor).cpu()
        mask = d(m.last_rulebook.representative_mask()) if self.duplicates == "last" else 1.0
        x = d(self.x).flatten(0, 1)
        for layer in (m.layer if isinstance(m.layer, nn.ModuleList) else [m.layer]):
            if isinstance(layer, SubMConv3d):
                x = subm_conv3d_dense(x * mask, idx, d(layer.weight), BS, m._spatial, K)
                x = x if layer.bias is None else x + d(layer.bias)
            elif isinstance(layer, nn.LayerNorm):
                x = F.layer_norm(x, (E,), d(layer.weight), d(layer.bias), layer.eps)
            else:
                x = torch.relu(x)
        if isinstance(m.output_proj, nn.Linear):
            x = F.linear(x, d(m.output_proj.weight), d(m.output_proj.bias))
        if self.residual is not None:
            x = x + d(self.residual).flatten(0, 1)
        return F.layer_norm(x, (E,), d(self.norm.weight), d(self.norm.bias), 1e-5).unflatten(0, (BS, G))


@functools.lru_cache(maxsize=None)
def block(family, duplicates):
    return Block(family, duplicates)


def _count_calls(modules):
    counts, handles = [0], []
    for mod in modules:
        handles.append(mod.register_forward_hook(lambda *a: counts.__setitem__(0, counts[0] + 1)))
    return counts, handles


@pytest.mark.parametrize("duplicates", ["sum", "last"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_native_tail_launches_and_accuracy(family, duplicates, spy):
    b = block(family, duplicates)
    dense = [l for l in b.m.modules() if isinstance(l, (nn.LayerNorm, nn.Linear, nn.ReLU))] + [b.norm]
    counts, handles = _count_calls(dense)
    del spy[:]
    native = b.call(True)
    assert spy == LAUNCHES[family]
    assert counts[0] == 0                                   # no torch layer ran, the passed norm included
    yard = b.call(False)
    assert counts[0] == len(dense)                          # native_tail = False: every one of them, once
    assert "gf_subm_conv_apply_epilogue" not in spy[len(LAUNCHES[family]):] and "gf_deform_output_forward" not in spy[len(LAUNCHES[family]):]
    for h in handles:
        h.remove()
    cells = b.m.voxel_indices(b.anchor).unique(dim=0).shape[0]
    assert 2.0 <= BS * G / cells <= 4.5                     # about three anchors share a cell
    truth = b.truth()
    assert native.shape == (BS, G, E)
    held(f"native tail {family} {duplicates}", native.cpu(), truth, bound(max_error(yard.cpu(), truth), truth))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_call_that_needs_autograd_is_the_torch_path(family, spy):
    b = block(family, "sum")
    m = b.m
    for p in list(m.parameters()) + list(b.norm.parameters()):
        p.grad = None
    x = b.x.clone().requires_grad_()
    del spy[:]
    out = m(x, b.anchor, residual=b.residual, norm=b.norm)
    assert "gf_subm_conv_apply_epilogue" not in spy and "gf_deform_output_forward" not in spy
    x2 = b.x.clone().requires_grad_()
    manual = m(x2, b.anchor)
    manual = b.norm(manual if b.residual is None else manual + b.residual)
    assert torch.equal(out.view(torch.int32), manual.view(torch.int32))
    out.square().mean().backward()
    convs = [l for l in m.modules() if isinstance(l, SubMConv3d)]
    for what, g in [("features", x.grad), *[("conv weight", c.weight.grad) for c in convs], ("norm weight", b.norm.weight.grad),
                    ("norm bias", b.norm.bias.grad)]:
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, what


def test_out_range_keeps_todays_behaviour():
    b = block("single_proj", "sum")
    m = b.m
    x, a = b.x[:1].contiguous(), b.anchor[:1].contiguous()
    with torch.no_grad():
        with pytest.raises(ValueError, match="out_range"):
            m(x, a, out_range=(10, 200), norm=b.norm)
        with pytest.raises(ValueError, match="out_range"):
            m(x, a, out_range=(10, 200), residual=x)
        part = m(x, a, out_range=(10, 200))
        # today's path: the torch projection on the range's rows of the plain convolution
        rb = m.last_rulebook
        want = m.output_proj(rb.apply(x[0], m.layer.weight)[10:200])[None]
        assert part.shape == (1, 190, E) and torch.equal(part.view(torch.int32), want.view(torch.int32))
