"""CPU checks of the DCNv2 restatement (tests/dcn_ref.py) against operators outside it, and of the drop-in modules and the
refusals of gaussianformer_amd.deform_conv."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dcn_ref
from gaussianformer_amd import _lib
from gaussianformer_amd.deform_conv import (DCNv2, ModulatedDeformConv2d, ModulatedDeformConv2dPack,
                                            modulated_deform_conv2d)

# (kh, kw, stride, padding, dilation)
GEOMS = [(3, 3, 1, 1, 1), (1, 1, 1, 0, 1), (3, 5, (2, 1), (1, 2), 1), (3, 3, 2, 0, 2), (2, 3, 1, (2, 0), (1, 2))]


def _inputs(N, C, H, W, Co, kh, kw, stride, padding, dilation, dg=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    dh, dw = (dilation, dilation) if isinstance(dilation, int) else dilation
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, C, kh, kw, generator=g, dtype=torch.float64)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    return x, w, b, (N, 2 * dg * kh * kw, Ho, Wo), (N, dg * kh * kw, Ho, Wo)


@pytest.mark.parametrize("kh,kw,stride,padding,dilation", GEOMS)
def test_zero_offsets_equal_conv2d(kh, kw, stride, padding, dilation):
    x, w, b, os_, ms = _inputs(2, 3, 9, 11, 4, kh, kw, stride, padding, dilation)
    off, m = torch.zeros(os_, dtype=torch.float64), torch.ones(ms, dtype=torch.float64)
    got = dcn_ref.modulated_deform_conv2d(x, off, m, w, b, stride, padding, dilation)
    want = F.conv2d(x, w, b, stride, padding, dilation)
    assert torch.allclose(got, want, atol=1e-12, rtol=1e-12)
    half = dcn_ref.modulated_deform_conv2d(x, off, m * 0.5, w, None, stride, padding, dilation)
    assert torch.allclose(half, 0.5 * F.conv2d(x, w, None, stride, padding, dilation), atol=1e-12, rtol=1e-12)


@pytest.mark.parametrize("kh,kw,stride,padding,dilation", GEOMS)
def test_integer_offset_is_a_shift(kh, kw, stride, padding, dilation):
    # (dy, dx) = (1, -2) samples input[h + 1, w - 2]: conv2d of the shifted, zero-filled input.  A swapped y / x order or a
    # swapped kh / kw fails this.
    x, w, b, os_, ms = _inputs(2, 3, 9, 11, 4, kh, kw, stride, padding, dilation, seed=1)
    off = torch.zeros(os_, dtype=torch.float64).reshape(os_[0], -1, 2, *os_[2:])
    off[:, :, 0], off[:, :, 1] = 1.0, -2.0
    off = off.reshape(os_)
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    xp = F.pad(x, (pw, pw, ph, ph))          # the shift is taken on the padded canvas: padding stays zero
    shifted = torch.zeros_like(xp)
    shifted[:, :, :-1, 2:] = xp[:, :, 1:, :-2]
    got = dcn_ref.modulated_deform_conv2d(x, off, torch.ones(ms, dtype=torch.float64), w, b, stride, padding, dilation)
    assert torch.allclose(got, F.conv2d(shifted, w, b, stride, 0, dilation), atol=1e-12, rtol=1e-12)


@pytest.mark.parametrize("dg", [1, 2])
def test_fractional_offsets_equal_grid_sample(dg):
    N, C, H, W, kh, kw = 2, 4, 7, 8, 3, 3
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    off = (torch.randn(N, 2 * dg * kh * kw, H, W, generator=g) * 3).to(torch.float32)
    o = off.reshape(N, dg, kh * kw, 2, H, W)
    # edges: exactly -1, H - 1 + eps, fully outside, exactly on the last row
    o[:, :, 0, 0, 0, :] = -1.0          # tap (0, 0) at ho = 0: y = -2
    o[:, :, 4, 0, 0, :] = -1.0          # centre tap at ho = 0: y = -1 exactly
    o[:, :, 4, 0, H - 1, :] = 1e-3      # centre tap at the last row: y = H - 1 + eps
    o[:, :, 5, 1, :, 0] = -50.0         # fully outside
    o[:, :, 7, 0, 2, :] = float(H - 3)  # y = H exactly at ho = 2 (centre row + 1)
    m = torch.rand(N, dg * kh * kw, H, W, generator=g, dtype=torch.float64)
    col = dcn_ref.columns(x, off, m, kh, kw, 1, 1, 1, dg)
    y, xx = dcn_ref.coords(off, H, W, kh, kw, 1, 1, 1, dg)
    Cg = C // dg
    for grp in range(dg):
        for k in range(kh * kw):
            grid = torch.stack(((2 * xx[:, grp, k] + 1) / W - 1, (2 * y[:, grp, k] + 1) / H - 1), dim=-1)
            s = F.grid_sample(x[:, grp * Cg:(grp + 1) * Cg], grid, mode="bilinear", padding_mode="zeros", align_corners=False)
            want = s * m.reshape(N, dg, kh * kw, H, W)[:, grp, k][:, None]
            assert torch.allclose(col[:, grp * Cg:(grp + 1) * Cg, k], want, atol=1e-12), (grp, k)


def test_restatement_gradcheck():
    N, C, H, W, Co, kh, kw = 1, 2, 5, 6, 2, 3, 3
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    off = (torch.rand(N, 2 * kh * kw, H, W, generator=g, dtype=torch.float64) * 3 - 1.5).requires_grad_(True)
    m = torch.rand(N, kh * kw, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Co, C, kh, kw, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Co, generator=g, dtype=torch.float64, requires_grad=True)
    f = lambda *a: dcn_ref.modulated_deform_conv2d(*a, 1, 1, 1, 1, 1, fp32_coords=False)
    assert torch.autograd.gradcheck(f, (x, off, m, w, b), eps=1e-6, atol=1e-6)


def test_pack_state_dict_and_init():
    mod = ModulatedDeformConv2dPack(64, 32, 3, padding=1, bias=False)
    assert set(mod.state_dict()) == {"weight", "conv_offset.weight", "conv_offset.bias"}
    assert mod._version == 2 and DCNv2 is ModulatedDeformConv2dPack
    assert tuple(mod.conv_offset.weight.shape) == (27, 64, 3, 3)
    assert not mod.conv_offset.weight.any() and not mod.conv_offset.bias.any()
    assert mod.weight.abs().max() <= 1 / (64 * 9) ** 0.5
    mb = ModulatedDeformConv2dPack(64, 32, 3, padding=1)
    assert set(mb.state_dict()) == {"weight", "bias", "conv_offset.weight", "conv_offset.bias"} and not mb.bias.any()
    assert ModulatedDeformConv2d(64, 32, (3, 5), deformable_groups=2).deform_groups == 2
    assert ModulatedDeformConv2dPack(64, 32, 3, deformable_groups=2).conv_offset.out_channels == 2 * 27


def test_pack_loads_version1_offset_keys():
    def parent():
        p = nn.Module()
        p.conv2 = ModulatedDeformConv2dPack(32, 32, 3, padding=1, bias=False)
        return p
    src = parent()
    with torch.no_grad():
        src.conv2.conv_offset.weight.normal_()
        src.conv2.conv_offset.bias.normal_()
    sd = src.state_dict()
    old = type(sd)((k.replace("conv2.conv_offset.", "conv2_offset."), v) for k, v in sd.items())
    old._metadata = type(sd._metadata)((k, dict(v)) for k, v in sd._metadata.items())
    old._metadata["conv2"]["version"] = 1
    # mmcv's upgrade path renames `<prefix>_offset.*` in the dict its _load_from_state_dict receives (the whole dict, as
    # torch passed it to every module before 2.0; later torch hands a child only the keys under its own prefix)
    dst = parent()
    missing, unexpected, errors = [], [], []
    dst.conv2._load_from_state_dict(old, "conv2.", {"version": 1}, True, missing, unexpected, errors)
    assert not missing and not errors and "conv2_offset.weight" not in old
    assert torch.equal(old["conv2.conv_offset.weight"], src.conv2.conv_offset.weight)   # renamed for the child to load
    assert torch.equal(old["conv2.conv_offset.bias"], src.conv2.conv_offset.bias)
    assert torch.equal(dst.conv2.weight, src.conv2.weight)
    top = ModulatedDeformConv2dPack(32, 32, 3, padding=1, bias=False)   # a top-level module: loaded through load_state_dict
    flat = type(sd)((k[len("conv2."):].replace("conv_offset.", "_offset."), v) for k, v in sd.items())
    flat._metadata = type(sd._metadata)([("", {"version": 1})])
    top.load_state_dict(flat, strict=True)
    assert torch.equal(top.conv_offset.weight, src.conv2.conv_offset.weight)
    dst2 = parent()
    dst2.load_state_dict(src.state_dict(), strict=True)   # version 2: keys as they are
    assert torch.equal(dst2.conv2.conv_offset.weight, src.conv2.conv_offset.weight)


def _op_args(C=64, Co=32, dtype=torch.float32, dg=1):
    x = torch.zeros(1, C, 6, 6, dtype=dtype)
    return x, torch.zeros(1, 18 * dg, 6, 6, dtype=dtype), torch.zeros(1, 9 * dg, 6, 6, dtype=dtype), \
        torch.zeros(Co, C, 3, 3, dtype=dtype)


def test_refusals():
    x, o, m, w = _op_args()
    with pytest.raises(ValueError, match="groups"):
        modulated_deform_conv2d(x, o, m, w, None, 1, 1, 1, 2, 1)
    with pytest.raises(TypeError, match="fp32"):
        modulated_deform_conv2d(*_op_args(dtype=torch.float16), None, 1, 1, 1, 1, 1)
    with pytest.raises(ValueError, match="multiples of 32"):
        modulated_deform_conv2d(*_op_args(C=48), None, 1, 1, 1, 1, 1)
    with pytest.raises(ValueError, match="multiples of 32"):
        modulated_deform_conv2d(*_op_args(Co=40), None, 1, 1, 1, 1, 1)
    with pytest.raises(ValueError, match="multiples of 32"):
        modulated_deform_conv2d(*_op_args(C=64, dg=4), None, 1, 1, 1, 1, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        modulated_deform_conv2d(x, o, m, w, None, 1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ModulatedDeformConv2dPack(64, 32, 3, padding=1)(x)


def test_abi_refuses_before_any_hip_call():
    lib = _lib.load()
    geom = [1, 64, 6, 6, 32, 3, 3, 1, 1, 1, 1, 1, 1]
    assert lib.gf_dcn_workspace_bytes(*geom, 1, 1, 0) > 0
    assert lib.gf_dcn_workspace_bytes(*geom, 2, 1, 0) == 0
    rc = lib.gf_dcn_forward(*geom, 2, 1, *([None] * 6), None, 0, None)
    assert rc == -1 and b"groups" in lib.gf_last_error()
    rc = lib.gf_dcn_forward(1, 48, 6, 6, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, *([None] * 6), None, 0, None)
    assert rc == -1 and b"multiples of 32" in lib.gf_last_error()
    rc = lib.gf_dcn_backward(1, 64, 6, 6, 32, 9, 3, 1, 1, 1, 1, 1, 1, 1, 1, *([None] * 10), None, 0, None)
    assert rc == -1 and b"kernel" in lib.gf_last_error()
    rc = lib.gf_dcn_forward(*geom, 1, 1, *([None] * 6), None, 0, None)
    assert rc == -1   # null pointers, still before any HIP call
