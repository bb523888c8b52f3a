"""A float64 restatement of mmcv's modulated_deform_conv2d (the contract of include/gf_hip.h), written from
the formula with explicit gathers.  The sample coordinate is rounded to fp32 exactly as the kernel rounds it (one fp32 add of
the exact integer base and the fp32 offset); everything after that is float64, so floor(y) agrees with the kernel and no entry
needs an exemption.  Its autograd is the truth for all five gradients.  Runs on CPU or, for the full-size checks, on the GPU.
"""
import torch
from torch.nn.modules.utils import _pair


def coords(offset, H, W, kh, kw, stride, padding, dilation, dg, fp32=True):
    """Sample coordinates ``y, x`` as float64 ``[N, dg, kh kw, Ho, Wo]``.  ``fp32=False`` adds in float64 (for gradcheck)."""
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    dh, dw = _pair(dilation)
    N, _, Ho, Wo = offset.shape
    kk = kh * kw
    dev = offset.device
    off = offset.reshape(N, dg, kk, 2, Ho, Wo)
    i = torch.arange(kh, device=dev).repeat_interleave(kw)
    j = torch.arange(kw, device=dev).repeat(kh)
    by = (torch.arange(Ho, device=dev)[None, :] * sh - ph + i[:, None] * dh)[:, :, None]   # [kk, Ho, 1]
    bx = (torch.arange(Wo, device=dev)[None, :] * sw - pw + j[:, None] * dw)[:, None, :]   # [kk, 1, Wo]
    dt = torch.float32 if fp32 else torch.float64
    y = (by.to(dt) + off[:, :, :, 0].to(dt)).to(torch.float64)
    x = (bx.to(dt) + off[:, :, :, 1].to(dt)).to(torch.float64)
    return y, x


def columns(input, offset, mask, kh, kw, stride=1, padding=0, dilation=1, deform_groups=1, fp32_coords=True):
    """The column tensor ``[N, Cin, kh kw, Ho, Wo]`` in float64 (differentiable in input, offset and mask)."""
    N, C, H, W = input.shape
    dg = deform_groups
    Cg = C // dg
    Ho, Wo = offset.shape[2:]
    kk = kh * kw
    y, x = coords(offset, H, W, kh, kw, stride, padding, dilation, dg, fp32_coords)
    inside = ((y > -1) & (x > -1) & (y < H) & (x < W)).to(torch.float64)
    h0 = torch.floor(y)
    w0 = torch.floor(x)
    lh, lw = y - h0, x - w0
    h0, w0 = h0.long(), w0.long()
    img = input.to(torch.float64).reshape(N, dg, Cg, H * W)
    val = 0
    for dy, dx, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        hh, ww = h0 + dy, w0 + dx
        ok = ((hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)).to(torch.float64)
        idx = (hh.clamp(0, H - 1) * W + ww.clamp(0, W - 1)).reshape(N, dg, 1, kk * Ho * Wo).expand(N, dg, Cg, kk * Ho * Wo)
        v = torch.gather(img, 3, idx).reshape(N, dg, Cg, kk, Ho, Wo)
        val = val + (wt * ok * inside)[:, :, None] * v
    m = mask.to(torch.float64).reshape(N, dg, 1, kk, Ho, Wo)
    return (val * m).reshape(N, C, kk, Ho, Wo)


def modulated_deform_conv2d(input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1,
                            deform_groups=1, fp32_coords=True):
    """float64 output ``[N, Cout, Ho, Wo]`` of mmcv's op (groups = 1)."""
    assert groups == 1
    Co, C, kh, kw = weight.shape
    col = columns(input, offset, mask, kh, kw, stride, padding, dilation, deform_groups, fp32_coords)
    out = torch.einsum("ock,nckhw->nohw", weight.to(torch.float64).reshape(Co, C, kh * kw), col)
    if bias is not None:
        out = out + bias.to(torch.float64)[None, :, None, None]
    return out


def abs_bound(input, offset, mask, weight, stride=1, padding=0, dilation=1, deform_groups=1):
    """``sum |w| |col|`` per output element: the scale of the forward's rounding bound."""
    Co, C, kh, kw = weight.shape
    with torch.no_grad():
        col = columns(input, offset, mask, kh, kw, stride, padding, dilation, deform_groups).abs()
        return torch.einsum("ock,nckhw->nohw", weight.to(torch.float64).abs().reshape(Co, C, kh * kw), col)
