"""Modulated deformable convolution (mmcv's DCNv2) as a HIP op (csrc/deform_conv.hip).

``modulated_deform_conv2d`` is mmcv's functional ``modulated_deform_conv2d`` with its positional order;
``ModulatedDeformConv2d`` and ``ModulatedDeformConv2dPack`` (alias ``DCNv2``) are drop-ins for mmcv's modules with their
constructors, parameter names, initialisation and state-dict upgrade path.  The reference builds its ResNet-101 backbone with
``dcn=dict(type='DCNv2', deform_groups=1, fallback_on_stride=False)`` and ``stage_with_dcn=(False, False, True, True)``.

Semantics (include/gf_hip.h has the full statement): for deform group ``g`` and tap ``k = i kw + j``, ``offset`` channel
``g 2 kh kw + 2 k`` is the row shift and ``+ 1`` the column shift, ``mask`` channel ``g kh kw + k`` the modulation; the sample
``y = (ho sh - ph + i dh) + dy`` (one fp32 add; likewise ``x``) is bilinear inside ``-1 < y < H, -1 < x < W`` (corners outside
the image add 0) and 0 outside; ``out = weight * (sample m) + bias``.

Supported: fp32 CUDA tensors, ``groups == 1``, kernel sides up to 7, ``Cin / deform_groups`` and ``Cout`` multiples of 32.
Anything else raises ``TypeError`` / ``ValueError`` before a kernel runs; CPU tensors raise ``RuntimeError`` (no CPU
fallback).  The op never synchronises the host, so it can be captured in a graph.  ``grad_input`` is summed with fp32 atomics
and is not bitwise reproducible; the output and the other gradients are.
"""
import math

import torch
import torch.nn as nn
from torch.nn.modules.utils import _pair

from . import _lib

GRANULE = _lib.GF_DCN_CHANNEL_GRANULE
MAX_KERNEL = _lib.GF_DCN_MAX_KERNEL


def _check(input, offset, mask, weight, bias, stride, padding, dilation, groups, deform_groups):
    tensors = (input, offset, mask, weight, bias)
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"modulated_deform_conv2d: fp32 tensors only, got {t.dtype}")
    if int(groups) != 1:
        raise ValueError(f"modulated_deform_conv2d: groups = {groups}; only groups = 1 is supported")
    if input.dim() != 4 or weight.dim() != 4:
        raise ValueError("modulated_deform_conv2d: input [N, Cin, H, W] and weight [Cout, Cin, kh, kw] expected")
    N, C, H, W = input.shape
    Co, Cw, kh, kw = weight.shape
    dg = int(deform_groups)
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    dh, dw = _pair(dilation)
    if Cw != C:
        raise ValueError(f"modulated_deform_conv2d: weight has {Cw} input channels, input {C}")
    if not (1 <= kh <= MAX_KERNEL and 1 <= kw <= MAX_KERNEL):
        raise ValueError(f"modulated_deform_conv2d: kernel {kh} x {kw}; each side in 1..{MAX_KERNEL}")
    if dg < 1 or C % dg:
        raise ValueError(f"modulated_deform_conv2d: deform_groups = {dg} must divide Cin = {C}")
    if (C // dg) % GRANULE or Co % GRANULE:
        raise ValueError(f"modulated_deform_conv2d: Cin / deform_groups = {C // dg} and Cout = {Co} must be multiples of {GRANULE}")
    if min(sh, sw, dh, dw) < 1 or min(ph, pw) < 0:
        raise ValueError("modulated_deform_conv2d: stride and dilation >= 1, padding >= 0 needed")
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    if H + 2 * ph < dh * (kh - 1) + 1 or W + 2 * pw < dw * (kw - 1) + 1:
        raise ValueError("modulated_deform_conv2d: the kernel does not fit the padded input")
    if tuple(offset.shape) != (N, 2 * dg * kh * kw, Ho, Wo):
        raise ValueError(f"modulated_deform_conv2d: offset must be {[N, 2 * dg * kh * kw, Ho, Wo]}, got {list(offset.shape)}")
    if tuple(mask.shape) != (N, dg * kh * kw, Ho, Wo):
        raise ValueError(f"modulated_deform_conv2d: mask must be {[N, dg * kh * kw, Ho, Wo]}, got {list(mask.shape)}")
    if bias is not None and tuple(bias.shape) != (Co,):
        raise ValueError(f"modulated_deform_conv2d: bias must be [{Co}], got {list(bias.shape)}")
    _lib.require_gpu(*tensors)
    return (N, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, 1, dg), (N, Co, Ho, Wo)


def _workspace(geom, backward, device):
    nbytes = _lib.load().gf_dcn_workspace_bytes(*geom, int(backward))
    if nbytes == 0:
        raise ValueError(f"gf_dcn_workspace_bytes refused {geom}: {_lib.load().gf_last_error().decode()}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


class _ModulatedDeformConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias, stride, padding, dilation, groups, deform_groups):
        geom, out_shape = _check(input, offset, mask, weight, bias, stride, padding, dilation, groups, deform_groups)
        x, off, m, w, b = (_lib.as_arg(t) for t in (input, offset, mask, weight, bias))   # (fp32 already: _check)
        out = torch.empty(out_shape, dtype=torch.float32, device=input.device)
        ws, nbytes = _workspace(geom, False, input.device)
        _lib.call("gf_dcn_forward", input.device, *geom, x, off, m, w, b, out, ws, nbytes)
        ctx.geom = geom
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, off, m, w)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, off, m, w = ctx.saved_tensors
        need = ctx.needs_input_grad
        go = _lib.as_arg(grad_out)
        gi = torch.empty_like(x) if need[0] else None
        goff = torch.empty_like(off) if need[1] else None
        gm = torch.empty_like(m) if need[2] else None
        gw = torch.empty_like(w) if need[3] else None
        gb = torch.empty(w.shape[0], dtype=torch.float32, device=x.device) if (ctx.has_bias and need[4]) else None
        if any(t is not None for t in (gi, goff, gm, gw, gb)):
            ws, nbytes = _workspace(ctx.geom, True, x.device)
            _lib.call("gf_dcn_backward", x.device, *ctx.geom, x, off, m, w, go, gi, goff, gm, gw, gb, ws, nbytes)
        return gi, goff, gm, gw, gb, None, None, None, None, None


def modulated_deform_conv2d(input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1,
                            deform_groups=1):
    """mmcv's ``modulated_deform_conv2d(input, offset, mask, weight, bias, stride, padding, dilation, groups,
    deform_groups)`` on the HIP kernels.  Saves its inputs (not columns) for the backward."""
    return _ModulatedDeformConv2d.apply(input, offset, mask, weight, bias, stride, padding, dilation, groups, deform_groups)


class ModulatedDeformConv2d(nn.Module):
    """mmcv's ``ModulatedDeformConv2d``: ``forward(x, offset, mask)``.  ``deformable_groups`` is the deprecated alias of
    ``deform_groups``."""

    _version = 2

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deform_groups=1,
                 bias=True, deformable_groups=None):
        super().__init__()
        if deformable_groups is not None:
            deform_groups = deformable_groups
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = _pair(stride)
        self.padding = _pair(padding)
        self.dilation = _pair(dilation)
        self.groups = groups
        self.deform_groups = deform_groups
        self.transposed = False
        self.output_padding = _pair(0)
        self.weight = nn.Parameter(torch.Tensor(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter("bias", None)
        self.init_weights()

    def init_weights(self):
        n = self.in_channels
        for k in self.kernel_size:
            n *= k
        stdv = 1.0 / math.sqrt(n)
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.zero_()

    def forward(self, x, offset, mask):
        return modulated_deform_conv2d(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                       self.groups, self.deform_groups)


class ModulatedDeformConv2dPack(ModulatedDeformConv2d):
    """mmcv's ``ModulatedDeformConv2dPack`` (registered as ``DCNv2``): the offsets and masks come from ``conv_offset``, a
    zero-initialised ``Conv2d`` with ``3 dg kh kw`` outputs -- ``o1, o2, m = chunk(., 3)``, ``offset = cat(o1, o2)``,
    ``mask = sigmoid(m)``."""

    _version = 2

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = nn.Conv2d(self.in_channels, self.deform_groups * 3 * self.kernel_size[0] * self.kernel_size[1],
                                     kernel_size=self.kernel_size, stride=self.stride, padding=self.padding,
                                     dilation=self.dilation, bias=True)
        self.init_weights()

    def init_weights(self):
        super().init_weights()
        if hasattr(self, "conv_offset"):
            self.conv_offset.weight.data.zero_()
            self.conv_offset.bias.data.zero_()

    def forward(self, x):
        out = self.conv_offset(x)
        o1, o2, mask = torch.chunk(out, 3, dim=1)
        offset = torch.cat((o1, o2), dim=1)
        mask = torch.sigmoid(mask)
        return modulated_deform_conv2d(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                       self.groups, self.deform_groups)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:
            # version < 2 (the original DCNv2 checkpoints) named conv_offset `<name>_offset`
            for k in ("weight", "bias"):
                new, old = prefix + "conv_offset." + k, prefix[:-1] + "_offset." + k
                if new not in state_dict and old in state_dict:
                    state_dict[new] = state_dict.pop(old)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


DCNv2 = ModulatedDeformConv2dPack
