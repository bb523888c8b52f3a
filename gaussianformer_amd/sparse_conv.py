"""Submanifold sparse 3-D convolution over the Gaussian centres.

Host mirror of ``SparseConv3D`` (model/encoder/gaussian_encoder/spconv3d_module.py:10-83), whose
``spconv.SubMConv3d`` has no ROCm build: the rulebook and the gather-GEMM run in
``gf_subm_rulebook_* / gf_subm_conv_apply / gf_subm_conv_weight_grad`` (include/gf_hip.h).  Without autograd the block's dense
tail -- bias, LayerNorm, ReLU, ``output_proj``, the encoder's ``"add"`` / ``"norm"`` -- runs inside the convolutions' last pass
(``gf_subm_conv_apply_epilogue``) and one ``gf_deform_output_forward`` launch.  With autograd, a stage
``relu?(LN((conv + bias) + residual))`` has a native training step (``subm_stage`` / ``subm_stages``, ``SubMStageFunction``,
the block's opt-in ``native_training``).
"""
import math

import ctypes
import os

import torch
import torch.nn as nn
from torch.autograd.function import Function, once_differentiable

from . import _lib

f32, i32 = torch.float32, torch.int32
E_NATIVE = 128   # the width at which the block's dense tail has a native form (gf_deform_output_forward)


class Rulebook:
    """Neighbour pairs of one point set (reusable across layers and by the backward pass).

    ``pair_capacity=None``: the pair count is read back once to size the pair arrays (spconv reads its pair counts
    the same way).  ``pair_capacity=n``: nothing is read back -- the arrays hold ``n`` pairs, a point set with more
    pairs produces an empty rulebook (NaN output: a refused point set must not look like a healthy zero) and a
    refusal flag that :meth:`check` raises on; call it at a point where the stream is synchronised anyway, or use
    :meth:`poll` (non-blocking: the status is copied to pinned host memory behind the build and read once that copy
    has completed).  Note the memory side of a generous capacity: ``apply`` sizes its partial-row buffer
    ``[pair_capacity, Cout]`` by it (32 KB per point at ``pairs_per_point=64``, Cout = 128)."""

    def __init__(self, indices, batch_size, spatial_shape, kernel_size, pair_capacity=None, out_range=None):
        """``out_range=(lo, hi)``: pairs only for the output points ``[lo, hi)`` (every point stays a neighbour) -- the rows an
        anchor-sharded rank owns, at ``(hi - lo) / N`` of the gather-GEMM work; the other rows of ``apply`` are zeros."""
        _lib.require_gpu(indices)
        lib = _lib.load()
        self.indices = _lib.as_arg(indices, i32)
        self.N = self.indices.shape[0]
        self.out_range = None if out_range is None else (int(out_range[0]), int(out_range[1]))
        rng = () if self.out_range is None else self.out_range
        suffix = "" if self.out_range is None else "_range"   # (the entry points used, so an error names the right one)
        self.dims = (self.N, int(batch_size), int(spatial_shape[0]), int(spatial_shape[1]), int(spatial_shape[2]),
                     int(kernel_size))
        dev = self.indices.device
        nbytes = lib.gf_subm_tables_bytes(*self.dims)
        if nbytes == 0:
            raise RuntimeError(f"unsupported sparse-conv geometry {self.dims}")
        self.tables = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._status = self.tables[nbytes - 256:nbytes - 240].view(torch.int64)   # (pair count, refusal bits)
        self.checked = pair_capacity is None
        if pair_capacity is not None:
            self.total = max(int(pair_capacity), 1)
            self.pair_in = torch.empty(self.total, dtype=i32, device=dev)
            self.pair_out = torch.empty(self.total, dtype=i32, device=dev)
            _lib.call("gf_subm_rulebook_build" + suffix, dev, *self.dims, *rng, self.indices, self.tables, nbytes,
                      self.pair_in, self.pair_out, self.total)
            # deferred check: status -> pinned host memory on the same stream, event behind the copy
            # (not while a HIP graph is being captured: no host allocation there; check() still works after a replay)
            self._host_status, self._status_event = _lib.host_copy(self._status, dev)
            return
        _lib.call("gf_subm_rulebook_count" + suffix, dev, *self.dims, *rng, self.indices, self.tables, nbytes)
        total = self.check()   # the one host read
        self.total = int(total)
        self.pair_in = torch.empty(max(self.total, 1), dtype=i32, device=dev)
        self.pair_out = torch.empty(max(self.total, 1), dtype=i32, device=dev)
        _lib.call("gf_subm_rulebook_fill" + suffix, dev, *self.dims, *rng, self.indices, self.tables, self.pair_in, self.pair_out)

    def representative_mask(self):
        """``[N,1]`` fp32, 1 for the point with the LARGEST index of its cell (and for points outside the grid), 0 for the
        others: the ``duplicates="last"`` mode of :func:`subm_conv3d` (cached)."""
        if getattr(self, "_rep_mask", None) is None:
            N, B, X, Y, Z, _ = self.dims
            idx = self.indices.long()
            b, x, y, z = idx.unbind(1)
            valid = (b >= 0) & (b < B) & (x >= 0) & (x < X) & (y >= 0) & (y < Y) & (z >= 0) & (z < Z)
            key = (((b * X + x) * Y + y) * Z + z).clamp(min=0, max=B * X * Y * Z - 1)
            me = torch.arange(N, device=idx.device)
            last = torch.full((B * X * Y * Z,), -1, dtype=torch.long, device=idx.device)
            last.scatter_reduce_(0, key[valid], me[valid], reduce="amax")
            self._rep_mask = ((last[key] == me) | ~valid).to(f32)[:, None]
        return self._rep_mask

    def sources(self, features, duplicates):
        """``features`` as a convolution reads them: with ``duplicates="last"`` only a cell's representative row is a source."""
        return features * self.representative_mask() if duplicates == "last" else features

    def check(self):
        """Reads the device status (synchronises): returns the pair count, raises if the point set was refused."""
        total, refused = self._status.tolist()
        self.checked = True
        self.pair_count = int(total)
        if refused:
            self._raise(total, refused)
        return total

    def poll(self):
        """Non-blocking :meth:`check` of a ``pair_capacity`` rulebook: ``None`` while the status copy is still in
        flight, else the pair count (the device's count, the same number :meth:`check` returns -- not the capacity the
        arrays were sized with) -- raising like :meth:`check` if the point set was refused."""
        if self.checked:
            return self.pair_count
        if self._status_event is None or not self._status_event.query():
            return None
        total, refused = self._host_status.tolist()
        self.checked = True
        self.pair_count = int(total)
        if refused:
            self._raise(total, refused)
        return total

    def _raise(self, total, refused):
        raise RuntimeError("sparse-conv rulebook refused: " +
                           ("a cell holds more than 65535 points" if refused & 1 else
                            "more than 2^31 - 1 neighbour pairs" if refused & 2 else
                            f"{total} neighbour pairs exceed the pair_capacity of {self.total}"))

    def apply(self, features, weight, bias=None, residual=None, norm=None, relu=False):
        """``out[N, Cout]`` for ``features [N, Cin]`` and ``weight [K^3, Cin, Cout]`` (no autograd).

        With any of the further arguments the convolution's last pass finishes the row before it stores it
        (``gf_subm_conv_apply_epilogue``): ``out = relu?(norm?((conv + bias) + residual))``, ``bias [Cout]``, ``residual [N, Cout]``,
        ``norm`` an affine ``nn.LayerNorm(Cout)`` with eps 1e-5 or a ``(weight, bias)`` pair.  Without them it is the plain call."""
        lib = _lib.load()
        features, weight = _lib.as_arg(features), _lib.as_arg(weight)
        cin, cout = weight.shape[1], weight.shape[2]
        dev = features.device
        epilogue = bias is not None or residual is not None or norm is not None or relu
        if epilogue:
            gamma, beta = _lib.norm_pair(norm, "Rulebook.apply")
            _lib.require_gpu(bias, residual, gamma, beta)
            for name, t, shape in (("bias", bias, (cout,)), ("residual", residual, (self.N, cout)), ("norm weight", gamma, (cout,)),
                                   ("norm bias", beta, (cout,))):
                if t is not None and tuple(t.shape) != shape:
                    raise ValueError(f"Rulebook.apply: {name} {tuple(t.shape)} is not {shape}")
            bias, residual, gamma, beta = (_lib.aligned(t) for t in (bias, residual, gamma, beta))
        out = torch.empty(self.N, cout, dtype=f32, device=dev)
        partial = torch.empty(max(self.total, 1), cout, dtype=f32, device=dev)
        # (the rows as two f16 terms under a power-of-two scale per row, split once per call: gf_subm_conv_apply_scratch)
        nscratch = int(lib.gf_subm_apply_scratch_bytes(self.N, cin))
        scratch = torch.empty(max(nscratch, 16), dtype=torch.uint8, device=dev)
        if epilogue:
            _lib.call("gf_subm_conv_apply_epilogue", dev, *self.dims, cin, cout, self.total, features, weight, self.tables,
                      self.pair_in, partial, out, scratch, nscratch, bias, residual, gamma, beta, int(bool(relu)))
            return out
        _lib.call("gf_subm_conv_apply_scratch", dev, *self.dims, cin, cout, self.total, features, weight, self.tables,
                  self.pair_in, partial, out, scratch, nscratch)
        return out

    def stage(self, features, weight, bias=None, residual=None, norm=None, relu=False):
        """The differentiable stage ``relu?(norm((conv + bias) + residual))`` with a native training step: :func:`subm_stage`."""
        return subm_stage(features, self, weight, bias=bias, residual=residual, norm=norm, relu=relu)

    def _scratch(self, cin, cout, dev):
        """``(partial, scratch, nscratch)`` of one convolution call."""
        nscratch = int(_lib.load().gf_subm_apply_scratch_bytes(self.N, cin))
        return (torch.empty(max(self.total, 1), cout, dtype=f32, device=dev),
                torch.empty(max(nscratch, 16), dtype=torch.uint8, device=dev), nscratch)

    def stage_forward(self, features, weight, bias, residual, gamma, beta, relu):
        """``(out, pre)`` of the saving forward (``gf_subm_conv_apply_epilogue_train``); the arguments as the library reads them."""
        cin, cout = weight.shape[1], weight.shape[2]
        dev = features.device
        out = torch.empty(self.N, cout, dtype=f32, device=dev)
        pre = torch.empty(self.N, cout, dtype=f32, device=dev)
        partial, scratch, nscratch = self._scratch(cin, cout, dev)
        _lib.call("gf_subm_conv_apply_epilogue_train", dev, *self.dims, cin, cout, self.total, features, weight, self.tables,
                  self.pair_in, partial, out, scratch, nscratch, bias, residual, gamma, beta, int(bool(relu)), pre)
        return out, pre

    def stage_backward(self, pre, gamma, beta, relu, want_bias, grad_out=None, grad_next=None, weight_t=None):
        """``(g_pre, g_gamma, g_beta, g_bias | None)`` of a stage.  With ``grad_out`` the standalone form
        (``gf_subm_stage_backward``); with ``grad_next`` / ``weight_t`` -- the next stage's ``g_pre`` and its mirrored, transposed
        weight -- the form inside that stage's data-gradient convolution (``gf_subm_conv_apply_stage_backward``): the same bits."""
        cout = pre.shape[1]
        dev = pre.device
        g_pre = torch.empty_like(pre)
        g_gamma, g_beta = torch.empty(cout, dtype=f32, device=dev), torch.empty(cout, dtype=f32, device=dev)
        g_bias = torch.empty(cout, dtype=f32, device=dev) if want_bias else None
        nwork = _lib.train_sizes("gf_subm_stage_train_sizes", self.N, cout)[1]
        work = torch.empty(max(nwork, 16), dtype=torch.uint8, device=dev)
        if grad_out is not None:
            _lib.call("gf_subm_stage_backward", dev, self.N, cout, pre, _lib.aligned(grad_out), gamma, beta, int(bool(relu)), g_pre,
                      g_gamma, g_beta, g_bias, work, nwork)
        else:
            cin = weight_t.shape[1]
            partial, scratch, nscratch = self._scratch(cin, cout, dev)
            _lib.call("gf_subm_conv_apply_stage_backward", dev, *self.dims, cin, cout, self.total, grad_next, weight_t, self.tables,
                      self.pair_in, partial, scratch, nscratch, pre, gamma, beta, int(bool(relu)), g_pre, g_gamma, g_beta, g_bias,
                      work, nwork)
        return g_pre, g_gamma, g_beta, g_bias

    def weight_grad(self, features, grad_out):
        features, grad_out = _lib.as_arg(features), _lib.as_arg(grad_out)
        cin, cout = features.shape[1], grad_out.shape[1]
        k3 = self.dims[5] ** 3
        gw = torch.empty(k3, cin, cout, dtype=f32, device=features.device)
        _lib.call("gf_subm_conv_weight_grad", features.device, *self.dims, cin, cout, self.total, features, grad_out,
                  self.tables, self.pair_in, self.pair_out, gw)
        return gw


class _SubMConv(Function):
    @staticmethod
    def forward(ctx, features, weight, rulebook):
        ctx.rulebook = rulebook
        ctx.save_for_backward(features, weight)
        return rulebook.apply(features, weight)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        features, weight = ctx.saved_tensors
        rb = ctx.rulebook
        g_feat = g_w = None
        if ctx.needs_input_grad[0]:
            # the neighbour relation is symmetric: same rulebook, kernel mirrored and transposed
            g_feat = rb.apply(grad_out, weight.flip(0).transpose(1, 2))
        if ctx.needs_input_grad[1]:
            g_w = rb.weight_grad(features, grad_out)
        return g_feat, g_w, None


STAGE_CHANNELS = (32, 64, 128)   # the widths the stage's training entries take (the epilogue's)


class SubMStageFunction(Function):
    """``S >= 1`` chained stages ``x <- relu?(LN((conv(x) + bias) + residual))`` on one rulebook with a native training step
    (DESIGN.md §3.7c).  Forward: ``gf_subm_conv_apply_epilogue_train`` per stage; saved are each stage's input, weight, ``pre`` and
    LayerNorm pair.  Backward, last stage first: the last stage's ``g_pre`` by ``gf_subm_stage_backward`` on ``grad_out``, every
    earlier one's inside the data-gradient convolution of the stage behind it (``gf_subm_conv_apply_stage_backward``: ``dL/dy`` of
    a stage in between never reaches memory), each followed by ``weight_grad(input, g_pre)``; the first stage's data gradient is
    the plain convolution.  Arguments: ``rulebook, relus, features``, then per stage ``weight, bias | None, residual | None,
    ln_weight, ln_bias``."""

    @staticmethod
    def forward(ctx, rulebook, relus, features, *flat):
        x = _lib.as_arg(features)
        saved, has = [], []
        for s, relu in enumerate(relus):
            weight, bias, residual, gamma, beta = flat[5 * s:5 * s + 5]
            weight = _lib.as_arg(weight)
            bias, residual, gamma, beta = (_lib.aligned(t) for t in (bias, residual, gamma, beta))
            out, pre = rulebook.stage_forward(x, weight, bias, residual, gamma, beta, relu)
            saved += [x, weight, gamma, beta, pre]
            has.append((bias is not None, residual is not None))
            x = out
        ctx.rulebook, ctx.relus, ctx.has = rulebook, tuple(relus), has
        ctx.save_for_backward(*saved)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        rb, saved, S = ctx.rulebook, ctx.saved_tensors, len(ctx.relus)
        need = ctx.needs_input_grad
        grads = [None] * (3 + 5 * S)
        g_pre = weight_t = None
        for s in reversed(range(S)):
            x, weight, gamma, beta, pre = saved[5 * s:5 * s + 5]
            has_bias, has_residual = ctx.has[s]
            if s == S - 1:
                g_pre, g_gamma, g_beta, g_bias = rb.stage_backward(pre, gamma, beta, ctx.relus[s], has_bias, grad_out=grad_out)
            else:
                g_pre, g_gamma, g_beta, g_bias = rb.stage_backward(pre, gamma, beta, ctx.relus[s], has_bias, grad_next=g_pre,
                                                                   weight_t=weight_t)
            # the neighbour relation is symmetric: same rulebook, kernel mirrored and transposed
            weight_t = weight.flip(0).transpose(1, 2).contiguous() if s > 0 or need[2] else None
            at = 3 + 5 * s
            if need[at]:
                grads[at] = rb.weight_grad(x, g_pre)
            if has_bias and need[at + 1]:
                grads[at + 1] = g_bias
            if has_residual and need[at + 2]:
                grads[at + 2] = g_pre
            grads[at + 3], grads[at + 4] = (g_gamma if need[at + 3] else None), (g_beta if need[at + 4] else None)
        if need[2]:
            grads[2] = rb.apply(g_pre, weight_t)
        return tuple(grads)


def subm_stages(features, rulebook, stages):
    """``stages``: a list of ``dict(weight=, bias=None, residual=None, norm=, relu=False)``, applied in their order to ``features``
    on one rulebook as ONE :class:`SubMStageFunction` (``duplicates="sum"`` semantics: every point is a source).  ``norm`` is
    required: a stage without a LayerNorm has no native training step."""
    if rulebook.out_range is not None:
        raise RuntimeError("a Rulebook with out_range is inference-only")
    for st in stages:
        if st.get("norm") is None:
            raise ValueError("subm_stage: norm is required (an affine LayerNorm with eps = 1e-5, or a (weight, bias) pair)")
        _lib.norm_pair(st["norm"], "subm_stage")
    _lib.require_gpu(features)
    flat, relus, cin = [], [], features.shape[-1]
    for st in stages:
        weight, bias, residual = st["weight"], st.get("bias"), st.get("residual")
        gamma, beta = _lib.norm_pair(st["norm"], "subm_stage")
        _lib.require_gpu(weight, bias, residual, gamma, beta)
        cout = weight.shape[2]
        if weight.shape[1] != cin or cin not in STAGE_CHANNELS or cout not in STAGE_CHANNELS:
            raise ValueError(f"subm_stage: weight {tuple(weight.shape)} on {cin} input channels; channels must be in {STAGE_CHANNELS}")
        for name, t, shape in (("bias", bias, (cout,)), ("residual", residual, (rulebook.N, cout)), ("norm weight", gamma, (cout,)),
                               ("norm bias", beta, (cout,))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f"subm_stage: {name} {tuple(t.shape)} is not {shape}")
        flat += [weight, bias, residual, gamma, beta]
        relus.append(bool(st.get("relu", False)))
        cin = cout
    return SubMStageFunction.apply(rulebook, tuple(relus), features, *flat)


def subm_stage(features, rulebook, weight, bias=None, residual=None, norm=None, relu=False):
    """The differentiable stage ``relu?(norm((conv(features) + bias) + residual))`` on ``rulebook`` (:meth:`Rulebook.apply`'s
    arguments; ``norm`` required) with a native forward and backward.  A chain of stages whose data gradients run inside one
    another's backward is :func:`subm_stages`; calls of this function chain too, unfused, to the same bits."""
    return subm_stages(features, rulebook, [dict(weight=weight, bias=bias, residual=residual, norm=norm, relu=relu)])


DUPLICATES = ("sum", "last")


def subm_conv3d(features, indices, weight, batch_size, spatial_shape, kernel_size, rulebook=None, duplicates="sum"):
    """Functional submanifold convolution; ``indices`` int ``[N,4]`` = (batch, x, y, z),
    ``weight [K^3, Cin, Cout]`` (offsets in [K,K,K] order).  Returns ``[N, Cout]``.

    ``duplicates`` says what several points in ONE cell mean.  ``"sum"`` (default): all of them are sources and each
    receives the cell's output -- the dense convolution of the scattered-and-summed features.  ``"last"``: only the point
    with the largest index of a cell is a source for its neighbours (every point still receives an output), which is one
    of the outcomes of spconv's hash insert, where the duplicate that ends up in the table is a race
    (spconv3d_module.py:73-77 hands the duplicates to ``spconv.SparseConvTensor`` as they are); the others get no
    gradient.  It is the same operator on features whose non-representative rows are zeroed."""
    if duplicates not in DUPLICATES:
        raise ValueError(f"duplicates must be one of {DUPLICATES}")
    rb = rulebook if rulebook is not None else Rulebook(indices, batch_size, spatial_shape, kernel_size)
    if rb.out_range is not None and torch.is_grad_enabled() and (features.requires_grad or weight.requires_grad):
        # (the backward relies on the neighbour relation being symmetric: a rulebook restricted to a range of output points is not)
        raise RuntimeError("a Rulebook with out_range is inference-only")
    return _SubMConv.apply(rb.sources(features, duplicates), weight, rb)


class SubMConv3d(nn.Module):
    """``spconv.SubMConv3d(in_channels, out_channels, kernel_size, stride=1, padding=k//2, bias=...)``
    as used by the reference (spconv3d_module.py:28-44); weight ``[K^3, Cin, Cout]``."""

    def __init__(self, in_channels, out_channels, kernel_size=5, bias=True, duplicates="sum"):
        super().__init__()
        if duplicates not in DUPLICATES:
            raise ValueError(f"duplicates must be one of {DUPLICATES}")
        self.duplicates = duplicates
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.weight = nn.Parameter(torch.empty(kernel_size ** 3, in_channels, out_channels))
        nn.init.kaiming_uniform_(self.weight.view(-1, out_channels), a=math.sqrt(5))
        if bias:
            bound = 1.0 / math.sqrt(in_channels * kernel_size ** 3)
            self.bias = nn.Parameter(torch.empty(out_channels).uniform_(-bound, bound))
        else:
            self.register_parameter("bias", None)

    def forward(self, features, indices, batch_size, spatial_shape, rulebook=None):
        out = subm_conv3d(features, indices, self.weight, batch_size, spatial_shape, self.kernel_size, rulebook,
                          duplicates=self.duplicates)
        return out if self.bias is None else out + self.bias


class SparseConv3D(nn.Module):
    """Drop-in for the reference's ``SparseConv3D`` block (spconv3d_module.py:10-83): voxelise the
    anchor centres, submanifold conv (one bias-free layer, or with ``use_multi_layer`` three
    conv + LayerNorm + ReLU stages, :26-37), output projection.  The three stages share one
    rulebook -- a submanifold convolution keeps the active set."""

    native_tail = True
    native_training = False   # opt-in: a call that needs autograd runs its LayerNorm stages' native training step (§3.7c)
    native_tail_training = False   # opt-in, with native_training: output_proj and the add / norm behind it as one native training step (§3.13f)

    def __init__(self, in_channels, embed_channels, pc_range, grid_size, xyz_activation="sigmoid", use_out_proj=False,
                 kernel_size=5, use_multi_layer=False, pairs_per_point=None, duplicates="sum", **kwargs):
        super().__init__()
        self.embed_channels = embed_channels
        # extra keyword ``duplicates`` ("sum" | "last"): what several anchors in one cell mean, see subm_conv3d
        # extra keyword: with ``pairs_per_point=n`` the rulebook is built for at most n * points neighbour pairs without
        # reading the pair count back (no host synchronisation in the encoder loop); ``self.last_rulebook.check()``
        # reports a point set that did not fit.  None = exact size, one host read per rulebook (like spconv).
        self.pairs_per_point = pairs_per_point
        self.last_rulebook = None
        self._unchecked = []   # pair_capacity rulebooks whose status has not been seen yet (polled, never waited for)
        if use_multi_layer:
            self.layer = nn.ModuleList()
            for i in range(3):
                self.layer.append(SubMConv3d(in_channels if i == 0 else embed_channels, embed_channels, kernel_size,
                                             duplicates=duplicates))
                self.layer.append(nn.LayerNorm(embed_channels))
                self.layer.append(nn.ReLU(True))
        else:
            self.layer = SubMConv3d(in_channels, embed_channels, kernel_size, bias=False, duplicates=duplicates)
        self.kernel_size = kernel_size
        self.output_proj = nn.Linear(embed_channels, embed_channels) if use_out_proj else nn.Identity()
        self.use_sigmoid = xyz_activation == "sigmoid"
        self._range = [float(v) for v in pc_range]
        self.register_buffer('pc_range', torch.tensor(pc_range, dtype=torch.float))
        self.register_buffer('grid_size', torch.tensor(grid_size, dtype=torch.float))
        # spatial_shape = ((pc_range[3:] - pc_range[:3]) / grid_size).to(int32), evaluated once in fp32 like the reference (:70-71)
        self._spatial = ((self.pc_range[3:] - self.pc_range[:3]) / self.grid_size).to(torch.int32).tolist()

    def voxel_indices(self, anchor):
        """int32 ``[b*g, 4]`` (batch, x, y, z) of the anchor centres (spconv3d_module.py:56-66,
        ``cartesian`` model/encoder/gaussian_encoder/utils.py:26-36, ``safe_sigmoid`` model/utils/safe_ops.py:7-9)."""
        bs, g = anchor.shape[:2]
        # (integer indices: nothing to differentiate either way)
        if anchor.is_cuda and anchor.dtype == torch.float32 and anchor.shape[-1] >= 3 and os.environ.get("GF_SUBM_TORCH_VOXELIZE") is None:
            return self._voxel_indices_native(anchor)
        return self._voxel_indices_torch(anchor)

    def _voxel_indices_native(self, anchor):
        """One launch (``gf_subm_voxelize``) instead of the dozen elementwise ops of ``_voxel_indices_torch``: the same fp32
        operations in the same order, so the same indices (``tests/test_subm_conv.py``)."""
        import numpy as np
        bs, g = anchor.shape[:2]
        a2 = anchor.detach().reshape(bs * g, anchor.shape[-1])
        if not a2.is_contiguous():
            a2 = a2.contiguous()
        key = (self.pc_range.data_ptr(), self.pc_range._version, self.grid_size.data_ptr(), self.grid_size._version)
        host = getattr(self, "_voxel_host", None)
        if host is None or host[0] != key:   # (buffers can be reloaded: one host read per change)
            r = self._range
            pc, gs = self.pc_range.detach().cpu().numpy().astype(np.float32), self.grid_size.detach().cpu().numpy().astype(np.float32)
            arr = lambda v: (ctypes.c_float * 3)(*[float(np.float32(x)) for x in v])
            host = self._voxel_host = (key, arr([r[3 + a] - r[a] for a in range(3)]), arr([r[a] for a in range(3)]), arr(pc[:3]), arr(gs[:3]))
        out = torch.empty((bs * g, 4), dtype=torch.int32, device=anchor.device)
        _lib.call("gf_subm_voxelize", anchor.device, bs * g, g, a2.shape[1], int(self.use_sigmoid), a2, *host[1:], out)
        return out

    def _voxel_indices_torch(self, anchor):
        bs, g = anchor.shape[:2]
        xyz = anchor[..., :3]
        xyz = xyz.clamp(-9.21, 9.21).sigmoid() if self.use_sigmoid else xyz.clamp(min=1e-6, max=1 - 1e-6)
        r = self._range
        xyz = torch.stack([xyz[..., a] * (r[3 + a] - r[a]) + r[a] for a in range(3)], dim=-1).flatten(0, 1)
        idx = ((xyz - self.pc_range[None, :3]) / self.grid_size[None, :]).to(torch.int32)
        bidx = torch.arange(bs, device=idx.device, dtype=torch.int32).repeat_interleave(g)[:, None]
        return torch.cat([bidx, idx], dim=-1)

    def forward(self, instance_feature, anchor, out_range=None, residual=None, norm=None):
        """``residual=`` / ``norm=`` (extra keywords, as on the deformable block): the encoder's ``"add"`` / ``"norm"`` behind the
        block, ``norm(block(instance_feature, anchor) + residual)`` with ``residual [b, g, C]`` and ``norm`` an ``nn.LayerNorm`` or a
        ``(weight, bias)`` pair.  With ``native_tail`` (a class attribute, not a constructor key and not part of the
        ``state_dict``), nothing that needs autograd, fp32 GPU tensors and ``embed_channels == 128`` they, the stages' bias,
        LayerNorm and ReLU and ``output_proj`` run inside the convolutions' last pass and one ``gf_deform_output_forward`` launch;
        every other call runs the torch layers, the two keywords as torch ops behind them.  With ``native_training`` (likewise a
        class attribute, off by default) a call that DOES need autograd runs every stage that has a LayerNorm -- a multi-layer
        block's three, a single-layer block's ``norm(conv + residual)`` where ``output_proj`` is the identity -- as a
        ``SubMStageFunction`` (fp32 GPU tensors, widths 32 / 64 / 128); ``output_proj`` and what follows it stay torch ops
        unless ``native_tail_training`` (a third class attribute, off by default, effective with ``native_training`` only) is
        set as well: then an ``output_proj`` that is a Linear with bias at ``embed_channels == 128``, with the ``residual=`` /
        ``norm=`` behind it, runs as ``deformable_output_autograd`` -- so a single-layer block with such an
        ``output_proj`` qualifies too: its convolution Function with the bias, then that tail.

        ``out_range=(lo, hi)`` (extra keyword, inference, batch size 1, single-layer blocks): ``instance_feature`` / ``anchor``
        are the WHOLE (all-gathered) anchor set, the block is evaluated for the anchors ``[lo, hi)`` only and returns
        ``[1, hi - lo, C]`` -- the rows an anchor-sharded rank owns, bit-identical to the same rows of the whole block, at
        ``(hi - lo) / g`` of the gather-GEMM and projection work."""
        if out_range is not None and (residual is not None or norm is not None):
            raise ValueError("SparseConv3D: out_range= does not take residual= / norm= (the sharded frame applies them to its own rows)")
        bs, g, _ = instance_feature.shape
        indices = self.voxel_indices(anchor)
        feats = instance_feature.flatten(0, 1)
        # refusals of earlier calls surface here, without blocking: a refused rulebook already produced NaN features,
        # this names the cause as soon as its status has reached the host.  (Both paths below: the list keeps at most the
        # eight youngest rulebooks whose status is still in flight, so a long inference loop holds a bounded set of tables.)
        if self._unchecked and not torch.cuda.is_current_stream_capturing():
            still = []
            for old in self._unchecked:
                if old.poll() is None:
                    still.append(old)
            self._unchecked = still[-8:]
        if out_range is not None:
            if bs != 1 or not isinstance(self.layer, SubMConv3d):
                raise RuntimeError("out_range needs batch size 1 and a single-layer block")
            lo, hi = int(out_range[0]), int(out_range[1])
            cap = None if self.pairs_per_point is None else int(self.pairs_per_point) * max(hi - lo, 1)
            rb = self.last_rulebook = Rulebook(indices, bs, self._spatial, self.kernel_size, pair_capacity=cap, out_range=(lo, hi))
            if cap is not None and not rb.checked and rb._status_event is not None:
                self._unchecked.append(rb)
            out = self.layer(feats, indices, bs, self._spatial, rulebook=rb)
            return self.output_proj(out[lo:hi])[None]
        cap = None if self.pairs_per_point is None else int(self.pairs_per_point) * indices.shape[0]
        rb = self.last_rulebook = Rulebook(indices, bs, self._spatial, self.kernel_size, pair_capacity=cap)
        if cap is not None and not rb.checked and rb._status_event is not None:
            self._unchecked.append(rb)
        if self._native_tail(instance_feature, anchor, residual, norm):
            return self._forward_native_tail(feats, rb, residual, norm).unflatten(0, (bs, g))
        if self._native_training(instance_feature, anchor, residual, norm):
            return self._forward_native_training(feats, rb, residual, norm, bs, g)
        if isinstance(self.layer, SubMConv3d):
            out = self.layer(feats, indices, bs, self._spatial, rulebook=rb)
        else:
            out = feats
            for m in self.layer:
                out = m(out, indices, bs, self._spatial, rulebook=rb) if isinstance(m, SubMConv3d) else m(out)
        out = self.output_proj(out.unflatten(0, (bs, g)))
        if residual is not None:
            out = out + residual
        if norm is not None:
            out = _lib.apply_norm(out, norm)
        return out

    def _native_tail(self, instance_feature, anchor, residual, norm):
        """Whether this call's dense tail runs natively: the checks ``Rulebook.apply`` and ``deformable_output`` make, asked first."""
        if not self.native_tail or self.embed_channels != E_NATIVE or not _lib.norm_native(norm):
            return False
        if not isinstance(self.output_proj, (nn.Linear, nn.Identity)):
            return False
        if isinstance(self.output_proj, nn.Linear) and self.output_proj.bias is None:
            return False
        if not isinstance(self.layer, SubMConv3d) and self._stage_modules() is None:
            return False
        tensors = [instance_feature, anchor, residual, *self.parameters(), *_lib.norm_tensors(norm)]
        return _lib.native_tensors(tensors) and not _lib.needs_grad(tensors)

    def _stage_modules(self):
        """``[(conv, ln)]`` of a multi-layer block built as conv + LayerNorm + ReLU three times, else ``None``."""
        if isinstance(self.layer, SubMConv3d):
            return None
        stages = list(self.layer)
        if len(stages) != 9:
            return None
        for conv, ln, act in zip(stages[0::3], stages[1::3], stages[2::3]):
            if not (isinstance(conv, SubMConv3d) and isinstance(ln, nn.LayerNorm) and _lib.norm_native(ln) and isinstance(act, nn.ReLU)):
                return None
        return list(zip(stages[0::3], stages[1::3]))

    def _native_training(self, instance_feature, anchor, residual, norm):
        """Whether this call's stages run their native training step (``native_training``): a call that needs
        autograd, fp32 GPU tensors, widths in ``STAGE_CHANNELS``, and stages that have a LayerNorm -- the three of a multi-layer
        block, or a single-layer block's ``norm(conv + residual)`` where ``output_proj`` is the identity and ``norm=`` is given,
        or a single-layer block whose ``output_proj`` has the native tail (``_tail_training``)."""
        if not self.native_training or self.embed_channels not in STAGE_CHANNELS or instance_feature.shape[-1] not in STAGE_CHANNELS:
            return False
        if isinstance(self.layer, SubMConv3d):
            if self._tail_training(norm):
                pass
            elif not isinstance(self.output_proj, nn.Identity) or norm is None or not _lib.norm_native(norm):
                return False
        elif self._stage_modules() is None:
            return False
        tensors = [instance_feature, anchor, residual, *self.parameters(), *_lib.norm_tensors(norm)]
        return _lib.native_tensors(tensors) and _lib.needs_grad(tensors)

    def _tail_training(self, norm):
        """Whether ``output_proj`` with the ``residual=`` / ``norm=`` behind it runs its native training step (§3.13f):
        ``native_tail_training``, a Linear with bias at width 128 and a norm the library takes."""
        proj = self.output_proj
        return self.native_tail_training and self.embed_channels == E_NATIVE and isinstance(proj, nn.Linear) and proj.bias is not None and _lib.norm_native(norm)

    def _forward_native_training(self, feats, rb, residual, norm, bs, g):
        """``[b, g, C]``: every stage that has a LayerNorm as a :class:`SubMStageFunction`, and ``output_proj`` with what follows
        it as ``deformable_output_autograd`` where ``_tail_training`` says so (torch ops otherwise).  ``duplicates="sum"``: the
        three stages are one chained Function; ``"last"``: the mask multiply sits between the stages, so they are three."""
        from .deformable_block import deformable_output_autograd   # (here: deformable_block's imports reach back to this package)
        tail = self._tail_training(norm)
        res = None if residual is None else residual.flatten(0, 1)
        if isinstance(self.layer, SubMConv3d):
            conv = self.layer
            if tail:
                out = conv(feats, rb.indices, bs, self._spatial, rulebook=rb)
                return deformable_output_autograd(out, self.output_proj, residual_mode="none", residual=res, norm=norm).unflatten(0, (bs, g))
            return subm_stage(rb.sources(feats, conv.duplicates), rb, conv.weight, bias=conv.bias, residual=res, norm=norm).unflatten(0, (bs, g))
        pairs = self._stage_modules()
        if all(conv.duplicates == "sum" for conv, _ in pairs):
            out = subm_stages(feats, rb, [dict(weight=conv.weight, bias=conv.bias, norm=ln, relu=True) for conv, ln in pairs])
        else:
            out = feats
            for conv, ln in pairs:
                out = subm_stage(rb.sources(out, conv.duplicates), rb, conv.weight, bias=conv.bias, norm=ln, relu=True)
        if tail:
            return deformable_output_autograd(out, self.output_proj, residual_mode="none", residual=res, norm=norm).unflatten(0, (bs, g))
        out = self.output_proj(out.unflatten(0, (bs, g)))
        if residual is not None:
            out = out + residual
        if norm is not None:
            out = _lib.apply_norm(out, norm)
        return out

    def _forward_native_tail(self, feats, rb, residual, norm):
        """``[b*g, 128]``: the block with every dense op behind a convolution inside that convolution's last pass, and
        ``output_proj`` with the encoder's ``"add"`` / ``"norm"`` in one ``gf_deform_output_forward`` launch."""
        from .deformable_block import deformable_output   # (here: deformable_block's imports reach back to this package)
        res = None if residual is None else residual.flatten(0, 1)
        proj = isinstance(self.output_proj, nn.Linear)
        if isinstance(self.layer, SubMConv3d):
            conv = self.layer
            if proj:
                out = rb.apply(rb.sources(feats, conv.duplicates), conv.weight, bias=conv.bias)
                return deformable_output(out, self.output_proj, residual_mode="none", residual=res, norm=norm)
            return rb.apply(rb.sources(feats, conv.duplicates), conv.weight, bias=conv.bias, residual=res, norm=norm)
        out = feats
        for conv, ln in self._stage_modules():
            out = rb.apply(rb.sources(out, conv.duplicates), conv.weight, bias=conv.bias, norm=ln, relu=True)
        if proj:
            return deformable_output(out, self.output_proj, residual_mode="none", residual=res, norm=norm)
        # (not the third stage's epilogue: its own LayerNorm and ReLU sit between the convolution and this add)
        if res is not None:
            out = out + res
        if norm is not None:
            out = _lib.apply_norm(out, norm)
        return out
