"""ctypes binding of ``libgf_hip.so`` (C ABI declared in ``include/gf_hip.h``).

There is NO fallback: if the library is missing or a call fails, a ``RuntimeError`` is
raised.  Tensors cross the boundary as raw device pointers + sizes; the stream is torch's
current HIP stream.

Also here, once for every module above: how arguments and parameter tables are made (``as_arg``, ``aligned``, ``param_table``,
``out_table``), how a training Function carries its parameter list to its backward (``ParamSlots``), and the
questions the modules' routes share (``needs_grad``, ``native_tensors``, ``refuse_autograd``, the post norm's ``norm_*``).
"""
import collections
import contextlib
import ctypes
import os

import torch
import torch.nn as nn

_HERE = os.path.dirname(os.path.abspath(__file__))
# GF_LIB selects an instrumentation build (-DGF_TIMELINE=1, -DGF_DAF_TL) made by build.build(lib_name=...) (tools/ only)
LIB_PATH = os.environ.get("GF_LIB") or os.path.join(_HERE, "csrc", "libgf_hip.so")

GF_ABI_VERSION = 10
GF_SPLAT_BASE, GF_SPLAT_PROB = 0, 1
GF_NUM_CHANNELS = 18
GF_LABELS_ARGMAX, GF_LABELS_PROB_THRESHOLD, GF_LABELS_PROB_GEOSEM = 0, 1, 2
GF_RADII_SCALAR, GF_RADII_SCALAR_CLAMPED, GF_RADII_PER_AXIS = 0, 1, 2
GF_PREPARE_MEAN_OUT_OF_GRID, GF_PREPARE_RADIUS_BELOW_ONE = 1, 2
GF_PTS_AUTO, GF_PTS_ASSUME_DENSE, GF_PTS_GENERAL, GF_FAST_EXP, GF_LIBM_EXP, GF_COMP_EXP = 0, 1, 2, 4, 8, 16
GF_PROB_NUMERATOR = 32
GF_PROB_EXACT_DET = 64
GF_MFMA_SPLAT = 128
GF_EXACT_FP32 = 256
GF_RECORDS_VALID = 512
GF_PREPARE_BACKWARD = 1024
GF_WORKSPACE_ZEROED = 2048
GF_OCC_PROB, GF_OCC_MASK, GF_OCC_LOVASZ_IGNORE, GF_OCC_IGNORE_EMPTY, GF_OCC_NO_LOVASZ, GF_OCC_SCAL, GF_OCC_MAX_LAYERS = 1, 2, 4, 8, 16, 32, 8
GF_LIFT_MAX_BINS, GF_LIFT_MAX_ANCHORS, GF_PIXEL_LOSS_SOFTMAX, GF_PIXEL_LOSS_SIGMOID = 256, 8, 1, 2
GF_DCN_MAX_KERNEL, GF_DCN_CHANNEL_GRANULE = 7, 32
GF_MIOU_TARGETS_U8, GF_MIOU_FILTER_MINMAX, GF_MIOU_REMAP, GF_MIOU_MAX_CLASSES, GF_MIOU_MAX_D = 1, 2, 4, 32, 64
GF_REFINE_RESTRICT_XYZ, GF_REFINE_XYZ_IDENTITY, GF_REFINE_OPACITY, GF_REFINE_SEM_SOFTMAX, GF_REFINE_SEM_SOFTPLUS = 1, 2, 4, 8, 16
GF_REFINE_MLP_PARAMS, GF_REFINE_MLP_WGRAD_ROWS, GF_REFINE_MLP_CHUNK_ROWS = 15, 512, 32768
GF_ANCHOR_EMBED_DIMS, GF_ANCHOR_EMBED_MAX_S, GF_ANCHOR_EMBED_PARAMS, GF_ANCHOR_EMBED_WGRAD_ROWS, GF_ANCHOR_EMBED_CHUNK_ROWS = 128, 32, 48, 512, 65536
GF_FFN_PARAMS, GF_FFN_EMBED_DIMS, GF_FFN_HIDDEN, GF_FFN_WGRAD_ROWS, GF_FFN_CHUNK_ROWS = 10, 128, 512, 512, 32768
GF_DEFORM_EMBED_DIMS, GF_DEFORM_MAX_LEARNED, GF_DEFORM_LOGITS_PARAMS, GF_DEFORM_OUTPUT_PARAMS, GF_DEFORM_OUTPUT_WGRAD_ROWS = 128, 32, 4, 4, 512
GF_DEFORM_NONE, GF_DEFORM_ADD, GF_DEFORM_CAT = 0, 1, 2
GF_DEFORM_LOGITS_WGRAD_ROWS = 512
GF_PATH_EXACT_TILE, GF_PATH_MATRIX_CORE, GF_PATH_ARBITRARY, GF_PATH_MATRIX_CORE_WAVE, GF_PATH_MATRIX_CORE_PAIR, GF_PATH_MATRIX_CORE_SOLO = 0, 1, 2, 3, 4, 5
GF_PATHS_MATRIX_CORE = (GF_PATH_MATRIX_CORE, GF_PATH_MATRIX_CORE_WAVE, GF_PATH_MATRIX_CORE_PAIR, GF_PATH_MATRIX_CORE_SOLO)
GF_STATE_NOT_DENSE, GF_STATE_PATH, GF_STATE_VERDICT, GF_STATE_GENERATION, GF_STATE_ROWS, GF_STATE_WORDS = 0, 1, 2, 3, 4, 5
GF_VERDICT_POINT, GF_VERDICT_LATTICE, GF_VERDICT_THETA, GF_VERDICT_OPASEM = 1, 2, 4, 8
GF_ROWS_READY, GF_ROWS_OVERFLOW = 1, 2
GF_SPLAT_FLAG_BYTES = 32 * 1024
STATE_USED_BYTES = 4 * GF_STATE_WORDS   # the part of the state block (gf_splat_state_bytes) that carries words

_vp, _i, _sz, _f, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_longlong

# name -> (restype, argtypes); must list every symbol include/gf_hip.h declares
SIGNATURES = {
    "gf_abi_version": (_i, []),
    "gf_last_error": (ctypes.c_char_p, []),
    "gf_set_option": (_i, [ctypes.c_char_p, _i]),
    "gf_get_option": (_i, [ctypes.c_char_p, _vp]),
    "gf_is_development_build": (_i, []),
    "gf_splat_workspace_bytes": (_sz, [_i] * 5),
    "gf_splat_state_bytes": (_sz, []),
    "gf_splat_forward": (_i, [_i] * 9 + [_vp] * 13 + [_vp, _sz, _vp]),
    "gf_splat_forward_labels": (_i, [_i] * 9 + [_vp] * 12 + [_i, _f, _i, _vp] + [_vp, _vp, _sz, _vp]),
    "gf_splat_backward": (_i, [_i] * 9 + [_vp] * 20 + [_vp, _sz, _vp]),
    "gf_splat_box_volumes": (_i, [_i] * 5 + [_vp] * 5),
    "gf_daf_forward": (_i, [_i] * 7 + [_vp] * 7),
    "gf_daf_forward_pinned": (_i, [_i] * 7 + [_vp] * 7),
    "gf_daf_backward": (_i, [_i] * 7 + [_vp] * 10),
    "gf_daf_backward_workspace_bytes": (_sz, [_i] * 7),
    "gf_daf_backward_sorted": (_i, [_i] * 7 + [_vp] * 9 + [_vp, _sz, _vp]),
    "gf_subm_voxelize": (_i, [ctypes.c_longlong, _i, _i, _i] + [_vp] * 6 + [_vp]),
    "gf_subm_tables_bytes": (_sz, [_i] * 6),
    "gf_subm_rulebook_count": (_i, [_i] * 6 + [_vp, _vp, _sz, _vp]),
    "gf_subm_rulebook_fill": (_i, [_i] * 6 + [_vp] * 4 + [_vp]),
    "gf_subm_rulebook_build": (_i, [_i] * 6 + [_vp, _vp, _sz, _vp, _vp, ctypes.c_longlong, _vp]),
    "gf_subm_rulebook_count_range": (_i, [_i] * 8 + [_vp, _vp, _sz, _vp]),
    "gf_subm_rulebook_fill_range": (_i, [_i] * 8 + [_vp] * 4 + [_vp]),
    "gf_subm_rulebook_build_range": (_i, [_i] * 8 + [_vp, _vp, _sz, _vp, _vp, ctypes.c_longlong, _vp]),
    "gf_subm_conv_apply": (_i, [_i] * 8 + [ctypes.c_longlong] + [_vp] * 6 + [_vp]),
    "gf_subm_apply_scratch_bytes": (_sz, [_i, _i]),
    "gf_subm_conv_apply_scratch": (_i, [_i] * 8 + [ctypes.c_longlong] + [_vp] * 6 + [_vp, _sz, _vp]),
    "gf_subm_conv_apply_epilogue": (_i, [_i] * 8 + [ctypes.c_longlong] + [_vp] * 6 + [_vp, _sz] + [_vp] * 4 + [_i, _vp]),
    "gf_subm_stage_train_sizes": (_i, [_i] * 2 + [_vp] * 2),
    "gf_subm_conv_apply_epilogue_train": (_i, [_i] * 8 + [ctypes.c_longlong] + [_vp] * 6 + [_vp, _sz] + [_vp] * 4 + [_i, _vp, _vp]),
    "gf_subm_stage_backward": (_i, [_i] * 2 + [_vp] * 4 + [_i] + [_vp] * 5 + [_sz, _vp]),
    "gf_subm_conv_apply_stage_backward": (_i, [_i] * 8 + [ctypes.c_longlong] + [_vp] * 5 + [_vp, _sz] + [_vp] * 3 + [_i] + [_vp] * 5 + [_sz, _vp]),
    "gf_subm_conv_weight_grad": (_i, [_i] * 8 + [ctypes.c_longlong] + [_vp] * 6 + [_vp]),
    "gf_feature_maps_format": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "gf_head_labels": (_i, [ctypes.c_longlong, _i, _i, _vp, _vp, _f, _i, _vp, _vp]),
    "gf_head_geosem_forward": (_i, [_ll, _i] + [_vp] * 4 + [_vp]),
    "gf_head_geosem_backward": (_i, [_ll, _i] + [_vp] * 5 + [_vp]),
    "gf_daf_fused_forward": (_i, [_i] * 8 + [_vp] * 11),
    "gf_daf_fused_forward_masked": (_i, [_i] * 8 + [_vp] * 12),
    "gf_daf_fused_backward_workspace_bytes": (_sz, [_i] * 6),
    "gf_daf_fused_backward": (_i, [_i] * 8 + [_vp] * 17 + [_sz, _vp]),
    "gf_daf_prepare": (_i, [_i] * 6 + [_vp] * 7 + [_vp]),
    "gf_daf_prepare_backward": (_i, [_i] * 6 + [_vp] * 8 + [_vp]),
    "gf_gaussian_prepare": (_i, [_i] * 4 + [_vp, _f, _f, _i, _i] + [_vp] * 8 + [_vp]),
    "gf_gaussian_prepare_backward": (_i, [_i] * 2 + [_vp] * 5 + [_vp]),
    "gf_gaussian_pack": (_i, [_i] * 7 + [_vp] * 14 + [_vp]),
    "gf_key_points": (_i, [_i] * 4 + [_vp] * 4 + [_f] * 3 + [_i, _vp, _vp]),
    "gf_key_points_backward": (_i, [_i] * 4 + [_vp] * 4 + [_f] * 3 + [_i] + [_vp] * 3 + [_vp]),
    "gf_fps_workspace_bytes": (_sz, [_i]),
    "gf_farthest_point_sampling": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gf_occ_loss_workspace_bytes": (_sz, [_i] * 4),
    "gf_occ_loss_scratch_bytes": (_sz, [_i] * 4),
    "gf_occ_loss_forward": (_i, [_i] * 4 + [_vp, _ll, _ll] + [_vp] * 3 + [_f, _f] + [_i] * 3 + [_vp, _vp, _sz, _vp, _sz, _vp]),
    "gf_occ_loss_backward": (_i, [_i] * 4 + [_vp, _ll, _ll] + [_vp] * 3 + [_f, _f] + [_i] * 3 + [_vp, _vp, _vp, _sz, _vp]),
    "gf_occ_loss_scal_forward": (_i, [_i] * 4 + [_vp, _ll, _ll] + [_vp] * 3 + [_f] * 4 + [_i] * 3 + [_vp, _vp, _sz, _vp, _sz, _vp]),
    "gf_occ_loss_scal_backward": (_i, [_i] * 4 + [_vp, _ll, _ll] + [_vp] * 3 + [_f] * 4 + [_i] * 3 + [_vp, _vp, _vp, _sz, _vp]),
    "gf_miou_workspace_size": (_sz, [_ll, _i, _i]),
    "gf_miou_step": (_i, [_ll, _i, _i] + [_vp] * 3 + [_i, _vp, _i, _i] + [_vp, _vp] + [_vp, _sz, _vp]),
    "gf_miou_step_logits": (_i, [_ll, _i, _i, _i, _i] + [_vp, _vp, _f] + [_vp, _vp] + [_i, _vp, _i, _i] + [_vp, _vp] + [_vp, _sz, _vp]),
    "gf_lift_workspace_bytes": (_sz, [_i] * 3),
    "gf_lift_pixels": (_i, [_i] * 6 + [_vp] * 5 + [_f] + [_i] * 3 + [_vp] * 6 + [_vp, _sz, _vp]),
    "gf_pixel_loss_workspace_bytes": (_sz, [_i] * 2),
    "gf_pixel_loss_forward": (_i, [_i] * 3 + [_vp] * 3 + [_vp, _sz, _vp]),
    "gf_pixel_loss_backward": (_i, [_i] * 3 + [_vp] * 4 + [_vp]),
    "gf_dcn_workspace_bytes": (_sz, [_i] * 16),
    "gf_dcn_forward": (_i, [_i] * 15 + [_vp] * 6 + [_vp, _sz, _vp]),
    "gf_dcn_backward": (_i, [_i] * 15 + [_vp] * 10 + [_vp, _sz, _vp]),
    "gf_refine_forward": (_i, [_i] * 7 + [_vp] * 11 + [_vp]),
    "gf_refine_backward": (_i, [_i] * 7 + [_vp] * 13 + [_vp]),
    "gf_refine_mlp_forward": (_i, [_i] * 8 + [_vp] * 14 + [_vp]),
    "gf_refine_mlp_train_sizes": (_i, [_i] * 3 + [_vp] * 2),
    "gf_refine_mlp_forward_train": (_i, [_i] * 8 + [_vp] * 14 + [_vp, _sz, _vp]),
    "gf_refine_mlp_backward": (_i, [_i] * 8 + [_vp] * 18 + [_vp, _sz, _vp]),
    "gf_anchor_embed_forward": (_i, [_i] * 5 + [_vp] * 3 + [_vp]),
    "gf_anchor_embed_train_sizes": (_i, [_i] * 3 + [_vp] * 2),
    "gf_anchor_embed_forward_train": (_i, [_i] * 5 + [_vp] * 3 + [_vp, _sz, _vp]),
    "gf_anchor_embed_backward": (_i, [_i] * 5 + [_vp] * 6 + [_vp, _sz, _vp]),
    "gf_ffn_forward": (_i, [_i] * 4 + [_vp] * 4 + [_vp]),
    "gf_ffn_train_sizes": (_i, [_i] * 2 + [_vp] * 2),
    "gf_ffn_forward_train": (_i, [_i] * 4 + [_vp] * 3 + [_vp, _f, _vp, _f] + [_vp] + [_vp, _sz, _vp]),
    "gf_ffn_backward": (_i, [_i] * 4 + [_vp] * 2 + [_vp, _f, _vp, _f] + [_vp] * 5 + [_vp, _sz, _vp]),
    "gf_deform_logits_forward": (_i, [_i] * 4 + [_vp] * 5 + [_vp]),
    "gf_deform_output_forward": (_i, [_i] * 3 + [_vp] * 5 + [_vp]),
    "gf_deform_output_train_sizes": (_i, [_i] * 4 + [_vp] * 2),
    "gf_deform_output_forward_train": (_i, [_i] * 3 + [_vp] * 5 + [_vp, _sz, _vp]),
    "gf_deform_output_backward": (_i, [_i] * 3 + [_vp] * 8 + [_vp, _sz, _vp]),
    "gf_deform_logits_train_sizes": (_i, [_i] * 4 + [_vp] * 2),
    "gf_deform_logits_backward": (_i, [_i] * 4 + [_vp] * 8 + [_vp, _sz, _vp]),
    "gf_profile_enable": (_i, [_i]),
    "gf_profile_stride": (_i, [_i]),
    "gf_profile_read": (_i, [_vp, _i]),
}

_lib = None


def load():
    """Load the library (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension has not been built. "
            "Run `python -m gaussianformer_amd.build` (needs hipcc; cross-compiles gfx950 without a GPU). "
            "There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.gf_abi_version() != GF_ABI_VERSION:
        raise RuntimeError(f"libgf_hip.so ABI {lib.gf_abi_version()} != expected {GF_ABI_VERSION}; rebuild")
    _lib = lib
    return lib


@contextlib.contextmanager
def routed_to(other):
    """Inside the block ``load()`` and ``call()`` use ``other``, another build of the library with ``SIGNATURES`` applied to
    the entry points it has (``tools/bench_loss.py --parent-lib`` times a parent commit's build this way)."""
    global _lib
    own = load()
    _lib = other
    try:
        yield other
    finally:
        _lib = own


def load_other(path):
    """Another build of the library, or of some of its entry points, for ``routed_to``: not cached, no ABI check."""
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().gf_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def set_option(name, value):
    """``gf_set_option``: a process-wide library option (include/gf_hip.h); explicit calls -- the library never reads the
    environment.  Returns the previous value."""
    lib = load()
    old = ctypes.c_int(0)
    check(lib.gf_get_option(name.encode(), ctypes.addressof(old)), f"gf_get_option({name})")
    check(lib.gf_set_option(name.encode(), int(value)), f"gf_set_option({name})")
    return old.value


def get_option(name):
    lib = load()
    v = ctypes.c_int(0)
    check(lib.gf_get_option(name.encode(), ctypes.addressof(v)), f"gf_get_option({name})")
    return v.value


class option:
    """``with _lib.option("splat.mfma_tile_kernel", 1): ...`` -- sets a library option for the block and restores it."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)
        return False


def is_development_build():
    return bool(load().gf_is_development_build())


def ptr(t):
    """Device pointer of a tensor (``None`` -> NULL)."""
    return None if t is None else t.data_ptr()


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "gaussianformer_amd ops run on MI355X only (HIP kernels); got a CPU tensor. "
                "There is no CPU fallback -- move the inputs to the GPU.")


def current_stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def as_arg(t, dtype=torch.float32):
    """An input as the library reads it: detached, of ``dtype`` (converted only when it differs) and contiguous; ``None`` stays
    ``None``."""
    if t is None:
        return None
    t = t.detach()
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def needs_grad(tensors):
    """Whether autograd would record a call on ``tensors`` (``None``s skipped)."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def refuse_autograd(name, tensors, hint):
    """A forward-only function's refusal of a call that autograd would record; ``hint`` says where training goes instead."""
    if needs_grad(tensors):
        raise RuntimeError(
            f"{name} is a forward without a native backward: call it under torch.no_grad() or with inputs and parameters that "
            f"do not require grad {hint}")


def native_tensors(tensors):
    """Whether every entry is ``None`` or an fp32 GPU tensor: what a module's native route asks of its inputs and parameters."""
    return all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in tensors)


# The post norm: the ``norm`` behind a block that the block's launch takes in (the encoder's ``"norm"``): ``None``, an affine
# ``nn.LayerNorm`` with eps 1e-5 (the kernels' constant), or its ``(weight, bias)`` pair.

def norm_pair(norm, what):
    """``(weight, bias)`` of a post norm, ``(None, None)`` for ``None``; anything else is refused under the caller's name."""
    if norm is None:
        return None, None
    if not norm_native(norm):
        raise ValueError(f"{what}: norm must be an affine LayerNorm with eps = 1e-5, or a (weight, bias) pair")
    return (norm.weight, norm.bias) if isinstance(norm, nn.Module) else tuple(norm)


def norm_native(norm):
    """Whether ``norm`` is a post norm as the library takes it (what ``norm_pair`` accepts, as a question)."""
    if norm is None:
        return True
    if isinstance(norm, nn.Module):
        return isinstance(norm, nn.LayerNorm) and not (norm.eps != 1e-5 or norm.weight is None or norm.bias is None)
    return isinstance(norm, (tuple, list)) and len(norm) == 2 and all(isinstance(t, torch.Tensor) for t in norm)


def norm_tensors(norm):
    """The tensors of a ``norm`` argument of any kind (a module's parameters, a pair's entries, none for ``None``)."""
    return list(norm.parameters()) if isinstance(norm, nn.Module) else list(norm or ())


def apply_norm(x, norm):
    """The post norm as a torch op, on the routes that do not take it into a launch."""
    return norm(x) if isinstance(norm, nn.Module) else nn.functional.layer_norm(x, (x.shape[-1],), norm[0], norm[1], 1e-5)


def aligned(t):
    """``as_arg(t)``, cloned where its address is not a multiple of 16 (the kernels move rows as float4s)."""
    t = as_arg(t)
    return t.clone() if t is not None and t.data_ptr() % 16 else t


def param_table(params, count):
    """``(table, held)``: the library's host table of ``count`` INPUT pointers (NULL for ``None``), and the tensors it points
    into, in the list's order without the ``None``s: a parameter as it is, or its converted copy (another dtype, not
    contiguous, misaligned), which the caller keeps alive until the launch is queued (the caching allocator orders its reuse)."""
    table = (ctypes.c_void_p * count)()
    held = []
    for i, p in enumerate(params):
        if p is None:
            continue
        if p.dtype != torch.float32 or not p.is_contiguous() or p.data_ptr() % 16:   # (a module's own parameters: never)
            p = aligned(p)
        held.append(p)
        table[i] = p.data_ptr()
    return ctypes.cast(table, ctypes.c_void_p), held


def out_table(tensors, count):
    """The host table of ``count`` OUTPUT pointers: the tensors themselves, never a copy -- what the library writes must land in
    them -- so each has to be what the library writes already."""
    table = (ctypes.c_void_p * count)()
    for i, t in enumerate(tensors):
        if t is not None:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16:
                raise ValueError("a gradient buffer must be a contiguous, 16-byte aligned float32 tensor")
            table[i] = t.data_ptr()
    return ctypes.cast(table, ctypes.c_void_p)


class ParamSlots:
    """A training ``autograd.Function``'s parameter list between its forward and its backward.  Three
    things correspond slot by slot: the list in the library's table order with ``None`` for an absent parameter; the tensors
    handed to the library (``param_table``'s ``held``: a parameter itself, or its converted copy), which travel through
    ``save_for_backward`` without the ``None``s; and each slot's own dtype, which its gradient goes back in.  This record
    holds the count and the dtypes and no tensor, so it is kept on ``ctx``.  Which slots get a gradient buffer is the op's
    decision, passed as a list of booleans."""

    def __init__(self, params, count):
        self.count = count
        self.dtypes = [None if p is None else p.dtype for p in params]

    @classmethod
    def pack(cls, params, count):
        """The forward's ``(slots, table, held)``: ``param_table(params, count)`` and the record; ``held`` is appended to
        ``save_for_backward``."""
        table, held = param_table(params, count)
        return cls(params, count), table, held

    def _spread(self, held):
        it = iter(held)
        return [None if d is None else next(it) for d in self.dtypes]

    def unpack(self, held):
        """The backward's ``(params, table)`` from the held tensors as ``ctx.saved_tensors`` returns them: the list with its
        ``None`` slots again, and a table made anew of exactly these tensors -- saved-tensor hooks may have handed back other
        storage than the forward's table pointed into, and what ``param_table`` had to copy of it stays alive in ``params``."""
        table, held = param_table(self._spread(held), self.count)
        return self._spread(held), table

    def grad_buffers(self, params, wanted):
        """``(grads, table)``: a buffer like the held tensor for every present slot whose ``wanted`` entry is true, ``None``
        (the library: a NULL slot) for the others, and their ``out_table``."""
        grads = [torch.empty_like(p) if p is not None and w else None for p, w in zip(params, wanted)]
        return grads, out_table(grads, self.count)

    def returned(self, grads, needed):
        """The gradients as ``backward`` returns them, one per slot: each buffer in its slot's own dtype where ``needed`` (the
        slots' part of ``ctx.needs_input_grad``, in the slots' order) says so, ``None`` otherwise."""
        return tuple(g.to(d) if g is not None and n else None for g, d, n in zip(grads, self.dtypes, needed))


def train_sizes(symbol, *ints):
    """``(saved_bytes, workspace_bytes)`` of a native training step: the size query ``symbol(*ints, &saved, &workspace)``."""
    saved, work = ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(getattr(load(), symbol)(*ints, ctypes.addressof(saved), ctypes.addressof(work)), symbol)
    return saved.value, work.value


_Tensor = torch.Tensor   # (a global of this module: call() tests every argument against it)


def call(name, device, *args):
    """The one way to launch: calls the entry point ``name`` of the loaded library with ``args`` -- every tensor as its data
    pointer, ``None`` (NULL), numbers and ctypes objects as they are -- and torch's current stream of ``device`` appended, with
    ``device`` current during the call (the launch goes to the tensors' device, not the current one; no guard is entered when
    it is current already), and raises under that same name if it fails.  The callers have refused CPU tensors already
    (``require_gpu``); a ``device`` that is not a GPU gets no guard and a NULL stream, for calls the library refuses before it
    touches a device."""
    fn = getattr(_lib or load(), name)
    argv = [a.data_ptr() if isinstance(a, _Tensor) else a for a in args]
    if device.type != "cuda":
        rc = fn(*argv, None)
    elif torch.cuda.current_device() == device.index:
        rc = fn(*argv, torch.cuda.current_stream(device).cuda_stream)
    else:
        with torch.cuda.device(device):
            rc = fn(*argv, torch.cuda.current_stream(device).cuda_stream)
    if rc:
        check(rc, name)


def host_copy(words, device):
    """``(host, event)``: the device tensor ``words`` copied to pinned host memory on ``device``'s current stream, and an event
    behind the copy -- to be queried, never waited for.  ``(None, None)`` while the stream is being captured into a graph: no
    host allocation there."""
    if torch.cuda.is_current_stream_capturing():
        return None, None
    host = torch.empty(words.shape, dtype=words.dtype, pin_memory=True)
    host.copy_(words, non_blocking=True)
    event = torch.cuda.Event()
    event.record(torch.cuda.current_stream(device))
    return host, event


class SplatState(collections.namedtuple("SplatState", "not_dense path verdict generation rows_ready rows_overflow on_matrix_cores")):
    """A forward's state block decoded (``include/gf_hip.h``, ``gf_splat_state_bytes``): the ``GF_PATH_*`` value, the ``GF_VERDICT_*``
    bits, the two ``GF_ROWS_*`` bits as bools; ``on_matrix_cores`` = dense pts and one of ``GF_PATHS_MATRIX_CORE`` rendered."""

    @classmethod
    def of(cls, src):
        """From the words as a list of ints (words a caller did not read count as 0), or from a state tensor -- the uint8 block or
        an int32 view of it: a device tensor is copied to the host here, which SYNCHRONISES with the device."""
        if isinstance(src, _Tensor):
            src = (src[:STATE_USED_BYTES].view(torch.int32) if src.dtype == torch.uint8 else src).tolist()
        nd, path, verdict, gen, rows = ([int(x) for x in src] + [0] * GF_STATE_WORDS)[:GF_STATE_WORDS]
        return cls(nd != 0, path, verdict, gen, bool(rows & GF_ROWS_READY), bool(rows & GF_ROWS_OVERFLOW), nd == 0 and path in GF_PATHS_MATRIX_CORE)


class StreamScratch:
    """Scratch reused across calls, one grow-only buffer per (device, stream): the kernels of a call run on torch's current
    stream, so two calls on different streams must not share it.  A buffer is allocated while its stream is current, so the
    caching allocator frees it in that stream's order.  The cache is bounded: after a hand-out, while it holds more than
    ``MAX_STREAMS`` buffers the least recently used one goes -- a process that keeps creating streams does not accumulate a
    buffer per stream ever used, and a recycled stream handle meets at worst its own old buffer.  A new buffer has at least
    ``min_bytes``, and its first ``zeroed_bytes`` are zeroed then and never afterwards."""
    MAX_STREAMS = 8

    def __init__(self, min_bytes=0, zeroed_bytes=0, stream_of=current_stream):
        self.min_bytes, self.zeroed_bytes, self.stream_of = min_bytes, zeroed_bytes, stream_of
        self._cache = {}
        self._uses = 0

    def get(self, device, nbytes):
        """The current stream's buffer, at least ``nbytes`` long."""
        key = (device.type, device.index, self.stream_of(device))
        buf = self._cache.pop(key, None)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, self.min_bytes), dtype=torch.uint8, device=device)
            if self.zeroed_bytes:
                buf[:self.zeroed_bytes].zero_()
        self._cache[key] = buf              # most recently used last
        while len(self._cache) > self.MAX_STREAMS:
            self._cache.pop(next(iter(self._cache)))
        self._uses += 1
        return buf

    def stamp(self, device):
        """(stream, its buffer, number of hand-outs of this cache so far): equal stamps = nobody has been given this cache's
        scratch in between, so the buffer still holds what the last call left in it."""
        key = (device.type, device.index, self.stream_of(device))
        buf = self._cache.get(key)
        return (key, None if buf is None else buf.data_ptr(), self._uses)
