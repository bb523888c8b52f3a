"""Farthest point sampling: host mirror of ``pointops.farthest_point_sampling(xyz, offset, new_offset)`` as
GaussianLifterV2 calls it with ``random_sampling=False`` (model/lifter/gaussian_lifter_v2.py:233-251), backed by
``gf_farthest_point_sampling`` (include/gf_hip.h).

Semantics (this op's own contract; pointops' tie order is not available to pin): per segment the first pick is the
segment's first point, every point keeps ``d = 1e10``, each pick lowers ``d[p]`` to the squared distance
``(dx*dx + dy*dy) + dz*dz`` (fp32, no fused operations) when that is smaller, and the next pick is the point with the
largest ``d`` -- ties go to the LOWEST index.  More picks than points repeat by the same rule.  The result is
bit-for-bit deterministic.  At most 262 144 points per segment.

The offsets are read to the host once (as pointops does: a synchronisation), validated by the library, and handed to
the kernel as device int32 copies.  The output is indices, so autograd does not apply."""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_SEGMENT_POINTS = 262144


def farthest_point_sampling(xyz, offset, new_offset):
    """``idx [new_offset[-1]] int32 = farthest_point_sampling(xyz [n, 3] f32, offset [b], new_offset [b])``:
    segment ``s`` is points ``[offset[s-1], offset[s])`` and fills ``idx[new_offset[s-1]:new_offset[s]]`` with
    global indices into ``xyz``."""
    _lib.require_gpu(xyz)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"farthest_point_sampling: xyz must be [n, 3], got {tuple(xyz.shape)}")
    lib = _lib.load()
    dev = xyz.device
    off_h = np.ascontiguousarray(torch.as_tensor(offset).detach().cpu().numpy().reshape(-1), dtype=np.int64)
    new_h = np.ascontiguousarray(torch.as_tensor(new_offset).detach().cpu().numpy().reshape(-1), dtype=np.int64)
    if off_h.size != new_h.size or off_h.size == 0:
        raise ValueError(f"farthest_point_sampling: offset and new_offset must have the same length >= 1 "
                         f"({off_h.size} and {new_h.size})")
    if off_h.max(initial=0) >= 2 ** 31 or new_h.max(initial=0) >= 2 ** 31 or min(off_h.min(), new_h.min()) < 0:
        raise ValueError("farthest_point_sampling: offsets out of the int32 range")
    off_h, new_h = off_h.astype(np.int32), new_h.astype(np.int32)
    n, b, total = int(xyz.shape[0]), int(off_h.size), int(new_h[-1])
    p = _lib.as_arg(xyz)
    off_d = torch.from_numpy(off_h).to(dev)
    new_d = torch.from_numpy(new_h).to(dev)
    idx = torch.empty(max(total, 0), dtype=torch.int32, device=dev)
    ws_bytes = lib.gf_fps_workspace_bytes(n)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    _lib.call("gf_farthest_point_sampling", dev, n, b, off_h.ctypes.data_as(ctypes.c_void_p),
              new_h.ctypes.data_as(ctypes.c_void_p), p, off_d, new_d, idx, ws, ws_bytes)
    return idx
