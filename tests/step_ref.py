"""Float64 restatement of the chained training step of tools/bench_step.py, in plain torch (TEST INFRASTRUCTURE, CPU or GPU).

The step, stage by stage: the anchor activations -> 4 x [submanifold conv (oracle/subm_ref.py's operator), ``weights_fc``,
the deformable block of tests/daf_fused_ref.py (projection, masked softmax, bilinear DAF, sum over key points)] -> the opacity
gate -> the head's pack (gaussian_head.py:88-109: zero column, whole-grid empty Gaussian or softmax) -> Sigma^-1
(oracle/prepare_ref.py) -> the splat (oracle/dense_ref.py's formulas, evaluated on the (Gaussian, voxel) pairs of the integer
boxes) -> the loss.  No native op is called.

Discrete decisions are inputs: the sparse-conv voxel indices, ``means3D_int`` and the radii come from the float32 rules the
product uses (:func:`decisions`); everything continuous is evaluated in the requested dtype.  :func:`step` runs in reverse mode
stage by stage -- the forward without autograd, keeping each stage's inputs, then each stage recomputed in slices under autograd
with the gradient of its output -- so that the step fits in memory at the benchmark's size; :func:`step_autograd` is the same
chain under one autograd graph, for small sizes (the check that slicing and the hand-off between stages lose nothing)."""
import math
import warnings

import torch

import daf_fused_ref as dref
from oracle.prepare_ref import covariance_inverse, pack6

CUT = 1e-9            # prob: a voxel whose probability sum is not above this gets the uniform row
NUM_CLASSES = 18


# ---- sparse convolution ----------------------------------------------------------------------------------------------------

def subm_conv_sparse(feat, idx, weight, batch, shape, K):
    """The operator of ``oracle.subm_ref.subm_conv3d_dense`` (duplicates in a cell sum, points outside the grid are inactive:
    they contribute nothing and receive zeros), evaluated sparsely: the features summed per occupied cell, then K^3 offset
    gathers through a sorted cell -> row table, ``index_add`` into the occupied cells' outputs, read back per point.
    ``feat [N, Cin]``, ``idx [N, 4]`` (batch, x, y, z), ``weight [K^3, Cin, Cout]`` -> ``[N, Cout]``; differentiable."""
    X, Y, Z = shape
    idx = idx.long().to(feat.device)
    b, x, y, z = idx.unbind(1)
    inside = (b >= 0) & (b < batch) & (x >= 0) & (x < X) & (y >= 0) & (y < Y) & (z >= 0) & (z < Z)
    lin = ((b * X + x) * Y + y) * Z + z
    cells, inv = torch.unique(lin[inside], return_inverse=True)                    # sorted occupied cells
    U = cells.shape[0]
    rows = torch.nonzero(inside).squeeze(1)
    cell_feat = feat.new_zeros(U, feat.shape[1]).index_add(0, inv, feat[rows])
    cb = cells // (X * Y * Z)
    cx, cy, cz = (cells // (Y * Z)) % X, (cells // Z) % Y, cells % Z
    out_cell = feat.new_zeros(U, weight.shape[2])
    r = K // 2
    for k in range(K ** 3):
        dx, dy, dz = k // (K * K) - r, (k // K) % K - r, k % K - r                  # cross-correlation: out[c] += in[c + d] W[d]
        nx, ny, nz = cx + dx, cy + dy, cz + dz
        ok = (nx >= 0) & (nx < X) & (ny >= 0) & (ny < Y) & (nz >= 0) & (nz < Z)
        key = ((cb * X + nx) * Y + ny) * Z + nz
        pos = torch.searchsorted(cells, key).clamp(max=max(U - 1, 0))
        ok &= cells[pos] == key if U else ok
        dst, src = torch.nonzero(ok).squeeze(1), pos[ok]
        if dst.numel():
            out_cell = out_cell.index_add(0, dst, cell_feat[src] @ weight[k])
    out = feat.new_zeros(feat.shape[0], weight.shape[2])
    return out.index_copy(0, rows, out_cell[inv])


# ---- splat -----------------------------------------------------------------------------------------------------------------

def box_bounds(means_int, radii, H, W, D):
    """The clipped integer boxes (src/auxiliary.h:8-20): ``lo, hi [P, 3]`` int64, ``hi`` exclusive."""
    mi = means_int.long()
    r = radii.long()
    r = r[:, None].expand(-1, 3) if r.dim() == 1 else r
    dims = torch.tensor([H, W, D], dtype=torch.long, device=mi.device)
    return torch.minimum(dims, (mi - r).clamp(min=0)), torch.minimum(dims, (mi + r + 1).clamp(min=0))


def pair_chunks(means_int, radii, H, W, D, budget=1 << 22):
    """Yields ``(g, key)``: Gaussian ids and voxel keys ((x W + y) D + z) of every (Gaussian, voxel) pair of the boxes, in
    chunks of about ``budget`` padded pairs (Gaussians of similar extent share a chunk, as oracle/torch_cpu_splat.py does)."""
    lo, hi = box_bounds(means_int, radii, H, W, D)
    ext = (hi - lo).clamp(min=0)
    vol = ext.prod(dim=1)
    order = torch.argsort(vol.cpu(), stable=True).to(lo.device)
    ext_s = ext[order].cpu()
    P, start = order.shape[0], 0
    while start < P:
        e_max = ext_s[start].clone()
        end = start + 1
        while end < P:
            e_new = torch.maximum(e_max, ext_s[end])
            if int(e_new.prod()) * (end - start + 1) > budget:
                break
            e_max, end = e_new, end + 1
        g = order[start:end]
        start = end
        ex, ey, ez = (int(v) for v in e_max)
        if ex * ey * ez == 0:
            continue
        dev = lo.device
        x = lo[g, 0][:, None, None, None] + torch.arange(ex, device=dev)[None, :, None, None]
        y = lo[g, 1][:, None, None, None] + torch.arange(ey, device=dev)[None, None, :, None]
        z = lo[g, 2][:, None, None, None] + torch.arange(ez, device=dev)[None, None, None, :]
        ok = (x < hi[g, 0][:, None, None, None]) & (y < hi[g, 1][:, None, None, None]) & (z < hi[g, 2][:, None, None, None])
        yield g[:, None, None, None].expand(ok.shape)[ok], ((x * W + y) * D + z)[ok]


def _pair_terms(pts, means3D, cov6, gi, key):
    """e = exp(power) of each pair (forward.cu:66-69; d = mean - point)."""
    d = means3D[gi] - pts[key]
    c = cov6[gi]
    power = -0.5 * (c[:, 0] * d[:, 0] * d[:, 0] + c[:, 1] * d[:, 1] * d[:, 1] + c[:, 2] * d[:, 2] * d[:, 2]) \
        - (c[:, 3] * d[:, 0] * d[:, 1] + c[:, 4] * d[:, 1] * d[:, 2] + c[:, 5] * d[:, 0] * d[:, 2])
    return torch.exp(power)


def _norm(cov6):
    """(2 pi)^-1.5 sqrt(det Sigma^-1) of oracle/dense_ref.py's prob formula."""
    xx, yy, zz, xy, yz, xz = cov6.unbind(-1)
    det = xx * yy * zz + 2 * xy * yz * xz - xx * yz * yz - yy * xz * xz - zz * xy * xy
    return (2 * math.pi) ** -1.5 * torch.sqrt(det)


def uniform_row(C, dtype, device):
    u = torch.full((C,), 1.0 / (C - 1), dtype=dtype, device=device)
    u[C - 1] = 0.0
    return u


def splat_pairs(variant, pts, points_int, means3D, means_int, opacity, semantics, radii, cov6, H, W, D, budget=1 << 22):
    """``oracle.dense_ref.splat_dense``'s base and prob formulas evaluated on the pairs of the integer boxes and ``index_add``ed
    into the grid, in the inputs' dtype, differentiable.  ``pts [N, 3]`` must be the dense voxel-centre grid (point n in voxel
    n = (x W + y) D + z, ``points_int`` only checked for that).  Returns logits (base) or (logits, bin_logits, density,
    prob_sum) (prob)."""
    N, C = pts.shape[0], semantics.shape[1]
    assert N == H * W * D and bool((((points_int[:, 0].long() * W + points_int[:, 1]) * D + points_int[:, 2])
                                    == torch.arange(N, device=points_int.device)).all())
    dt, dev = means3D.dtype, means3D.device
    opacity = opacity.reshape(-1)
    num = torch.zeros(N, C, dtype=dt, device=dev)
    if variant == "base":
        for gi, key in pair_chunks(means_int, radii, H, W, D, budget):
            num = num.index_add(0, key, (opacity[gi] * _pair_terms(pts, means3D, cov6, gi, key))[:, None] * semantics[gi])
        return num
    ps = torch.zeros(N, dtype=dt, device=dev)
    dens = torch.zeros(N, dtype=dt, device=dev)
    keep = torch.ones(N, dtype=dt, device=dev)
    norm = _norm(cov6)
    for gi, key in pair_chunks(means_int, radii, H, W, D, budget):
        e = _pair_terms(pts, means3D, cov6, gi, key)
        p = norm[gi] * e * opacity[gi]
        ps, dens = ps.index_add(0, key, p), dens.index_add(0, key, e)
        num = num.index_add(0, key, p[:, None] * semantics[gi])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                   # (index_reduce is marked beta)
            keep = keep.index_reduce(0, key, 1 - e, "prod")
    has = ps > CUT
    logits = torch.where(has[:, None], num / torch.where(has, ps, torch.ones_like(ps))[:, None], uniform_row(C, dt, dev))
    return logits, 1 - keep, dens, ps


def _splat_forward(variant, pts, means3D, means_int, opacity, semantics, radii, cov6, H, W, D):
    """Forward of the splat stage without autograd: base -> {logits}; prob -> {logits, bin_logits, density, prob_sum, keep}."""
    with torch.no_grad():
        N, C = pts.shape[0], semantics.shape[1]
        dt, dev = means3D.dtype, means3D.device
        opacity = opacity.reshape(-1)
        num = torch.zeros(N, C, dtype=dt, device=dev)
        if variant == "base":
            for gi, key in pair_chunks(means_int, radii, H, W, D):
                num.index_add_(0, key, (opacity[gi] * _pair_terms(pts, means3D, cov6, gi, key))[:, None] * semantics[gi])
            return dict(logits=num)
        ps, dens = torch.zeros(N, dtype=dt, device=dev), torch.zeros(N, dtype=dt, device=dev)
        keep = torch.ones(N, dtype=dt, device=dev)
        norm = _norm(cov6)
        for gi, key in pair_chunks(means_int, radii, H, W, D):
            e = _pair_terms(pts, means3D, cov6, gi, key)
            p = norm[gi] * e * opacity[gi]
            ps.index_add_(0, key, p)
            dens.index_add_(0, key, e)
            num.index_add_(0, key, p[:, None] * semantics[gi])
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")               # (index_reduce is marked beta)
                keep.index_reduce_(0, key, 1 - e, "prod")
        has = ps > CUT
        logits = torch.where(has[:, None], num / torch.where(has, ps, torch.ones_like(ps))[:, None], uniform_row(C, dt, dev))
        return dict(logits=logits, bin_logits=1 - keep, density=dens, prob_sum=ps, keep=keep)


def _splat_backward(variant, pts, means3D, means_int, opacity, semantics, radii, cov6, H, W, D, fwd, grads):
    """Vector-Jacobian product of the splat stage, Gaussians in slices: each slice's pairs recomputed under autograd against the
    per-voxel upstream gradients (prob: formed once from the forward's per-voxel sums).  -> grads of (means3D, opacity [P],
    semantics, cov6)."""
    dt = means3D.dtype
    gl = grads["logits"].to(dt)
    if variant == "prob":
        ps, keep, logits = fwd["prob_sum"], fwd["keep"], fwd["logits"]
        has = ps > CUT
        safe = torch.where(has, ps, torch.ones_like(ps))
        g_num = torch.where(has[:, None], gl / safe[:, None], torch.zeros_like(gl))           # d loss / d num
        g_ps = torch.where(has, -(gl * logits).sum(1) / safe, torch.zeros_like(ps))           # d loss / d prob_sum
        gb, gd = grads["bin_logits"].to(dt), grads["density"].to(dt)
    out = [torch.zeros_like(means3D), torch.zeros_like(opacity.reshape(-1)), torch.zeros_like(semantics), torch.zeros_like(cov6)]
    for gi_all, key_all in pair_chunks(means_int, radii, H, W, D):
        sl = torch.unique(gi_all)
        remap = torch.full((means3D.shape[0],), -1, dtype=torch.long, device=means3D.device)
        remap[sl] = torch.arange(sl.shape[0], device=means3D.device)
        gi = remap[gi_all]
        m, o, s, c = (t[sl].detach().clone().requires_grad_(True) for t in (means3D, opacity.reshape(-1), semantics, cov6))
        e = _pair_terms(pts, m, c, gi, key_all)
        if variant == "base":
            surrogate = ((o[gi] * e)[:, None] * s[gi] * gl[key_all]).sum()
        else:
            p = _norm(c)[gi] * e * o[gi]
            # bin_logits = 1 - prod(1 - e): d / d e_g = prod over the others = keep / (1 - e_g) (e_g = 1 needs a voxel centre exactly
            # on a Gaussian's mean)
            one_m = (1 - e).detach()
            g_e = gb[key_all] * torch.where(one_m != 0, keep[key_all] / torch.where(one_m != 0, one_m, torch.ones_like(one_m)),
                                            torch.zeros_like(one_m)) + gd[key_all]
            surrogate = (p * ((s[gi] * g_num[key_all]).sum(1) + g_ps[key_all])).sum() + (e * g_e).sum()
        gm, go, gs, gc = torch.autograd.grad(surrogate, (m, o, s, c))
        for acc, g in zip(out, (gm, go, gs, gc)):
            acc.index_add_(0, sl, g)
    return out


# ---- the step --------------------------------------------------------------------------------------------------------------

def decisions(named, const):
    """The integer decisions of the product's float32 rules, from the float32 leaves: the sparse-conv voxel indices
    (SparseConv3D._voxel_indices_torch), ``means3D_int`` (fp32 subtract, divide, truncate) and the radii (the ceil rule of the
    head's radii mode; prob clamps them to >= 1), the empty Gaussian appended where the head has one; and per block the float32
    sampling locations whose tap cells the bilinear samples use (daf_fused_ref.bilinear's ``cell_uv``): where a tap coordinate
    lies within float32 rounding of a pixel centre, the sample's location derivative jumps, and the truth is the float64
    evaluation on the side float32 chose."""
    from types import SimpleNamespace

    from gaussianformer_amd.sparse_conv import SparseConv3D
    anchor = named["anchor"].detach().float()
    dev = anchor.device
    pc = const["pc_range"]
    cell = const["cell"]
    # (the method's own state, without building a module: that would draw its weight from the global generator)
    sc = SimpleNamespace(use_sigmoid=True, _range=[float(v) for v in pc], pc_range=torch.tensor(pc, dtype=torch.float, device=dev),
                         grid_size=torch.tensor([cell] * 3, dtype=torch.float, device=dev))
    vox = SparseConv3D._voxel_indices_torch(sc, anchor)
    lo = torch.tensor(pc[:3], device=dev)
    span = torch.tensor(pc[3:], device=dev) - lo
    means = anchor[..., :3].clamp(-9.21, 9.21).sigmoid() * span + lo
    scales = anchor[..., 3:6].sigmoid() * (0.64 - 0.08) + 0.08
    means, scales = means[0], scales[0]
    if const["head"] == "empty":
        ea = const["empty_args"]
        means = torch.cat([means, torch.tensor([ea["mean"]], device=dev)])
        scales = torch.cat([scales, torch.tensor([ea["scale"]], device=dev)])
    means_int = ((means - lo[None]) / cell).to(torch.int)
    radii = torch.ceil(scales.max(dim=-1)[0] * const["scale_multiplier"] / cell).to(torch.int)
    if const["head"] == "prob":
        radii = radii.clamp(min=1)
    # the bilinear taps' cells: from the float32 key points of each block (the product's ops), projected in float32
    m32, s32, _, _ = _front(anchor, const)
    cells = [dref.project(_kp(m32, s32, b["key_offsets"].detach().float()), const["pm"].float(), const["wh"].float())[0]
             for b in named["blocks"]]
    return dict(voxels=vox, means_int=means_int, radii=radii, cells=cells)


def _front(anchor, const):
    """means, scales, rotations, opacity before the gate (bench_step.build's forward)."""
    pc = const["pc_range"]
    lo = anchor.new_tensor(pc[:3])
    span = anchor.new_tensor(pc[3:]) - lo
    means = anchor[..., :3].clamp(-9.21, 9.21).sigmoid() * span + lo
    scales = anchor[..., 3:6].sigmoid() * (0.64 - 0.08) + 0.08
    rots = torch.nn.functional.normalize(anchor[..., 6:10], dim=-1)
    return means, scales, rots, anchor[..., 10:11].sigmoid()


def _pack(head, means, scales, rots, sem_raw, opa, empty_scalar, const):
    """gaussian_head.py:88-109 as GaussianArgs._forward_torch states it (batch 1, nuScenes order), for the three heads ->
    [P', .] tensors: means, scales, rotations, semantics (18 columns), opacity [P'], and Sigma^-1 packed [P', 6]."""
    means, scales, rots, opa = means[0], scales[0], rots[0], opa[0, :, 0]
    if head == "plain":
        sem = torch.nn.functional.softplus(sem_raw[0])
    elif head == "empty":
        sem = torch.nn.functional.softplus(sem_raw[0])
        sem = torch.cat([sem, torch.zeros_like(sem[:, :1])], dim=1)
        ea = const["empty_args"]
        means = torch.cat([means, means.new_tensor([ea["mean"]])])
        scales = torch.cat([scales, scales.new_tensor([ea["scale"]])])
        rots = torch.cat([rots, rots.new_tensor([[1.0, 0.0, 0.0, 0.0]])])
        empty_sem = torch.cat([sem.new_zeros(1, NUM_CLASSES - 1), empty_scalar.reshape(1, 1).to(sem.dtype)], dim=1)
        sem = torch.cat([sem, empty_sem])
        opa = torch.cat([opa, opa.new_ones(1)])
    else:
        sem = sem_raw[0].softmax(dim=-1)
        sem = torch.cat([sem, torch.zeros_like(sem[:, :1])], dim=1)
    return means, scales, rots, sem, opa, pack6(covariance_inverse(scales, rots))


def _table(maps):
    """DAF.feature_maps_format in torch: the ``[b, cams, num_feat, C]`` table and its index tensors."""
    b, cams, C = maps[0].shape[:3]
    ss = torch.tensor([list(m.shape[-2:]) for m in maps], dtype=torch.int64, device=maps[0].device)
    st = torch.cat([ss.new_zeros(1), torch.cumsum(ss[:, 0] * ss[:, 1], 0)[:-1]])
    return torch.cat([m.reshape(b, cams, C, -1) for m in maps], dim=-1).permute(0, 1, 3, 2), ss, st


def _kp(means, scales, key_offsets):
    return means.unsqueeze(2) + key_offsets * scales.unsqueeze(2)


def _raw(feat, w, b, const):
    bs, A, _ = feat.shape
    cams, L = const["pm"].shape[1], len(const["levels"])
    return torch.nn.functional.linear(feat, w, b).reshape(bs, A, cams, L, const["key_pts"], const["groups"])


def _spconv(feat, w, vox, const):
    H, W, D = [int((const["pc_range"][3 + a] - const["pc_range"][a]) / const["cell"]) for a in range(3)]
    return feat + subm_conv_sparse(feat[0], vox, w, 1, (H, W, D), const["kernel_size"])[None]


def _loss(head, outs, targets):
    loss = (outs[0].reshape(-1, NUM_CLASSES) * targets[0]).mean()
    for o, t in zip(outs[1:], targets[1:]):
        loss = loss + (o.reshape(-1) * t).mean()
    return loss


def _leaves(named, dtype, grad):
    cast = lambda t: t.detach().to(dtype).requires_grad_(grad)
    out = dict(anchor=cast(named["anchor"]), sem_raw=cast(named["sem_raw"]), feat0=cast(named["feat0"]),
               maps=[cast(m) for m in named["maps"]], blocks=[{k: cast(v) for k, v in b.items()} for b in named["blocks"]])
    if "empty_scalar" in named:
        out["empty_scalar"] = cast(named["empty_scalar"])
    return out


def _grads(lv):
    out = dict(anchor=lv["anchor"].grad, sem_raw=lv["sem_raw"].grad, feat0=lv["feat0"].grad, maps=[m.grad for m in lv["maps"]],
               blocks=[{k: v.grad for k, v in b.items()} for b in lv["blocks"]])
    if "empty_scalar" in lv:
        out["empty_scalar"] = lv["empty_scalar"].grad
    return out


def _cast_const(const, dtype):
    return dict(pm=const["pm"].to(dtype), wh=const["wh"].to(dtype), pts=const["pts"].reshape(-1, 3).to(dtype),
                targets=[t.to(dtype) for t in const["targets"]])


def step_autograd(named, const, dec, dtype=torch.float64):
    """The whole step under one autograd graph (small sizes only) -> (outputs dict, leaf gradients dict)."""
    head = const["head"]
    cc = _cast_const(const, dtype)
    lv = _leaves(named, dtype, True)
    means, scales, rots, opa = _front(lv["anchor"], const)
    feat = lv["feat0"]
    for b, cells in zip(lv["blocks"], dec["cells"]):
        feat = _spconv(feat, b["spconv"], dec["voxels"], const)
        raw = _raw(feat, b["fc_weight"], b["fc_bias"], const)
        feat = feat + dref.block(_kp(means, scales, b["key_offsets"]), cc["pm"], cc["wh"], lv["maps"], raw, cell_uv=cells)
    opa = opa * feat.mean(-1, keepdim=True).sigmoid()
    m, s, q, sem, o, cov6 = _pack(head, means, scales, rots, lv["sem_raw"], opa, lv.get("empty_scalar"), const)
    H, W, D = const["grid"]
    pts_int = _points_int(const)
    outs = splat_pairs("prob" if head == "prob" else "base", cc["pts"], pts_int, m, dec["means_int"], o, sem, dec["radii"], cov6,
                       H, W, D)
    outs = outs[:3] if head == "prob" else (outs,)
    loss = _loss(head, outs, cc["targets"])
    loss.backward()
    names = ("logits", "bin_logits", "density")
    return dict(loss=loss.detach(), **{n: t.detach() for n, t in zip(names, outs)}), _grads(lv)


def _points_int(const):
    H, W, D = const["grid"]
    pts = const["pts"].reshape(-1, 3)
    return ((pts - pts.new_tensor(const["pc_range"][:3])) / const["cell"]).to(torch.int)


def _daf_forward(kp, pm, wh, maps, raw, cells, step):
    with torch.no_grad():
        outs = [dref.block(kp[:, s:s + step], pm, wh, maps, raw[:, s:s + step], cell_uv=cells[:, s:s + step])
                for s in range(0, kp.shape[1], step)]
    return torch.cat(outs, dim=1)


def step(named, const, dec, dtype=torch.float64, chunk=None):
    """The step in reverse mode, stage by stage (see the module docstring) -> (outputs dict: loss, logits [+ bin_logits, density,
    prob_sum], key_points per block; leaf gradients dict in the leaves' layouts)."""
    head = const["head"]
    variant = "prob" if head == "prob" else "base"
    cc = _cast_const(const, dtype)
    pm, wh, pts = cc["pm"], cc["wh"], cc["pts"]
    H, W, D = const["grid"]
    lv = _leaves(named, dtype, False)
    C = lv["feat0"].shape[-1]
    cams, L = pm.shape[1], len(const["levels"])
    step_a = max(1, (chunk or dref.slice_len(cams, C, L)) // const["key_pts"])

    # ---- forward, no autograd: each stage's inputs kept
    with torch.no_grad():
        means, scales, rots, opa0 = _front(lv["anchor"], const)
        table, ss, st = _table(lv["maps"])
        feat = lv["feat0"]
        saved = []
        for b, cells in zip(lv["blocks"], dec["cells"]):
            f_in = feat
            f_mid = _spconv(f_in, b["spconv"], dec["voxels"], const)
            raw = _raw(f_mid, b["fc_weight"], b["fc_bias"], const)
            kp = _kp(means, scales, b["key_offsets"])
            feat = f_mid + _daf_forward(kp, pm, wh, lv["maps"], raw, cells, step_a)
            saved.append((f_in, f_mid, raw, kp))
        feat_final = feat
        opa = opa0 * feat.mean(-1, keepdim=True).sigmoid()
        m, s, q, sem, o, cov6 = _pack(head, means, scales, rots, lv["sem_raw"], opa, lv.get("empty_scalar"), const)
        fwd = _splat_forward(variant, pts, m, dec["means_int"], o, sem, dec["radii"], cov6, H, W, D)
    names = ("logits", "bin_logits", "density") if head == "prob" else ("logits",)
    outs_leaf = [fwd[n].clone().requires_grad_(True) for n in names]
    loss = _loss(head, outs_leaf, cc["targets"])
    g_outs = dict(zip(names, torch.autograd.grad(loss, outs_leaf)))

    # ---- backward: the splat, then the head's small graph (pack, Sigma^-1, gate) back to means / scales / rotations / opacity
    gm, go, gs, gc = _splat_backward(variant, pts, m, dec["means_int"], o, sem, dec["radii"], cov6, H, W, D, fwd, g_outs)
    hm, hs, hq, ho0 = (t.detach().requires_grad_(True) for t in (means, scales, rots, opa0))
    hf = feat_final.detach().requires_grad_(True)
    es = lv.get("empty_scalar")
    if es is not None:
        es.requires_grad_(True)
    sem_raw = lv["sem_raw"].requires_grad_(True)
    ho = ho0 * hf.mean(-1, keepdim=True).sigmoid()
    pm_, ps_, pq_, psem, po, pcov = _pack(head, hm, hs, hq, sem_raw, ho, es, const)
    torch.autograd.backward([pm_, po, psem, pcov], [gm, go, gs, gc])
    g_means, g_scales, g_feat = hm.grad, hs.grad, hf.grad
    grads = dict(sem_raw=sem_raw.grad, maps=None, blocks=[None] * len(lv["blocks"]))
    if es is not None:
        grads["empty_scalar"] = es.grad

    # ---- the blocks in reverse
    g_table = torch.zeros_like(table)
    for bi in reversed(range(len(lv["blocks"]))):
        b = lv["blocks"][bi]
        f_in, f_mid, raw, kp = saved[bi]
        _, gd = dref.block_chunked(kp, pm, wh, table, ss, st, g_feat, raw=raw, dtype=dtype, chunk=chunk, cell_uv=dec["cells"][bi])
        g_table += gd["feat"]
        fm = f_mid.detach().requires_grad_(True)
        wf, bf = b["fc_weight"].detach().requires_grad_(True), b["fc_bias"].detach().requires_grad_(True)
        torch.autograd.backward(_raw(fm, wf, bf, const), gd["raw"])
        km, ks = means.detach().requires_grad_(True), scales.detach().requires_grad_(True)
        ko = b["key_offsets"].detach().requires_grad_(True)
        torch.autograd.backward(_kp(km, ks, ko), gd["kp"])
        g_means, g_scales = g_means + km.grad, g_scales + ks.grad
        fi = f_in.detach().requires_grad_(True)
        ws = b["spconv"].detach().requires_grad_(True)
        torch.autograd.backward(_spconv(fi, ws, dec["voxels"], const), g_feat + fm.grad)
        grads["blocks"][bi] = dict(spconv=ws.grad, fc_weight=wf.grad, fc_bias=bf.grad, key_offsets=ko.grad)
        g_feat = fi.grad
    grads["feat0"] = g_feat
    grads["maps"] = [t.contiguous() for t in dref.table_levels(g_table, ss, st)]

    # ---- the front: anchor -> means, scales, rotations, opacity
    an = lv["anchor"].detach().requires_grad_(True)
    fm_, fs_, fq_, fo_ = _front(an, const)
    torch.autograd.backward([fm_, fs_, fq_, fo_], [g_means, g_scales, hq.grad, ho0.grad])
    grads["anchor"] = an.grad
    out = dict(loss=loss.detach(), kp=[sv[3] for sv in saved], **{n: fwd[n] for n in names})
    if head == "prob":
        out["prob_sum"] = fwd["prob_sum"]
    return out, grads
