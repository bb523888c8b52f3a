"""Float64 torch restatement of the reference's deformable-aggregation block for training
(model/encoder/gaussian_encoder/deformable_module.py:174-242): project_points (:268-285), the visibility and keep-mask
(:199-207), all_miss (:208-210), the masked softmax over (key points, cameras, levels) per group (:211-221), the bilinear
DAF of ops/src/deformable_aggregation_cuda.cu:13-53,125-187 (taps outside the image are 0, sampling locations outside
(0, 1) are skipped) and the sum over the key points (:242).  Plain torch ops, so torch autograd gives its gradients.
Test infrastructure, CPU or GPU."""
import torch

DEPTH_EPS = 1e-5


def project(key_points, projection_mat, image_wh=None):
    """key_points [b, A, pts, 3], projection_mat [b, cams, 4, 4], image_wh [b, cams, 2] | None
    -> uv [b, A, pts, cams, 2], visible [b, A, pts, cams]."""
    hom = torch.cat([key_points, torch.ones_like(key_points[..., :1])], dim=-1)
    cs = torch.einsum("bcij,bapj->bapci", projection_mat, hom)
    uv = cs[..., 0:2] / cs[..., 2:3].clamp(min=DEPTH_EPS)
    if image_wh is not None:
        uv = uv / image_wh[:, None, None]
    u, v = uv[..., 0], uv[..., 1]
    return uv, (cs[..., 2] > DEPTH_EPS) & (u > 0) & (u < 1) & (v > 0) & (v < 1)


def bilinear(fmap, uv, cell_uv=None):
    """fmap [b, cams, C, h, w], uv [b, N, cams, 2] -> [b, N, cams, C]: bilinear_sampling (cu:13-53) at (v h - 0.5, u w - 0.5),
    zero where the location is outside (0, 1) (cu:166).  ``cell_uv`` (like ``uv``, optional): the locations whose tap cells
    (floor(v h - 0.5), floor(u w - 0.5), in their own dtype) are used -- the discrete choice of a float32 computation, with
    the value and its derivative evaluated at ``uv`` on that cell's bilinear patch."""
    b, cams, C, h, w = fmap.shape
    h_im = uv[..., 1] * h - 0.5
    w_im = uv[..., 0] * w - 0.5
    if cell_uv is None:
        h0, w0 = torch.floor(h_im).detach(), torch.floor(w_im).detach()
    else:
        h0 = torch.floor(cell_uv[..., 1].detach() * h - 0.5).to(uv.dtype)
        w0 = torch.floor(cell_uv[..., 0].detach() * w - 0.5).to(uv.dtype)
    lh, lw = h_im - h0, w_im - w0
    flat = fmap.permute(0, 1, 3, 4, 2).reshape(b, cams, h * w, C)
    out = 0
    for dy, dx, coef in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        py, px = (h0 + dy).long(), (w0 + dx).long()
        ok = (py >= 0) & (py <= h - 1) & (px >= 0) & (px <= w - 1)
        idx = (py.clamp(0, h - 1) * w + px.clamp(0, w - 1))                     # [b, N, cams]
        g = torch.stack([flat[bi][torch.arange(cams)[None, :], idx[bi]] for bi in range(b)])   # [b, N, cams, C]
        out = out + (coef * ok)[..., None] * g
    inside = (uv[..., 0] > 0) & (uv[..., 0] < 1) & (uv[..., 1] > 0) & (uv[..., 1] < 1)
    return out * inside[..., None]


def daf(maps, uv, weights, cell_uv=None):
    """The DAF of the reference: maps = per-level [b, cams, C, h, w], uv [b, N, cams, 2], weights [b, N, cams, L, G]
    -> [b, N, C] (cu:125-187).  ``cell_uv``: see :func:`bilinear`."""
    out = 0
    C = maps[0].shape[2]
    G = weights.shape[-1]
    for l, fmap in enumerate(maps):
        s = bilinear(fmap, uv, cell_uv)                                            # [b, N, cams, C]
        wl = weights[:, :, :, l].repeat_interleave(C // G, dim=-1)        # [b, N, cams, C]
        out = out + (s * wl).sum(dim=2)
    return out


def softmax_weights(visible, raw, weight_mask=None):
    """visible [b, A, pts, cams], raw logits [b, A, cams, L, pts, G], keep-mask like raw | None
    -> weights [b, A, pts, cams, L, G] (:199-221)."""
    x = raw.permute(0, 1, 4, 2, 3, 5)
    mask = visible[..., None, None].expand(x.shape)
    if weight_mask is not None:
        mask = mask & weight_mask.permute(0, 1, 4, 2, 3, 5).bool()
    b, A, pts, cams, L, G = x.shape
    all_miss = mask.sum(dim=(2, 3, 4), keepdim=True) == 0
    x = torch.where(mask, x, torch.full_like(x, -torch.inf))
    x = torch.where(all_miss.expand(x.shape), torch.zeros_like(x), x)
    w = x.reshape(b, A, pts * cams * L, G).softmax(dim=2).reshape(b, A, pts, cams, L, G)
    return w * (~all_miss).to(w.dtype)


def block(key_points, projection_mat, image_wh, maps, raw, weight_mask=None, cell_uv=None):
    """features [b, A, C] of DeformableFeatureAggregation.forward before output_proj (:174-242).  ``cell_uv`` [b, A, pts, cams, 2]
    (optional): the locations whose tap cells are used (:func:`bilinear`)."""
    uv, visible = project(key_points, projection_mat, image_wh)
    w = softmax_weights(visible, raw, weight_mask)
    b, A, pts, cams = visible.shape
    L, G = w.shape[4], w.shape[5]
    cu = None if cell_uv is None else cell_uv.reshape(b, A * pts, cams, 2)
    out = daf(maps, uv.reshape(b, A * pts, cams, 2), w.reshape(b, A * pts, cams, L, G), cu)
    return out.reshape(b, A, pts, -1).sum(dim=2)


# ---- chunked drivers: the same restatement at full size (points in slices, leaf gradients accumulated across slices) ----------

def table_levels(feat, spatial_shape, scale_start):
    """The formatted table ``[b, cams, num_feat, C]`` (DAF.feature_maps_format) as per-level ``[b, cams, C, h, w]`` views, so that
    the restatement's gradient lands in the table's own layout."""
    b, cams, _, C = feat.shape
    out = []
    for (h, w), s in zip(spatial_shape.tolist(), scale_start.tolist()):
        out.append(feat[:, :, s:s + h * w].reshape(b, cams, h, w, C).permute(0, 1, 4, 2, 3))
    return out


def slice_len(cams, C, L, budget=3e9, lo=1024, hi=32768):
    """Points per slice: what autograd keeps of one slice (about 40 gathered [n, cams, C] tensors per level of taps) under
    ``budget`` bytes of float64."""
    return int(max(lo, min(hi, budget // (cams * C * 8 * 10 * L))))


def daf_chunked(feat, spatial_shape, scale_start, loc, weights, grad_out, dtype=torch.float64, chunk=None):
    """DAF.apply's forward and its three gradients by the restatement in ``dtype``: feat [b, cams, num_feat, C], loc
    [b, N, cams, 2], weights [b, N, cams, L, G], grad_out [b, N, C] -> (out [b, N, C], grad_feat, grad_loc, grad_weights)."""
    b, N, cams = loc.shape[:3]
    C, L = feat.shape[3], weights.shape[3]
    chunk = chunk or slice_len(cams, C, L)
    ft = feat.detach().to(dtype).requires_grad_(True)
    out = torch.empty(b, N, C, dtype=dtype, device=feat.device)
    g_loc = torch.empty(loc.shape, dtype=dtype, device=feat.device)
    g_w = torch.empty(weights.shape, dtype=dtype, device=feat.device)
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        uv = loc[:, s:e].detach().to(dtype).requires_grad_(True)
        w = weights[:, s:e].detach().to(dtype).requires_grad_(True)
        o = daf(table_levels(ft, spatial_shape, scale_start), uv, w)
        o.backward(grad_out[:, s:e].to(dtype))
        out[:, s:e], g_loc[:, s:e], g_w[:, s:e] = o.detach(), uv.grad, w.grad
        del o, uv, w
    return out, ft.grad, g_loc, g_w


def block_chunked(key_points, projection_mat, image_wh, feat, spatial_shape, scale_start, grad_out, raw=None, raw_anchor=None,
                  raw_cam=None, weight_mask=None, dtype=torch.float64, chunk=None, cell_uv=None):
    """The fused op (deformable_fused) by the restatement in ``dtype``, anchors in slices: key_points [b, A, pts, 3], feat the
    formatted table, logits ``raw`` [b, A, cams, L, pts, G] or ``raw_anchor`` [b, A, L, pts, G] + ``raw_cam`` [b, cams, L, pts, G],
    grad_out [b, A, C], ``cell_uv`` [b, A, pts, cams, 2] (optional, :func:`bilinear`) -> (out [b, A, C], dict of leaf gradients:
    kp, feat, and raw or ra and rc)."""
    b, A, pts = key_points.shape[:3]
    cams, C, L = feat.shape[1], feat.shape[3], spatial_shape.shape[0]
    step = max(1, (chunk or slice_len(cams, C, L)) // pts)
    cast = lambda t: None if t is None else t.detach().to(dtype)
    pm, wh = cast(projection_mat), cast(image_wh)
    ft = feat.detach().to(dtype).requires_grad_(True)
    rc = None if raw_cam is None else raw_cam.detach().to(dtype).requires_grad_(True)
    out = torch.empty(b, A, C, dtype=dtype, device=feat.device)
    grads = {"kp": torch.empty(key_points.shape, dtype=dtype, device=feat.device)}
    lead = raw if raw is not None else raw_anchor
    grads["raw" if raw is not None else "ra"] = torch.empty(lead.shape, dtype=dtype, device=feat.device)
    for s in range(0, A, step):
        e = min(A, s + step)
        kp = key_points[:, s:e].detach().to(dtype).requires_grad_(True)
        lg = lead[:, s:e].detach().to(dtype).requires_grad_(True)
        x = lg if raw is not None else lg[:, :, None] + rc[:, None]
        wm = None if weight_mask is None else weight_mask[:, s:e]
        cu = None if cell_uv is None else cell_uv[:, s:e]
        o = block(kp, pm, wh, table_levels(ft, spatial_shape, scale_start), x, wm, cu)
        o.backward(grad_out[:, s:e].to(dtype))
        out[:, s:e] = o.detach()
        grads["kp"][:, s:e] = kp.grad
        grads["raw" if raw is not None else "ra"][:, s:e] = lg.grad
        del o, kp, lg, x
    grads["feat"] = ft.grad
    if rc is not None:
        grads["rc"] = rc.grad
    return out, grads


def touched_rows(spatial_shape, scale_start, loc, num_feat, slack=1e-4):
    """[b, cams, num_feat] bool: the table rows some tap of a visible (point, camera) pair lands on (in the map), at any level.
    A tap coordinate within ``slack`` pixels of a cell edge marks the cells on both sides (float32 arithmetic may round it either
    way; the coefficient of the extra row is then ~0)."""
    b, N, cams = loc.shape[:3]
    inside = ((loc > 0) & (loc < 1)).all(-1)                                          # [b, N, cams]
    hit = torch.zeros(b, cams, num_feat, dtype=torch.bool, device=loc.device)
    bi = torch.arange(b, device=loc.device)[:, None, None].expand(b, N, cams)
    ci = torch.arange(cams, device=loc.device)[None, None, :].expand(b, N, cams)
    for (h, w), st in zip(spatial_shape.tolist(), scale_start.tolist()):
        y, x = loc[..., 1].double() * h - 0.5, loc[..., 0].double() * w - 0.5
        for ey in (-slack, slack):
            for ex in (-slack, slack):
                h0, w0 = torch.floor(y + ey).long(), torch.floor(x + ex).long()
                for dy in (0, 1):
                    for dx in (0, 1):
                        py, px = h0 + dy, w0 + dx
                        ok = inside & (py >= 0) & (py < h) & (px >= 0) & (px < w)
                        hit[bi[ok], ci[ok], st + py[ok] * w + px[ok]] = True
    return hit


def visible_pairs(loc):
    """[b, N, cams]: the (point, camera) pairs whose sampling location is inside the strict (0, 1) window."""
    return ((loc > 0) & (loc < 1)).all(-1)


def edge_pairs(loc, ss, slack=None):
    """[b, N, cams]: visible pairs whose tap coordinate ``loc * size - 0.5`` lies on a different side of a cell edge in float32
    arithmetic (fused or not) than in exact arithmetic, at some level -- or, given ``slack`` (locations the kernel computes
    itself, from the key points), within ``slack`` pixels of a cell edge.  The bilinear sample's derivative with respect to its
    location jumps there, so such a pair's location gradient has no float32-resolvable truth."""
    edge = torch.zeros(loc.shape[:3], dtype=torch.bool, device=loc.device)
    for h, w in ss.tolist():
        for v, n in ((loc[..., 1], h), (loc[..., 0], w)):
            exact = v.double() * n - 0.5                                  # exact: a float32 times an integer below 2^11
            if slack is not None:
                edge |= (exact - torch.round(exact)).abs() < slack
                continue
            f = torch.floor(exact)
            edge |= (torch.floor(exact.float()) != f) | (torch.floor(v * n - 0.5) != f)
    return edge & visible_pairs(loc)
