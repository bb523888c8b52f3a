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


def bilinear(fmap, uv):
    """fmap [b, cams, C, h, w], uv [b, N, cams, 2] -> [b, N, cams, C]: bilinear_sampling (cu:13-53) at (v h - 0.5, u w - 0.5),
    zero where the location is outside (0, 1) (cu:166)."""
    b, cams, C, h, w = fmap.shape
    h_im = uv[..., 1] * h - 0.5
    w_im = uv[..., 0] * w - 0.5
    h0, w0 = torch.floor(h_im).detach(), torch.floor(w_im).detach()
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


def daf(maps, uv, weights):
    """The DAF of the reference: maps = per-level [b, cams, C, h, w], uv [b, N, cams, 2], weights [b, N, cams, L, G]
    -> [b, N, C] (cu:125-187)."""
    out = 0
    C = maps[0].shape[2]
    G = weights.shape[-1]
    for l, fmap in enumerate(maps):
        s = bilinear(fmap, uv)                                            # [b, N, cams, C]
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


def block(key_points, projection_mat, image_wh, maps, raw, weight_mask=None):
    """features [b, A, C] of DeformableFeatureAggregation.forward before output_proj (:174-242)."""
    uv, visible = project(key_points, projection_mat, image_wh)
    w = softmax_weights(visible, raw, weight_mask)
    b, A, pts, cams = visible.shape
    L, G = w.shape[4], w.shape[5]
    out = daf(maps, uv.reshape(b, A * pts, cams, 2), w.reshape(b, A * pts, cams, L, G))
    return out.reshape(b, A, pts, -1).sum(dim=2)
