"""TEST INFRASTRUCTURE: the float64 restatement of the sparse convolution block's training stage,
``y = mask * LN((c + bias) + residual)``, and of the block above it, with the ReLU masks AS GIVEN TENSORS -- a float32 route is
judged against the truth that takes the ReLUs' sides the way that route took them, so a pre-activation within rounding of 0 is
no error.  Built on ``oracle/subm_ref.subm_conv3d_dense``; gradients of the fixed scalar by float64 autograd
(``row_ref.scalar_gradients``).  CPU only; never imported by the product."""
import torch
import torch.nn.functional as F

import row_ref
from oracle.subm_ref import subm_conv3d_dense

EPS = 1e-5


def stage_parts(pre, gamma, beta):
    """``(xhat, u)`` of the LayerNorm: eps 1e-5, biased variance."""
    mean = pre.mean(dim=1, keepdim=True)
    var = ((pre - mean) ** 2).mean(dim=1, keepdim=True)
    xhat = (pre - mean) / torch.sqrt(var + EPS)
    return xhat, xhat * gamma + beta


def stage(c, bias, residual, gamma, beta, mask):
    """``(y, pre, u, xhat)``; ``mask``: the ReLU's 0 / 1 tensor, ``None`` for a stage without a ReLU, ``"own"`` for ``u > 0``."""
    pre = c
    if bias is not None:
        pre = pre + bias
    if residual is not None:
        pre = pre + residual
    xhat, u = stage_parts(pre, gamma, beta)
    if isinstance(mask, str):
        mask = (u > 0).to(u.dtype)
    return (u if mask is None else u * mask), pre, u, xhat


def outside_margin(u, xhat, gamma, beta, m):
    """bool like ``u``: ``|u| >= m (1 + |xhat gamma| + |beta|)`` -- where a float32 evaluation of u, whose error is a tenth of the
    margin's, cannot take the other side of 0."""
    return u.abs() >= m * (1.0 + (xhat * gamma).abs() + beta.abs())


def stage_backward(pre, grad_out, gamma, beta, mask, dtype=torch.float64):
    """``{g_pre, ln_weight, ln_bias, bias}``: the gradients of ``sum(y * grad_out)``, y the stage on the rows ``pre`` (its
    ``bias`` gradient is the column sum of ``g_pre``), by autograd in ``dtype``."""
    t = lambda v: None if v is None or isinstance(v, str) else v.detach().to(dtype)
    pre, gamma, beta = (t(v).requires_grad_(True) for v in (pre, gamma, beta))
    y = stage(pre, None, None, gamma, beta, mask if isinstance(mask, str) else t(mask))[0]
    g_pre, g_gamma, g_beta = torch.autograd.grad((y * t(grad_out)).sum(), [pre, gamma, beta])
    return {"g_pre": g_pre, "ln_weight": g_gamma, "ln_bias": g_beta, "bias": g_pre.sum(0)}


def block_keys(multi, proj):
    """The block's leaves in the restatement's naming: ``conv{s}.weight / .bias``, ``ln{s}.weight / .bias``, ``proj.*``, ``norm.*``."""
    keys = []
    for s in range(3 if multi else 1):
        keys += [f"conv{s}.weight"] + ([f"conv{s}.bias", f"ln{s}.weight", f"ln{s}.bias"] if multi else [])
    return keys + (["proj.weight", "proj.bias"] if proj else []) + ["norm.weight", "norm.bias"]


def block(x, residual, p, idx, batch, shape, K, masks, rep=None, with_stages=False):
    """The block ``norm(output_proj?(stages(x)) + residual?)`` on ``x [b, g, C]``: with ``ln0.weight`` in ``p`` three stages
    ``mask_s * LN(conv_s(.) + bias_s)`` (``masks``: three tensors, or ``"own"``), else the one bias-free convolution; ``rep``:
    the ``duplicates="last"`` source mask ``[N, 1]``.  ``with_stages``: also ``[(pre, u, xhat)]`` of the stages."""
    bs, g = x.shape[:2]
    out, seen = x.flatten(0, 1), []
    src = (lambda t: t * rep) if rep is not None else (lambda t: t)
    if "ln0.weight" in p:
        for s in range(3):
            c = subm_conv3d_dense(src(out), idx, p[f"conv{s}.weight"], batch, shape, K)
            out, pre, u, xhat = stage(c, p[f"conv{s}.bias"], None, p[f"ln{s}.weight"], p[f"ln{s}.bias"], masks if isinstance(masks, str) else masks[s])
            seen.append((pre, u, xhat))
    else:
        out = subm_conv3d_dense(src(out), idx, p["conv0.weight"], batch, shape, K)
    if "proj.weight" in p:
        out = F.linear(out, p["proj.weight"], p["proj.bias"])
    out = out.unflatten(0, (bs, g))
    if residual is not None:
        out = out + residual
    out = F.layer_norm(out, (out.shape[-1],), p["norm.weight"], p["norm.bias"], EPS)
    return (out, seen) if with_stages else out


def block_gradients(x, residual, p, idx, batch, shape, K, masks, rep=None, dtype=torch.float64):
    """``{"x", "residual", leaf key: gradient}`` of the fixed scalar in ``dtype`` on the CPU; the scalar's weights are
    ``row_ref.output_weights`` rounded to float32, the values a float32 route multiplies by."""
    t = lambda v: None if v is None else v.detach().cpu().to(dtype)
    masks = masks if isinstance(masks, str) or masks is None else [t(m) for m in masks]
    fwd = lambda x_, r_, leaves: block(x_, r_, leaves, idx.cpu(), batch, shape, K, masks, t(rep))
    cot = row_ref.output_weights((*x.shape[:2], p["norm.weight"].shape[0]), torch.float32).to(dtype)
    return row_ref.scalar_gradients(fwd, {"x": t(x), "residual": t(residual)}, {k: t(v) for k, v in p.items()}, cotangent=cot)
