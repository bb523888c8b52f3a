"""TEST INFRASTRUCTURE for the feed-forward block's training step: ``ffn_ref``'s block with the module's two dropouts as given
keep masks and scales, in a generic dtype; the kink filter on the hidden layer's pre-activations; seeded masks; and the
gradients of the fixed scalar ``sum(out * output_weights)``.

The kink filter is tests/row_ref.py's, on the hidden layer's 512 pre-activations (``layers.0.0``, the only Linear in front of
a ReLU).  Never imported by the product."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import ffn_ref as ref
import row_ref
from row_ref import CANDIDATES, output_weights  # noqa: F401  (output_weights is re-exported)

E, HIDDEN = ref.E, ref.HIDDEN


def ffn_train_ref(x, sd, residual=None, keep_hidden=None, scale_hidden=1.0, keep_out=None, scale_out=1.0, norm=True):
    """The block in ``x``'s dtype on the mapping ``sd``: ``ffn_ref`` with ``h' = h * keep_hidden * scale_hidden`` behind the ReLU
    and ``a' = (W2 h' + b2) * keep_out * scale_out`` behind ``layers.1`` (a ``None`` mask: no dropout there)."""
    u = x
    if "pre_norm.weight" in sd:
        u = F.layer_norm(x, (x.shape[-1],), sd["pre_norm.weight"], sd["pre_norm.bias"], 1e-5)
    h = F.relu(F.linear(u, sd["layers.0.0.weight"], sd["layers.0.0.bias"]))
    if keep_hidden is not None:
        h = h * (keep_hidden != 0).to(x.dtype) * scale_hidden
    y = F.linear(h, sd["layers.1.weight"], sd["layers.1.bias"])
    if keep_out is not None:
        y = y * (keep_out != 0).to(x.dtype) * scale_out
    if "identity_fc.weight" in sd:
        y = F.linear(u, sd["identity_fc.weight"], sd["identity_fc.bias"]) + y
    if residual is not None:
        y = y + residual
    if norm and "norm.weight" in sd:
        y = F.layer_norm(y, (y.shape[-1],), sd["norm.weight"], sd["norm.bias"], 1e-5)
    return y


def relu_stages(x, sd):
    """The ``(z, scale)`` the kink filter judges the rows of ``x`` (float32 values) by: in float64, on the CPU."""
    with torch.no_grad():
        sd = ref.cast(sd, torch.float64, "cpu")
        u = x.double().cpu()
        if "pre_norm.weight" in sd:
            u = F.layer_norm(u, (u.shape[-1],), sd["pre_norm.weight"], sd["pre_norm.bias"], 1e-5)
        return [row_ref.linear_stage(u, sd["layers.0.0.weight"], sd["layers.0.0.bias"])]


@functools.lru_cache(maxsize=None)
def candidates(cin, pre_norm, identity, norm=True, seed=0, count=CANDIDATES, dead=False):
    """``(x [count, cin] float32, keep bool [count], sd)``: candidate rows ``fixed_input(count, cin, 100 + seed)``, which of them
    the filter keeps, and the weights ``fixed_weights(seed)`` (``dead``: the first layer's bias at -1e6, the hidden row all 0)."""
    sd = ref.fixed_weights(cin, pre_norm, identity, norm, seed=seed)
    if dead:
        sd["layers.0.0.bias"] = torch.full_like(sd["layers.0.0.bias"], -1e6)
    x = ref.fixed_input(count, cin, 100 + seed)
    return x, row_ref.kink_free(relu_stages(x, sd)), sd


def survivors(cin, pre_norm, identity, norm=True, seed=0, count=CANDIDATES, dead=False):
    """``(rows [m, cin] float32 on the CPU, sd)``: the candidates the filter keeps, in their order."""
    x, keep, sd = candidates(cin, pre_norm, identity, norm, seed, count, dead)
    return x[keep].contiguous(), sd


def masks(n, p, seed, device="cpu"):
    """``(keep_hidden u8 [n, 512], keep_out u8 [n, 128], scale)``: seeded Bernoulli(1 - p) keep masks (a row's bits do not depend
    on n) and the scale ``1 / (1 - p)`` both dropouts use."""
    rng = np.random.default_rng(1000 + seed)
    draw = rng.random((n, HIDDEN + E)) >= p
    kh = torch.from_numpy(draw[:, :HIDDEN].astype(np.uint8)).contiguous().to(device)
    ko = torch.from_numpy(draw[:, HIDDEN:].astype(np.uint8)).contiguous().to(device)
    return kh, ko, 1.0 / (1.0 - p)


def kind(key):
    """The kind of a leaf, for the parameter gradients' yardsticks: by how its gradient is formed.  A "matrix" (a Linear
    weight) is a contraction over the rows; a "vector" (a Linear bias, a LayerNorm weight or bias) is a plain sum over the rows
    of a per-row quantity.  The block has at most two leaves of each finer kind and, without one of the norms, a single one --
    a kind of one leaf would be that leaf's own yardstick, which the rule (the largest error over a kind) exists to avoid."""
    return "matrix" if key.endswith("weight") and "norm" not in key else "vector"
