"""TEST INFRASTRUCTURE shared by the row ops' references (the anchor encoder, the feed-forward block, the refinement MLP, the
deformable block's dense ends): the seeded draws, the kink filter and the gradients of the fixed scalar.  CPU only; the per-op
``*_ref.py`` modules restate each op's forward and call this.  Never imported by the product.

The kink filter.  A ReLU whose pre-activation z lies within float32 rounding of 0 can take different sides in float64 and in
float32; that is no error of a float32 kernel, but it moves that row's gradient by about 10 %.  A row is therefore kept iff, at
every Linear in front of a ReLU and every feature, ``|z| >= KINK_MARGIN (1 + sum_k |W_ok x_k| + |b_o|)``, judged in float64 on
the CPU: the margin (about 1e-4 for ordinary rows) is 10-20 times the forwards' measured error of 4-5.5e-6."""
import numpy as np
import torch
import torch.nn.functional as F

NORM_KEYS = ("norm.weight", "norm.bias")   # the post norm's place in a weight mapping (not part of a module's state_dict)
KINK_MARGIN = 1e-5
CANDIDATES = 1400


# ---- seeded draws ---------------------------------------------------------------------------------------------------------------

def _uniform(count, stream):
    """``count`` values in [-1, 1) from an integer hash of (index, stream): exactly reproducible, no generator state."""
    m = np.uint64(0xFFFFFFFF)
    x = (np.arange(count, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(stream) * np.uint64(40503) + np.uint64(12345)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(3266489917)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.float64) / 2.0 ** 31 - 1.0


def fixed_weights(shape_map, stream_offset, seed=0, dtype=torch.float32):
    """A seeded weight mapping away from the initial state for ``{key: shape}``: Linear weights uniform with variance 1 / fan_in,
    biases of +-0.3, LayerNorm weights (the one-dimensional ``*weight`` keys) in [0.7, 1.3] and biases of +-0.3 (computed in
    float64, rounded once to float32, then cast).  ``stream_offset`` keeps the ops' streams apart."""
    sd = {}
    for i, (key, shape) in enumerate(shape_map.items()):
        u = _uniform(int(np.prod(shape)), 1000 * seed + stream_offset + i).reshape(shape)
        if len(shape) == 2:
            v = u * np.sqrt(3.0 / shape[1])
        elif key.endswith("weight"):
            v = 1.0 + 0.3 * u
        else:
            v = 0.3 * u
        sd[key] = torch.from_numpy(v.astype(np.float32)).to(dtype)
    return sd


def cast(sd, dtype=None, device=None):
    return {k: v.to(dtype=dtype, device=device) for k, v in sd.items()}


def module_state(sd):
    """The module's part of a weight mapping (without the post norm's pair): what ``load_state_dict`` takes."""
    return {k: v for k, v in sd.items() if k not in NORM_KEYS}


def fixed_input(n, width, seed):
    """N(0, 1) rows [n, width], float32."""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, width)).astype(np.float32))


def planted(x):
    """Rows that a random draw does not reach (as many as ``x`` has room for): zeros, tiny, +-1e4 in a few columns."""
    x = x.clone()
    plant = [lambda r: r.zero_(), lambda r: r.fill_(1e-30), lambda r: r[3:6].fill_(1e4), lambda r: r[40:43].fill_(-1e4)]
    for i, f in enumerate(plant):
        if i < x.shape[0]:
            f(x[i])
    return x


def output_weights(shape, dtype=torch.float64):
    """The fixed weights of the scalar that gradients come from: cos(0.37 i) over the output's elements."""
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.37).reshape(shape).to(dtype)


# ---- the kink filter ------------------------------------------------------------------------------------------------------------

def linear_stage(x, W, b):
    """``(z, scale)`` of a Linear: its pre-activation and ``scale = sum_k |W_ok x_k| + |b_o|``, the size of the terms z is the sum of."""
    return F.linear(x, W, b), x.abs() @ W.abs().t() + b.abs()


def kink_free(stages):
    """bool [n]: the rows the filter keeps, from the ``(z [n, features], scale)`` of every Linear in front of a ReLU."""
    keep = torch.ones(stages[0][0].shape[0], dtype=torch.bool)
    for z, scale in stages:
        keep &= (z.abs() >= KINK_MARGIN * (1.0 + scale)).all(dim=1)
    return keep


# ---- gradients of the fixed scalar ----------------------------------------------------------------------------------------------

def scalar_gradients(forward, inputs, leaves, cotangent=None, with_out=False):
    """``{input name: d/d input, leaf key: d/d leaf}`` (and ``"out"`` where ``with_out``) of ``sum(forward(*inputs, leaves) *
    cotangent)`` in the inputs' dtype and on their device.  ``inputs``: ``{name: tensor | None}``, passed on in their order as
    fresh leaves (a ``None`` stays ``None`` and gets no gradient); ``cotangent = None``: ``output_weights``."""
    inputs = {k: None if v is None else v.detach().clone().requires_grad_(True) for k, v in inputs.items()}
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
    out = forward(*inputs.values(), leaves)
    if cotangent is None:
        cotangent = output_weights(out.shape, out.dtype).to(out.device)
    wanted = {**{k: v for k, v in inputs.items() if v is not None}, **leaves}
    got = dict(zip(wanted, torch.autograd.grad((out * cotangent).sum(), list(wanted.values()), allow_unused=True)))
    return {"out": out.detach(), **got} if with_out else got
