"""The three native training steps, bit for bit: the output, every input gradient and every parameter gradient of
``ffn_block_autograd``, ``anchor_embed_autograd`` and ``refine_fused_autograd`` against SHA-256 digests recorded in
tests/golden/train_step_digests.json (tools/make_golden_train_step_digests.py).  The training tests hold the gradients to the
float64 truth; only this one notices a change of the arithmetic that stays inside those bounds (a reordered chain, another
order of the partial sums), which a restructuring of the kernels or of their shared row helpers must not bring.  A digest
needs determinism: ``test_two_calls_agree`` and the ``test_repeatable_...`` tests of the three training files hold that.

The inputs, the weights, the output gradients and the feed-forward block's keep masks come from integer draws alone (numpy's
generator, no torch generator): 24-bit mantissas times powers of two, rows and output gradients of magnitude O(1), weights
O(0.1); a mask keeps an entry where a draw from 0 .. 9 is not 0 (p = 0.1).  Variants, from the existing tests' tables: the
feed-forward block's ``base_norm`` (Cin 256, pre norm, identity) and ``prob_add_norm`` (Cin 128, residual), both masked; the
anchor encoder's ``opa_s17`` and ``noopa_s0``; the refinement MLP's ``solid``, ``prob`` and ``D43``.  Rows:
    1        a tile of one live lane
    33       a second wave with one row
    129      a second tile with one row
    513      a second weight-gradient block of one row: the sum kernel's count == 2 tail, the flush loop's short last chain
    1100     2 * 512 + 76: three blocks, the four-way interleave's remainder path
    chunk rows + 1 on one variant per op (32 769, 65 537 for the anchor encoder): a second chunk of one row."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import anchor_embed_ref
import ffn_ref
from gaussianformer_amd import _lib
from anchor_embed_ref import LAYOUTS as ANCHOR_FAMILIES
from ffn_ref import VARIANTS as FFN_VARIANTS, parts
from refine_ref import VARIANTS as REFINE_VARIANTS, make_module, outputs_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_step_digests.json")
ROWS = (1, 33, 129, 513, 1100)
P = 0.1
OPS = {   # op: (variants, the one that also runs at chunk rows + 1, chunk rows)
    "ffn": (("base_norm", "prob_add_norm"), "base_norm", _lib.GF_FFN_CHUNK_ROWS),
    "anchor": (("opa_s17", "noopa_s0"), "opa_s17", _lib.GF_ANCHOR_EMBED_CHUNK_ROWS),
    "refine": (("solid", "prob", "D43"), "solid", _lib.GF_REFINE_MLP_CHUNK_ROWS),
}
CASES = [(op, v, n) for op, (variants, big, chunk) in OPS.items() for v in variants for n in ROWS + ((chunk + 1,) if v == big else ())]
assert [_lib.GF_FFN_WGRAD_ROWS, _lib.GF_ANCHOR_EMBED_WGRAD_ROWS, _lib.GF_REFINE_MLP_WGRAD_ROWS] == [512] * 3   # what ROWS is cut for


def case_name(op, variant, n):
    return f"{op}.{variant}.n{n}"


def _draw(rng, shape, lo, hi):
    """24-bit mantissas times 2^e, e in [lo, hi), as float32 (exact) on the host."""
    v = rng.integers(-2 ** 23, 2 ** 23, shape) * 2.0 ** rng.integers(lo, hi, shape)
    return torch.from_numpy(v.astype(np.float32))


def _rows(rng, n, width):
    return _draw(rng, (n, width), -25, -22)       # |x| < 2


def _weights(rng, shapes):
    return {k: _draw(rng, tuple(s), -29, -25) for k, s in shapes.items()}     # |w| < 1 / 4


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _step(forward, inputs, params, rng):
    """``{name: digest}`` of one forward and backward: ``forward(inputs, params) -> {name: output}`` on leaves that require grad,
    the output gradients drawn here, every tensor checked finite (a NaN's payload is nobody's arithmetic)."""
    inputs = {k: v.clone().requires_grad_(True) for k, v in inputs.items()}
    params = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    outs = {k: v for k, v in forward(inputs, params).items() if v.numel()}
    gouts = [_rows(rng, *v.shape).to(v.device) for v in outs.values()]
    leaves = {**{"grad." + k: v for k, v in inputs.items()}, **{"grad." + k: v for k, v in params.items()}}
    grads = torch.autograd.grad(list(outs.values()), list(leaves.values()), gouts)
    result = {**{"out." + k: v for k, v in outs.items()}, **dict(zip(leaves, grads))}
    for k, v in result.items():
        assert bool(torch.isfinite(v).all()), k
    return {k: _digest(v) for k, v in result.items()}


def compute(op, variant, n):
    """The digests of one case on the GPU."""
    from gaussianformer_amd.anchor_encoder import anchor_embed_autograd
    from gaussianformer_amd.ffn import ffn_block_autograd
    from gaussianformer_amd.refine import refine_fused_autograd
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    if op == "ffn":
        cin, pre, ident, has_res, norm = FFN_VARIANTS[variant]
        params = _weights(rng, ffn_ref.shapes(cin, pre, ident, norm))
        inputs = {"x": _rows(rng, n, cin)}
        if has_res:
            inputs["residual"] = _rows(rng, n, 128)
        kh = torch.from_numpy((rng.integers(0, 10, (n, 512)) != 0).astype(np.uint8)).to(dev)
        ko = torch.from_numpy((rng.integers(0, 10, (n, 128)) != 0).astype(np.uint8)).to(dev)

        def forward(i, p):
            module, post = parts(p)
            return {"out": ffn_block_autograd(i["x"], module, norm=post, residual=i.get("residual"), p_hidden=P, p_out=P,
                                              keep_hidden=kh, keep_out=ko)}
    elif op == "anchor":
        opa, S, Da = ANCHOR_FAMILIES[variant]
        params = _weights(rng, anchor_embed_ref.shapes(bool(opa), S))
        inputs = {"anchor": _rows(rng, n, Da)}

        def forward(i, p):
            return {"out": anchor_embed_autograd(i["anchor"], p)}
    else:
        cfg, extra = REFINE_VARIANTS[variant]
        module = make_module(cfg, 0)       # its structure and configuration; every value is drawn below
        rcfg, D = module._cfg, module.output_dim
        params = _weights(rng, {k: v.shape for k, v in module.named_parameters()})
        inputs = {"instance_feature": _rows(rng, n, 128), "anchor": _rows(rng, n, D + extra), "anchor_embed": _rows(rng, n, 128)}

        def forward(i, p):
            return outputs_of(*refine_fused_autograd(i["instance_feature"], i["anchor"], i["anchor_embed"], p, rcfg))
    return _step(forward, {k: v.to(dev) for k, v in inputs.items()}, {k: v.to(dev) for k, v in params.items()}, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("op,variant,n", CASES, ids=[case_name(*c) for c in CASES])
def test_training_step_bits_are_the_recorded_ones(gpu, op, variant, n):
    got = compute(op, variant, n)
    with open(GOLDEN) as f:
        want = json.load(f)[case_name(op, variant, n)]
    assert sorted(got) == sorted(want)
    differ = [k for k in got if got[k] != want[k]]
    assert not differ, (f"{case_name(op, variant, n)}: the bits of {differ} are not the recorded ones.  The training step's arithmetic changed.  "
                        "Regenerate tests/golden/train_step_digests.json (tools/make_golden_train_step_digests.py) ONLY if that change is intended.")
