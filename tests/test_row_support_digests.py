"""The row ops' seeded draws and kink-filter survivors, bit for bit: SHA-256 digests of what tests/row_ref.py and the per-op
``*_ref.py`` modules hand the anchor encoder's, the feed-forward block's, the refinement MLP's and the deformable block's tests,
against tests/golden/row_support_digests.json (tools/make_golden_row_support_digests.py).  Every bound those tests print
follows from these values, so a change of the shared helpers that moves one bit of a weight, an input, a mask or the set of
surviving rows shows here, on the CPU, and not as a shifted ratio on the GPU.  The anchor encoder's eight layouts are all
recorded (the training tests use every one of them)."""
import hashlib
import json
import os

import numpy as np
import pytest

import anchor_embed_ref
import anchor_embed_train_ref
import deform_block_ref
import ffn_ref
import ffn_train_ref
import refine_mlp_train_ref
import row_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_support_digests.json")


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.numpy() if hasattr(t, "numpy") else t).tobytes())
    return h.hexdigest()


def _keep(keep):
    return _digest(np.packbits(keep.numpy()))


def compute():
    """``{name: digest}``; a mapping of weights is hashed as its tensors' bytes in key order."""
    out = {}
    for name, (opa, S, _) in anchor_embed_ref.LAYOUTS.items():
        out[f"weights.anchor.{name}"] = _digest(*anchor_embed_ref.fixed_weights(bool(opa), S, seed=0).values())
        out[f"keep.anchor.{name}"] = _keep(anchor_embed_train_ref.candidates(name)[1])
    for name, (cin, pre, ident, _, norm) in ffn_ref.VARIANTS.items():
        out[f"weights.ffn.{name}"] = _digest(*ffn_ref.fixed_weights(cin, pre, ident, norm, seed=0).values())
        out[f"keep.ffn.{name}"] = _keep(ffn_train_ref.candidates(cin, pre, ident, norm)[1])
    for name in refine_mlp_train_ref.VARIANTS:
        out[f"keep.refine.{name}"] = _keep(refine_mlp_train_ref.candidates(name)[4])
    for name, shapes in (("module", deform_block_ref.shapes(deform_block_ref.FIXTURE_CONFIG, norm=True)),
                         ("dense", deform_block_ref.dense_shapes(6, 144, norm=True))):
        out[f"weights.deform.{name}"] = _digest(*deform_block_ref.fixed_weights(shapes, seed=0).values())
    x = row_ref.fixed_input(8, 16, 3)
    out["fixed_input(8, 16, 3)"] = _digest(x)
    out["planted(fixed_input(8, 16, 3))"] = _digest(row_ref.planted(x))
    out["output_weights((4, 8))"] = _digest(row_ref.output_weights((4, 8)))
    kh, ko, scale = ffn_train_ref.masks(8, 0.1, 0)
    out["masks(8, 0.1, 0)"] = _digest(kh, ko, np.float64(scale))
    return out


@pytest.fixture(scope="module")
def computed():
    return compute()


def test_every_recorded_digest_is_computed(computed):
    with open(GOLDEN) as f:
        assert sorted(json.load(f)) == sorted(computed)


def test_draws_and_survivors_are_the_recorded_ones(computed):
    with open(GOLDEN) as f:
        want = json.load(f)
    differ = [k for k in want if computed.get(k) != want[k]]
    assert not differ, (f"the bits of {differ} are not the recorded ones: a seeded draw or the kink filter changed, and with it every bound "
                        "the row ops' tests print.  Regenerate tests/golden/row_support_digests.json ONLY if that change is intended.")
