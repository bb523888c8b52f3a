"""TEST INFRASTRUCTURE shared by the row ops' tests: the acceptance rule and the scaffolding of raw library
calls.  Never imported by the product.

The rule.  A float32 result is held to the float64 truth by ``max|native - truth| <= 2 Y + 4 eps32 max|truth|``, Y the error of
the float32 torch composition (what a user of the reference runs today) against the same truth.  A training step's per-row
tensors take Y at the family size (rows are independent, and a small sample must not set its own yardstick); a parameter leaf
is judged relative to its ``max|truth|`` with Y the LARGEST relative float32 error over the leaves of its kind, so that one
lucky 128-value leaf does not set its own yardstick either."""
import ctypes

import numpy as np
import pytest
import torch

from gaussianformer_amd import _lib

EPS32 = float(np.finfo(np.float32).eps)


def _f64(a):
    return (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).double()


def max_error(got, truth):
    """``max|got - truth|`` in float64; torch or numpy."""
    return (_f64(got) - _f64(truth)).abs().max().item()


def bound(yardstick_error, truth):
    """``2 Y + 4 eps32 max|truth|``; ``truth``: a tensor, an array or a number (1.0 for a relative bound)."""
    return 2 * yardstick_error + 4 * EPS32 * _f64(truth).abs().max().item()


def _ratio(err, bound):
    return err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))


def held(what, got, truth, bound):
    """``max|got - truth| <= bound``, the shapes equal, ``got`` finite; prints the error, the bound and their ratio (-s)."""
    assert tuple(got.shape) == tuple(truth.shape), (what, tuple(got.shape), tuple(truth.shape))
    err = max_error(got, truth)
    print(f"{what}: max|native - truth| = {err:.3e}, bound = {bound:.3e}, ratio = {_ratio(err, bound):.3f}")
    assert bool(torch.isfinite(_f64(got)).all()), what
    assert err <= bound, (what, err, bound)


def judge_leaves(native, truth, torch32, kind, what, per_row=(), row_yardstick=None):
    """The training rule on one step's results, each a ``{key: tensor}`` on one device.  A key in ``per_row`` (skipped where the
    truth has none) is held to ``bound(row_yardstick[key], truth)``.  Every other key is a parameter leaf, held relative to its
    ``max|truth|`` to ``2 Y + 4 eps32`` with Y the largest relative error of ``torch32`` over the leaves of ``kind(key)``; where
    the truth is identically 0, so must the native leaf be.  Every leaf must have the truth's shape and be finite.  All
    failures go into one assertion; the worst error / bound per per-row key and per kind is printed (-s) and returned."""
    failed, worst = [], {}

    def sound(k):
        ok = native[k].shape == truth[k].shape and bool(torch.isfinite(native[k]).all())
        if not ok:
            failed.append((k, "shape or non-finite", tuple(native[k].shape), tuple(truth[k].shape)))
        return ok

    def rel(g, k):
        scale = truth[k].abs().max().item()
        return max_error(g[k], truth[k]) / scale if scale > 0 else None

    for k in per_row:
        if k in truth and sound(k):
            err, b = max_error(native[k], truth[k]), bound(row_yardstick[k], truth[k])
            worst[k] = _ratio(err, b)
            print(f"{what} {k}: max|native - truth| = {err:.3e}, bound = {b:.3e}, ratio = {worst[k]:.3f}")
            if not err <= b:
                failed.append((k, err, b))
    leaves = [k for k in truth if k not in per_row]
    yard = {}
    for k in leaves:
        r = rel(torch32, k)
        if r is not None:
            yard[kind(k)] = max(yard.get(kind(k), 0.0), r)
    kinds = {}
    for k in leaves:
        if not sound(k):
            continue
        r = rel(native, k)
        if r is None:
            if not bool((native[k] == 0).all()):
                failed.append((k, "the truth is identically 0, the native leaf is not"))
            continue
        b = bound(yard[kind(k)], 1.0)
        kinds[kind(k)] = max(kinds.get(kind(k), 0.0), r / b)
        if not r <= b:
            failed.append((k, r, b))
    print(f"{what} parameters, worst ratio per kind: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(kinds.items())))
    assert not failed, (what, failed)
    return {**worst, **kinds}


# ---- raw library calls ----------------------------------------------------------------------------------------------------------

@pytest.fixture
def spy(monkeypatch):
    """The names passed to ``_lib.call`` while the test runs, in order."""
    names = []
    real = _lib.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", call)
    return names


def ptr_table(entries, slots=None):
    """A ``void *`` to a table of ``slots`` pointers (default: one per entry): a tensor's ``data_ptr()``, an address as it is,
    ``None`` as NULL; the slots beyond the entries are NULL."""
    table = (ctypes.c_void_p * (len(entries) if slots is None else slots))(*[p.data_ptr() if hasattr(p, "data_ptr") else p for p in entries])
    return ctypes.cast(table, ctypes.c_void_p)


def host_table(buf, slots, drop=(), misalign=None):
    """``ptr_table`` of ``slots`` times the host buffer ``buf``, for refusals that come before any HIP call: the slots in
    ``drop`` NULL, the slot ``misalign`` four bytes in."""
    entries = [buf.data_ptr()] * slots
    for i in drop:
        entries[i] = None
    if misalign is not None:
        entries[misalign] += 4
    return ptr_table(entries)


def _fill(part, value):
    if value is not None:
        (part.view(torch.float32) if isinstance(value, float) else part).fill_(value)


class Guarded:
    """A caller-made buffer of ``nbytes`` with ``guard`` sentinel bytes behind it.  ``sentinel`` and ``body`` (what the caller's
    bytes are prefilled with; ``None``: left as allocated) are a byte value (int) or a float32 value (float)."""

    def __init__(self, nbytes, device, guard, sentinel=0xA5, body=None):
        self.nbytes, self.sentinel = nbytes, sentinel
        self.buf = torch.empty(nbytes + guard, dtype=torch.uint8, device=device)
        _fill(self.buf[:nbytes], body)
        _fill(self.buf[nbytes:], sentinel)

    def floats(self, *shape):
        return self.buf[:self.nbytes].view(torch.float32).view(*shape)

    def intact(self):
        """Nothing was written beyond: every sentinel survived."""
        tail = self.buf[self.nbytes:]
        return bool(((tail.view(torch.float32) if isinstance(self.sentinel, float) else tail) == self.sentinel).all())


TILE_EDGES = (1, 31, 32, 33, 127, 128, 129)      # row counts at the edges of a wave's 32 rows and of a workgroup's 128
ROWS = TILE_EDGES + (1000,)                      # ... and the family size, at which the yardsticks are taken


def edge_rows(B):
    """The tile's edges, the edges of a weight-gradient block of ``B`` rows, three blocks with a ragged tail."""
    return TILE_EDGES + (B - 1, B, B + 1, 2 * B + 76)
