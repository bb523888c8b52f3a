"""``_lib.ParamSlots``: how a training Function carries its parameter list across ``save_for_backward``.
The carrier alone, on CPU tensors: it builds pointer tables and buffers and never calls the library."""
import ctypes

import pytest
import torch

from gaussianformer_amd import _lib

COUNT = 6     # the table is longer than the list: the slots behind it stay NULL


def entries(table, count=COUNT):
    """The pointers of a host table as ints (0 for NULL)."""
    return [p or 0 for p in (ctypes.c_void_p * count).from_address(table.value)]


def params():
    """``[fp32, None, float64, None, non-contiguous, one float into a larger buffer]``"""
    plain = torch.arange(12.0).reshape(3, 4)
    double = torch.arange(4.0, dtype=torch.float64)
    strided = torch.arange(12.0).reshape(4, 3).t()
    shifted = torch.arange(9.0)[1:]
    assert not strided.is_contiguous() and shifted.data_ptr() % 16 == 4 and plain.data_ptr() % 16 == 0
    return [plain, None, double, None, strided, shifted]


def test_none_slots_survive_the_round_trip():
    ps = params()
    slots, table, held = _lib.ParamSlots.pack(ps, COUNT)
    assert len(held) == 4 and all(isinstance(t, torch.Tensor) for t in held)
    assert not any(isinstance(v, torch.Tensor) for v in vars(slots).values())       # the record goes on ctx: no tensor in it
    assert slots.dtypes == [torch.float32, None, torch.float64, None, torch.float32, torch.float32]
    back, _ = slots.unpack(tuple(held))
    assert [p is None for p in back] == [p is None for p in ps]
    assert all(b is h for b, h in zip([p for p in back if p is not None], held))    # nothing to convert a second time


def test_a_parameter_the_library_cannot_read_is_held_as_a_copy_the_table_points_at():
    ps = params()
    slots, table, held = _lib.ParamSlots.pack(ps, COUNT)
    ptrs = entries(table)
    assert held[0] is ps[0] and ptrs[0] == ps[0].data_ptr()                         # a parameter as it is
    for i, h in zip((2, 4, 5), held[1:]):
        assert h is not ps[i] and h.data_ptr() != ps[i].data_ptr()
        assert h.dtype == torch.float32 and h.is_contiguous() and h.data_ptr() % 16 == 0
        assert torch.equal(h, ps[i].float()) and ptrs[i] == h.data_ptr()
    assert ptrs[1] == 0 and ptrs[3] == 0


def test_the_rebuilt_table_equals_the_forward_s_on_the_same_tensors():
    slots, table, held = _lib.ParamSlots.pack(params(), COUNT)
    back, again = slots.unpack(held)
    assert entries(again) == entries(table) and again is not table
    # other storage handed back (a saved-tensor hook): the table follows it, and a copy made for it stays alive in the list
    moved = [h.clone() for h in held[:3]] + [torch.cat([torch.zeros(1), held[3]])[1:]]
    back, again = slots.unpack(moved)
    kept = [p for p in back if p is not None]
    assert [p.data_ptr() for p in kept[:3]] == [m.data_ptr() for m in moved[:3]] and kept[3].data_ptr() % 16 == 0
    assert entries(again) == [0 if p is None else p.data_ptr() for p in back]
    assert all(torch.equal(k, h) for k, h in zip(kept, held))


def test_the_carrier_reaches_the_tables_through_the_module(monkeypatch):
    seen = []
    real_in, real_out = _lib.param_table, _lib.out_table
    monkeypatch.setattr(_lib, "param_table", lambda ps, count: seen.append(("in", count)) or real_in(ps, count))
    monkeypatch.setattr(_lib, "out_table", lambda ts, count: seen.append(("out", count)) or real_out(ts, count))
    slots, table, held = _lib.ParamSlots.pack(params(), COUNT)
    back, _ = slots.unpack(held)
    slots.grad_buffers(back, [True] * len(back))
    assert seen == [("in", COUNT), ("in", COUNT), ("out", COUNT)]


def test_the_wanted_list_selects_the_buffers():
    slots, table, held = _lib.ParamSlots.pack(params(), COUNT)
    back, _ = slots.unpack(held)
    every, gtable = slots.grad_buffers(back, [True] * 6)
    assert [g is not None for g in every] == [True, False, True, False, True, True]      # an absent slot has none to want
    assert entries(gtable) == [0 if g is None else g.data_ptr() for g in every]
    some, gtable = slots.grad_buffers(back, [True, True, False, False, False, True])
    assert [g is not None for g in some] == [True, False, False, False, False, True]
    assert entries(gtable) == [0 if g is None else g.data_ptr() for g in some]
    for g, p in zip(every, back):
        if g is not None:
            assert g.shape == p.shape and g.dtype == torch.float32 and g.is_contiguous() and g.data_ptr() != p.data_ptr()


def test_the_return_tuple_has_each_slot_s_dtype_and_none_where_not_needed():
    ps = params()
    slots, table, held = _lib.ParamSlots.pack(ps, COUNT)
    back, _ = slots.unpack(held)
    grads, _ = slots.grad_buffers(back, [True] * 6)
    for g in grads:
        if g is not None:
            g.copy_(torch.arange(float(g.numel())).reshape(g.shape) + 0.5)
    out = slots.returned(grads, [True, True, True, False, False, True])
    assert isinstance(out, tuple) and [g is not None for g in out] == [True, False, True, False, False, True]
    assert [g.dtype for g in out if g is not None] == [torch.float32, torch.float64, torch.float32]
    assert all(g.shape == p.shape for g, p in zip(out, ps) if g is not None)
    assert out[0] is grads[0] and torch.equal(out[2], grads[2].double())                  # cast only where the dtype differs
    # a buffer the op did not ask for stays None even where autograd would take a gradient
    some, _ = slots.grad_buffers(back, [True, False, False, False, False, False])
    assert [g is not None for g in slots.returned(some, [True] * 6)] == [True] + [False] * 5


@pytest.mark.parametrize("bad", [torch.zeros(4, dtype=torch.float64), torch.zeros(4, 3).t(), torch.zeros(9)[1:]],
                         ids=["float64", "non-contiguous", "misaligned"])
def test_out_table_still_refuses_a_buffer_the_library_cannot_write(bad):
    with pytest.raises(ValueError, match="a gradient buffer must be a contiguous, 16-byte aligned float32 tensor"):
        _lib.out_table([torch.zeros(4), None, bad], COUNT)
