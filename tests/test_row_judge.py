"""The row ops' shared judge (tests/row_judge.py) and kink filter (tests/row_ref.py) against hand-made numbers: two kinds of
two ``[4, 3]`` leaves each, every value a sum of a few powers of two, so that every error, yardstick and bound below is exact in
float64.  A leaf's truth is 0.5 everywhere but one 2.0, and the errors sit on a 0.5: the rule scales by ``max|truth|``, so an
absolute error e is the relative error e / 2.  CPU only."""
import pytest
import torch

import row_ref
from row_judge import EPS32, bound, held, judge_leaves

KEYS = ("a1", "a2", "b1", "b2")
Y_A, Y_B = 2.0 ** -20, 2.0 ** -18          # the kinds' yardsticks: a1's and b1's relative float32 error
OWN_A2 = 2.0 ** -24                        # a2's own float32 error: far below its kind's
FLOOR = 2.0 ** -21                        # 4 eps32


def kind(key):
    return key[0]


def leaf(error=0.0):
    """A truth leaf, moved by the RELATIVE error ``error`` at one element of value 0.5."""
    t = torch.full((4, 3), 0.5, dtype=torch.float64)
    t[0, 0] = 2.0
    t[3, 2] += 2.0 * error
    return t


def results(**native_errors):
    """(native, truth, torch32): the float32 composition has the relative errors Y_A, OWN_A2, Y_B, 0; the native result equals it
    except at the keys given."""
    truth = {k: leaf() for k in KEYS}
    torch32 = {"a1": leaf(Y_A), "a2": leaf(OWN_A2), "b1": leaf(Y_B), "b2": leaf()}
    native = {k: leaf(native_errors[k]) if k in native_errors else torch32[k].clone() for k in KEYS}
    return native, truth, torch32


def judge(native, truth, torch32, **kw):
    return judge_leaves(native, truth, torch32, kind, "hand-made", **kw)


def fails(native, truth, torch32, **kw):
    with pytest.raises(AssertionError) as e:
        judge(native, truth, torch32, **kw)
    return str(e.value)


def test_the_constants():
    assert EPS32 == 2.0 ** -23 and FLOOR == 4 * 2.0 ** -23
    assert bound(Y_A, 1.0) == 2.0 ** -19 + 2.0 ** -21 and bound(2.0 ** -10, leaf()) == 2.0 ** -9 + 2.0 ** -20
    assert bound(0.0, leaf().numpy()) == 2.0 ** -20


def test_the_float32_composition_itself_passes():
    worst = judge(*results())
    assert worst == {"a": Y_A / bound(Y_A, 1.0), "b": Y_B / bound(Y_B, 1.0)}


def test_a_leaf_is_judged_by_its_kind_s_largest_error():
    """a2's own float32 error is 2^-24: alone it would allow 2^-23 + 2^-21.  Its kind's yardstick is a1's 2^-20."""
    limit = 2 * Y_A + FLOOR
    assert limit - 2.0 ** -40 > 2 * OWN_A2 + FLOOR                # its own yardstick would refuse what follows
    worst = judge(*results(a2=limit - 2.0 ** -40))                    # just under 2 Y + 4 eps32
    assert worst["a"] == (limit - 2.0 ** -40) / limit
    judge(*results(a2=limit))                                         # the bound itself is met
    assert "a2" in fails(*results(a2=3 * Y_A + FLOOR))
    assert "b2" in fails(*results(b2=3 * Y_B + FLOOR))
    judge(*results(b2=3 * Y_A + FLOOR))                           # ... which the other kind's yardstick allows


def test_a_zero_truth_needs_exact_zeros():
    native, truth, torch32 = results()
    truth["b2"], torch32["b2"], native["b2"] = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3), torch.zeros(4, 3)
    assert judge(native, truth, torch32)["b"] == Y_B / bound(Y_B, 1.0)
    native["b2"][1, 1] = 1e-30
    assert "b2" in fails(native, truth, torch32)


def test_a_nan_and_a_wrong_shape_fail():
    native, truth, torch32 = results()
    native["a1"][2, 1] = float("nan")
    assert "a1" in fails(native, truth, torch32)
    native, truth, torch32 = results()
    native["b1"] = native["b1"].t().contiguous()
    assert "b1" in fails(native, truth, torch32)


def test_a_per_row_tensor_takes_the_yardstick_passed_in():
    """``max|truth| = 2`` and Y = 2^-10: the bound is 2^-9 + 2^-20, whatever the float32 composition of these rows did."""
    limit = 2.0 ** -9 + 2.0 ** -20
    for torch32_error in (0.0, 1.0):
        native, truth, torch32 = results()
        truth["x"], torch32["x"] = leaf(), leaf(torch32_error)
        native["x"] = leaf((limit - 2.0 ** -40) / 2)                  # leaf() takes a relative error: the absolute one / 2
        worst = judge(native, truth, torch32, per_row=("x", "residual"), row_yardstick={"x": 2.0 ** -10})
        assert worst["x"] == (limit - 2.0 ** -40) / limit and sorted(worst) == ["a", "b", "x"]
        native["x"] = leaf((limit + 2.0 ** -40) / 2)
        assert "x" in fails(native, truth, torch32, per_row=("x",), row_yardstick={"x": 2.0 ** -10})


def test_every_failure_is_in_the_one_message():
    native, truth, torch32 = results(a1=1.0, b2=1.0)
    truth["x"] = torch32["x"] = leaf()
    native["x"] = leaf(1.0)
    native["b1"][0, 1] = float("inf")
    message = fails(native, truth, torch32, per_row=("x",), row_yardstick={"x": 0.0})
    assert all(repr(k) in message for k in ("x", "a1", "b1", "b2")) and repr("a2") not in message


def test_held_takes_torch_and_numpy():
    truth = leaf()
    held("torch", leaf(2.0 ** -12).float(), truth, 2.0 ** -11)
    held("numpy", leaf(2.0 ** -12).numpy(), truth.numpy(), 2.0 ** -11)
    for got in (leaf(2.0 ** -10), leaf()[:3], torch.full((4, 3), float("nan"), dtype=torch.float64)):
        with pytest.raises(AssertionError):
            held("beyond the bound, another shape, not finite", got, truth, 2.0 ** -11)


# ---- the kink filter ------------------------------------------------------------------------------------------------------------

def test_linear_stage():
    x = torch.tensor([[1.0, -2.0], [0.5, 4.0]], dtype=torch.float64)
    W = torch.tensor([[2.0, 1.0], [-4.0, 0.5], [0.0, -1.0]], dtype=torch.float64)
    b = torch.tensor([-1.0, 0.25, 8.0], dtype=torch.float64)
    z, scale = row_ref.linear_stage(x, W, b)
    assert torch.equal(z, torch.tensor([[-1.0, -4.75, 10.0], [4.0, 0.25, 4.0]], dtype=torch.float64))
    assert torch.equal(scale, torch.tensor([[5.0, 5.25, 10.0], [6.0, 4.25, 12.0]], dtype=torch.float64))


def test_kink_filter():
    """Row 0 sits on a kink in one feature of one stage; row 1 is at twice the margin everywhere; row 2 is inside the margin
    only at a stage that no ReLU follows (the refinement MLP's last Linear), which the caller does not pass in."""
    assert row_ref.KINK_MARGIN == 1e-5
    scale = torch.tensor([[3.0, 0.5], [1.0, 7.0], [2.0, 2.0]], dtype=torch.float64)
    twice = 2e-5 * (1.0 + scale)
    relu1, relu2, last = twice.clone(), -twice, twice.clone()
    relu2[0, 1] = 0.0
    last[2, 0] = 0.5e-5 * (1.0 + scale[2, 0])
    assert row_ref.kink_free([(relu1, scale), (relu2, scale)]).tolist() == [False, True, True]
    assert row_ref.kink_free([(relu1, scale), (relu2, scale), (last, scale)]).tolist() == [False, True, False]
    assert row_ref.kink_free([(relu1, scale)]).tolist() == [True, True, True]
