"""The feed-forward block on the GPU: ``gf_ffn_forward``, ``ffn_block`` and the drop-in ``AsymmetricFFN`` above it.

Values.  The truth is the float64 restatement (tests/ffn_ref.py) on the same inputs and weights.  Per case
``max|native - truth| <= 2 Y + 4 eps32 max|truth|`` with ``Y = max|float32 torch composition on this GPU - truth|`` taken at the
variant's n = 1 000 case (the project's rule: test_anchor_encoder_gpu.py, test_refine_gpu.py).  Every n of a variant is a
prefix of the variant's 1 000 rows, so one truth and one yardstick per variant serve all its cases.  The measured
``max|native - truth| / bound`` per variant is printed (-s) and recorded in DESIGN.md §3.13c.

Invariants are bitwise.  Nothing here reads past an input's end or inspects code."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ffn_ref as ref
from ffn_ref import VARIANTS, parts
from gaussianformer_amd import _lib, ffn as ffn_mod
from gaussianformer_amd.ffn import AsymmetricFFN, ffn_block
from row_judge import ROWS, TILE_EDGES, bound, held, max_error, ptr_table, spy  # noqa: F401  (spy is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ffn.npz")

N_VARIANT = 1000


class Case:
    """A variant's weights, its 1 000 rows, the float64 truth, the float32 torch composition and the native result of those."""

    def __init__(self, name, seed=0, dead=False):
        self.cin, pre, ident, self.has_res, norm = VARIANTS[name]
        sd = ref.fixed_weights(self.cin, pre, ident, norm, seed=seed)
        if dead:   # a first-layer bias that drives the whole hidden row to 0, whatever the input
            sd["layers.0.0.bias"] = torch.full_like(sd["layers.0.0.bias"], -1e6)
        self.sd = ref.cast(sd, device=DEV)
        self.sd64 = ref.cast(sd, torch.float64, DEV)
        self.x = ref.planted(ref.fixed_input(N_VARIANT, self.cin, 7 + seed)).to(DEV)
        self.res = self.x.clone() if self.has_res else None     # "add" of the block's input (Cin = 128 = E)
        with torch.no_grad():
            self.truth = ref.ffn_ref(self.x.double(), self.sd64, None if self.res is None else self.res.double())
            self.torch32 = ref.ffn_ref(self.x, self.sd, self.res)
            self.native = self.run(self.x, self.res)
        self.Y = max_error(self.torch32, self.truth)
        self.bound = bound(self.Y, self.truth)

    def run(self, x, res=None, sd=None):
        module, norm = parts(self.sd if sd is None else sd)
        with torch.no_grad():
            return ffn_block(x, module, norm=norm, residual=res)


@functools.lru_cache(maxsize=None)
def case(name, dead=False):
    return Case(name, dead=dead)


def raw_call(x, sd, out, res=None, n=None, cin=None, F_=512, E=128):
    """The C entry point on caller-made buffers (``sd``: a weight mapping on the GPU)."""
    module, norm = parts(sd)
    _lib.call("gf_ffn_forward", x.device, x.shape[0] if n is None else n, x.shape[1] if cin is None else cin, F_, E,
              x, ptr_table(ffn_mod._param_list(module, norm), 10), res, out)
    return out


# ---- 1. values ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", list(VARIANTS))
def test_values(name, n):
    c = case(name)
    got = c.native if n == N_VARIANT else c.run(c.x[:n].contiguous(), None if c.res is None else c.res[:n].contiguous())
    held(f"{name} n={n}", got, c.truth[:n], c.bound)


def test_values_many_tiles():
    """n = 40 000: 313 workgroups of 128 rows, more than the chip holds at once."""
    c = case("base_norm")
    x = ref.fixed_input(40000, c.cin, 99).to(DEV)
    with torch.no_grad():
        held("base_norm n=40000", c.run(x), ref.ffn_ref(x.double(), c.sd64), c.bound)


def big_rows():
    """The least multiple of 128 rows that the tile kernel takes (the 32-row kernel runs while n <= 32 x the CU count), plus a tile."""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    return (32 * cus + 127) // 128 * 128 + 128


@functools.lru_cache(maxsize=None)
def big_case(name):
    """The variant on big_rows() + 129 rows, whose first 1 000 are the variant's own: input, residual, truth, native result."""
    c = case(name)
    x = torch.cat([c.x, ref.fixed_input(big_rows() + 129 - N_VARIANT, c.cin, 98).to(DEV)])
    res = x.clone() if c.has_res else None
    with torch.no_grad():
        truth = ref.ffn_ref(x.double(), c.sd64, None if res is None else res.double())
    return x, res, truth, c.run(x, res)


@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_the_two_kernels_give_the_same_bits(name):
    """Up to 32 rows per CU a workgroup owns 32 rows and its waves split the features; beyond, a workgroup owns 128 rows.  Which
    one runs is a matter of speed: the variant's 1 000 rows alone (the first) and as a prefix of many (the second) agree bitwise."""
    c = case(name)
    x, res, truth, native = big_case(name)
    held(f"{name} n={x.shape[0]}", native, truth, c.bound)
    assert torch.equal(native[:N_VARIANT], c.native)


@pytest.mark.parametrize("r", TILE_EDGES)
@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_tile_kernel_at_its_edges(name, r):
    """The 128-row kernel with r rows in its last tile: the values, the prefix, and nothing written beyond row n."""
    c = case(name)
    x, res, truth, native = big_case(name)
    n = big_rows() + r
    out = torch.full((n + 200, 128), 12345.0, device=DEV)
    raw_call(x, c.sd, out, res=res, n=n)
    assert torch.equal(out[:n], native[:n])
    assert bool((out[n:] == 12345.0).all())
    held(f"{name} n={n}", out[:n], truth[:n], c.bound)


def test_values_leading_shape():
    c = case("prob_add_norm")
    got = c.run(c.x.view(2, 500, c.cin), c.res.view(2, 500, 128))
    assert got.shape == (2, 500, 128)
    assert torch.equal(got.view(1000, 128), c.native)
    held("prob_add_norm [2, 500, Cin]", got.view(1000, 128), c.truth, c.bound)
    b = case("base_norm")
    assert torch.equal(b.run(b.x.view(2, 500, b.cin)).view(1000, 128), b.native)


def test_zero_row_gives_the_pre_norm_s_bias():
    """Row 0 is all zeros: LN_pre of a constant row is its bias exactly, so the row's result is the block on that bias --
    in the truth and here."""
    c = case("base_norm")
    sd64 = dict(c.sd64)
    u = sd64.pop("pre_norm.bias")[None]
    sd64.pop("pre_norm.weight")
    with torch.no_grad():
        truth = ref.ffn_ref(u, sd64)
    held("zero row against the bias form", c.native[:1], truth, c.bound)


@pytest.mark.parametrize("name", ["base_norm", "prob"])
def test_dead_hidden_layer(name):
    """``layers.0.0.bias = -1e6``: the hidden row is 0 in every feature, the result is ``b2 + identity`` (+ residual, norm) and no
    longer depends on ``layers.0.0.weight``, bitwise."""
    c = case(name, dead=True)
    held(f"dead hidden {name}", c.native, c.truth, c.bound)
    sd = dict(c.sd)
    sd["layers.0.0.weight"] = torch.randn(sd["layers.0.0.weight"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    assert torch.equal(c.run(c.x, c.res, sd), c.native)
    with torch.no_grad():   # the truth from b2 + identity alone
        s64 = c.sd64
        u = F.layer_norm(c.x.double(), (c.cin,), s64["pre_norm.weight"], s64["pre_norm.bias"], 1e-5) if "pre_norm.weight" in s64 else c.x.double()
        y = s64["layers.1.bias"].expand(N_VARIANT, 128)
        if "identity_fc.weight" in s64:
            y = F.linear(u, s64["identity_fc.weight"], s64["identity_fc.bias"]) + y
        if "norm.weight" in s64:
            y = F.layer_norm(y, (128,), s64["norm.weight"], s64["norm.bias"], 1e-5)
    held(f"dead hidden {name} against b2 + identity", c.native, y, c.bound)


@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_module_with_the_fixture_s_weights(name):
    """The drop-in on the reference's recorded input: held to the recorded float64 outputs, the recorded float32 outputs (the
    reference's own, on the CPU) as the yardstick -- the FFN alone through the module, the block through ``ffn_block``."""
    g = np.load(GOLDEN)
    shapes = ref.family_shapes(name)
    weights = ref.fixed_weights(shapes["layers.0.0.weight"][1], "pre_norm.weight" in shapes, "identity_fc.weight" in shapes, seed=int(g[name + ".seed"]))
    module = AsymmetricFFN(**ref.FAMILIES[name])
    module.load_state_dict(ref.module_state(weights), strict=True)
    module.to(DEV).eval()
    norm = torch.nn.LayerNorm(128)
    norm.load_state_dict({"weight": weights["norm.weight"], "bias": weights["norm.bias"]})
    norm.to(DEV)
    x = torch.from_numpy(g[name + ".input"]).to(DEV)

    def recorded(key):
        t = g[f"{name}.{key}64"]
        return bound(max_error(g[f"{name}.{key}32"], t), t)
    with torch.no_grad():
        held(f"fixture {name} ffn", module(x), torch.from_numpy(g[name + ".ffn64"]).to(DEV), recorded("ffn"))
        block = ffn_block(x, module, norm=norm, residual=x if ref.FOLLOWED_BY_ADD[name] else None)
        held(f"fixture {name} block", block, torch.from_numpy(g[name + ".block64"]).to(DEV), recorded("block"))


# ---- 2. invariants, bitwise -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_two_calls_agree(name):
    c = case(name)
    assert torch.equal(c.run(c.x, c.res), c.native)


@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_permutation_of_rows(name):
    c = case(name)
    perm = torch.randperm(N_VARIANT, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    assert torch.equal(c.run(c.x[perm], None if c.res is None else c.res[perm]), c.native[perm])


@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_rows_do_not_depend_on_n(name):
    c = case(name)
    assert torch.equal(c.run(c.x[:129].contiguous(), None if c.res is None else c.res[:129].contiguous()), c.native[:129])


@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_nothing_is_written_beyond_row_n(name):
    c = case(name)
    for n in (1, 33, 129):
        out = torch.full((n + 200, 128), 12345.0, device=DEV)
        raw_call(c.x, c.sd, out, res=c.res, n=n)
        assert torch.equal(out[:n], c.native[:n])
        assert bool((out[n:] == 12345.0).all())


@pytest.mark.parametrize("col", [0, 100, 255])
@pytest.mark.parametrize("name", ["base_norm", "c256_nopre_id", "prob_add_norm"])
def test_a_nan_stays_in_its_row(name, col):
    c = case(name)
    x = c.x.clone()
    x[77, col % c.cin] = float("nan")
    got = c.run(x, x.clone() if c.has_res else None)
    assert bool(torch.isnan(got[77]).all())
    keep = torch.arange(N_VARIANT, device=DEV) != 77
    assert torch.equal(got[keep], c.native[keep])


def test_a_residual_of_zeros_changes_nothing():
    """The residual is added last, so zeros change no bit: with and without the post norm."""
    for name in ("prob", "c128_pre"):
        c = case(name)
        assert torch.equal(c.run(c.x, torch.zeros(N_VARIANT, 128, device=DEV)), c.native)
    c = case("prob_add_norm")
    sd64 = c.sd64
    with torch.no_grad():
        held("prob + norm, zeros for the residual", c.run(c.x, torch.zeros(N_VARIANT, 128, device=DEV)), ref.ffn_ref(c.x.double(), sd64), c.bound)


# ---- 3. module --------------------------------------------------------------------------------------------------------------

def _module(name="base", seed=0, **over):
    """The family's module with the variant's weights (``base`` = the variants base / base_norm, ``prob`` = prob / prob_add_norm)."""
    cfg = dict(ref.FAMILIES[name], **over)
    m = AsymmetricFFN(**cfg)
    shapes = ref.family_shapes(name)
    m.load_state_dict(ref.module_state(ref.fixed_weights(shapes["layers.0.0.weight"][1], "pre_norm.weight" in shapes, "identity_fc.weight" in shapes,
                                                         norm=False, seed=seed)), strict=True)
    return m.to(DEV)


def test_module_runs_native_in_eval(spy):
    c = case("base")
    m = _module().eval()
    with torch.no_grad():
        out = m(c.x)
    assert spy == ["gf_ffn_forward"]
    assert torch.equal(out, c.native)
    p = case("prob")
    with torch.no_grad():
        assert torch.equal(_module("prob").eval()(p.x), p.native) and len(spy) == 2


def test_module_in_training(spy):
    c = case("base")
    m = _module().train()                    # ffn_drop = 0.1
    with torch.no_grad():
        m(c.x)
    assert spy == []
    m = _module(ffn_drop=0.0).train()
    for p in m.parameters():
        p.requires_grad_(False)
    assert torch.equal(m(c.x), c.native) and spy == ["gf_ffn_forward"]     # grad mode on, nothing requires grad, no dropout


def test_module_trains_through_torch(spy):
    c = case("base")
    m = _module().eval()
    x = c.x[:129].clone().requires_grad_(True)
    out = m(x)
    assert spy == []
    (out * torch.cos(torch.arange(out.numel(), device=DEV) * 0.37).view_as(out)).sum().backward()
    assert x.grad is not None and bool(x.grad.abs().sum() > 0)
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0), k
    held("torch route", out.detach(), c.truth[:129], c.bound)


def test_module_uses_the_current_weights():
    c = case("base")
    m = _module().eval()
    with torch.no_grad():
        before = m(c.x)
        m.layers[1].weight[5, 7] += 0.5
        m.layers[0][0].bias[3] -= 0.25
        m.pre_norm.weight[9] *= 2.0
        after = m(c.x)
        truth = ref.ffn_ref(c.x.double(), ref.cast(m.state_dict(), torch.float64))
    assert torch.equal(before, c.native) and not torch.equal(after, before)
    held("changed weights", after, truth, c.bound)


def test_graph_replay_equals_eager():
    c = case("base")
    m = _module().eval()
    x = c.x.clone()
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(x)
        graph.replay()
        assert torch.equal(out, c.native)
        x.copy_(c.x.flip(0))
        graph.replay()
        assert torch.equal(out, c.native.flip(0))


def test_entry_point_refuses_what_it_does_not_support():
    c = case("base_norm")
    out = torch.empty(N_VARIANT, 128, device=DEV)
    fail = r"gf_ffn_forward failed \(code -1\): .*"
    with pytest.raises(RuntimeError, match=fail + "E = 256"):
        raw_call(c.x, c.sd, out, E=256)
    with pytest.raises(RuntimeError, match=fail + "F = 1024"):
        raw_call(c.x, c.sd, out, F_=1024)
    with pytest.raises(RuntimeError, match=fail + "Cin = 192"):
        raw_call(c.x, c.sd, out, cin=192)
    with pytest.raises(RuntimeError, match=fail + "out is not 16-byte aligned"):
        raw_call(c.x, c.sd, torch.empty(N_VARIANT * 128 + 1, device=DEV)[1:])
    raw_call(c.x, c.sd, out, n=0)    # GF_OK, no launch
    with pytest.raises(RuntimeError, match="without a native backward"):
        ffn_block(c.x.clone().requires_grad_(True), *parts(c.sd))


def _own_truth(what, out, truth, y32):
    held(what, out, truth, bound(max_error(y32, truth), truth))


def test_other_configurations_take_the_torch_route(spy):
    x = ref.planted(ref.fixed_input(129, 256, 11)).to(DEV)
    with torch.no_grad():
        # embed_dims = 256
        m = AsymmetricFFN(in_channels=256, pre_norm=dict(type="LN"), embed_dims=256, feedforward_channels=1024).to(DEV).eval()
        sd = ref.cast(ref.fixed_weights(256, True, True, False, e=256, f=1024, seed=4), device=DEV)
        m.load_state_dict(sd, strict=True)
        out = m(x)
        assert out.shape == (129, 256)
        _own_truth("embed_dims 256", out, ref.ffn_ref(x.double(), ref.cast(sd, torch.float64)), ref.ffn_ref(x, sd))
        # GELU
        m = _module(act_cfg=dict(type="GELU")).eval()
        sd = dict(m.state_dict())
        _own_truth("GELU", m(x), ref.ffn_ref(x.double(), ref.cast(sd, torch.float64), act=F.gelu), ref.ffn_ref(x, sd, act=F.gelu))
        # an explicit identity
        m = _module().eval()
        sd = dict(m.state_dict())
        ident = ref.fixed_input(129, 256, 12).to(DEV)

        def with_identity(x, ident, sd):
            plain = {k: v for k, v in sd.items() if not k.startswith("identity_fc")}
            return F.linear(ident, sd["identity_fc.weight"], sd["identity_fc.bias"]) + ref.ffn_ref(x, plain)
        _own_truth("explicit identity", m(x, ident), with_identity(x.double(), ident.double(), ref.cast(sd, torch.float64)), with_identity(x, ident, sd))
    assert spy == []
