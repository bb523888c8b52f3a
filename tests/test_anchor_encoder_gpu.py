"""The anchor encoder on the GPU: ``gf_anchor_embed_forward`` and the drop-in ``SparseGaussian3DEncoder`` above it.

Values.  The truth is the float64 restatement (tests/anchor_embed_ref.py) on the same inputs and weights.  Per case
``max|native - truth| <= 2 Y + 4 eps32 max|truth|`` with ``Y = max|float32 torch composition on this GPU - truth|`` taken at the
family's n = 1 000 case (the error statistics do not depend on n, and a 128-value sample must not set its own yardstick); the
factor 2 and the floor are test_refine_gpu.py's.  Every n of a family is a prefix of the family's 1 000 rows, so one truth and
one yardstick per family serve all its cases.  The measured ``max|native - truth| / bound`` per family is printed (-s) and
recorded in DESIGN.md §3.13.

Invariants are bitwise.  Nothing here reads past an input's end or inspects code."""
import functools
import os

import numpy as np
import pytest
import torch

import anchor_embed_ref as ref
from anchor_embed_ref import LAYOUTS as FAMILIES, make_input
from gaussianformer_amd import _lib, anchor_encoder
from gaussianformer_amd.anchor_encoder import SparseGaussian3DEncoder, anchor_embed
from row_judge import ROWS, bound, held, max_error, ptr_table, spy  # noqa: F401  (spy is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_embed.npz")

N_FAMILY = 1000


class Case:
    """A family's weights, its 1 000 rows, the float64 truth, the float32 torch composition and the native result of those."""

    def __init__(self, name, seed=0, dead_branch=None):
        self.opa, self.S, self.Da = FAMILIES[name]
        sd = ref.fixed_weights(bool(self.opa), self.S, seed=seed)
        if dead_branch:   # a first-layer bias that drives the branch's whole ReLU output to 0, whatever the input
            sd[dead_branch + ".0.bias"] = torch.full_like(sd[dead_branch + ".0.bias"], -1e6)
        self.sd = ref.cast(sd, device=DEV)
        self.sd64 = ref.cast(sd, torch.float64, DEV)
        self.x = make_input(N_FAMILY, self.opa, self.S, self.Da, 7 + seed).to(DEV)
        with torch.no_grad():
            self.truth = ref.anchor_embed_ref(self.x.double(), self.sd64)
            self.torch32 = ref.anchor_embed_ref(self.x, self.sd)
            self.native = anchor_embed(self.x, self.sd)
        self.Y = max_error(self.torch32, self.truth)
        self.bound = bound(self.Y, self.truth)


@functools.lru_cache(maxsize=None)
def case(name, dead_branch=None):
    return Case(name, dead_branch=dead_branch)


def raw_call(x, sd, opa, S, out, n=None, Da=None, E=128):
    """The C entry point on caller-made buffers (``sd``: a state_dict on the GPU)."""
    _lib.call("gf_anchor_embed_forward", x.device, x.shape[0] if n is None else n, x.shape[1] if Da is None else Da, E, opa, S,
              x, ptr_table(anchor_encoder._param_list(sd), 48), out)
    return out


# ---- 1. values ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_values(name, n):
    c = case(name)
    with torch.no_grad():
        got = c.native if n == N_FAMILY else anchor_embed(c.x[:n].contiguous(), c.sd)
    held(f"{name} n={n}", got, c.truth[:n], c.bound)


def test_values_many_tiles():
    """n = 40 000: 313 workgroups, more than the chip holds at once."""
    c = case("opa_s17")
    x = ref.fixed_input(40000, c.Da, 99).to(DEV)
    with torch.no_grad():
        held("opa_s17 n=40000", anchor_embed(x, c.sd), ref.anchor_embed_ref(x.double(), c.sd64), c.bound)


def test_values_leading_shape():
    c = case("opa_s17")
    with torch.no_grad():
        got = anchor_embed(c.x.view(2, 500, c.Da), c.sd)
    assert got.shape == (2, 500, 128)
    assert torch.equal(got.view(1000, 128), c.native)
    held("opa_s17 [2, 500, Da]", got.view(1000, 128), c.truth, c.bound)


@pytest.mark.parametrize("branch", ["xyz_fc", "semantics_fc"])
def test_dead_branch_layernorm_gives_its_bias(branch):
    """The branch's first ReLU is 0 in every feature, so its LayerNorm sees a constant row: mean 0, deviations 0, and the result
    is the LayerNorm's bias exactly -- in the truth and here.  Then the branch no longer depends on its input columns, bitwise."""
    c = case("opa_s17", dead_branch=branch)
    held(f"dead {branch}", c.native, c.truth, c.bound)
    x2 = c.x.clone()
    cols = slice(0, 3) if branch == "xyz_fc" else slice(11, 28)
    x2[:, cols] = torch.randn(N_FAMILY, cols.stop - cols.start, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    with torch.no_grad():
        assert torch.equal(anchor_embed(x2, c.sd), c.native)
        # ... and the truth with the branch's feature computed FROM that bias: LN1 gives be1, so stage two sees W2 be1 + b2
        sd64, xd = c.sd64, c.x.double()
        h = torch.relu(sd64[branch + ".3.weight"] @ sd64[branch + ".2.bias"] + sd64[branch + ".3.bias"])
        feats = {"xyz_fc": ref._stage(xd[:, 0:3], sd64, "xyz_fc"), "scale_fc": ref._stage(xd[:, 3:6], sd64, "scale_fc"),
                 "rot_fc": ref._stage(xd[:, 6:10], sd64, "rot_fc"), "opacity_fc": ref._stage(xd[:, 10:11], sd64, "opacity_fc"),
                 "semantics_fc": ref._stage(xd[:, 11:28], sd64, "semantics_fc")}
        feats[branch] = torch.nn.functional.layer_norm(h, (128,), sd64[branch + ".5.weight"], sd64[branch + ".5.bias"], 1e-5).expand(N_FAMILY, 128)
        total = feats["xyz_fc"] + feats["scale_fc"] + feats["rot_fc"] + feats["opacity_fc"] + feats["semantics_fc"]
        truth = ref._stage(total, sd64, "output_fc")
    held(f"dead {branch} against the bias form", c.native, truth, c.bound)


@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_module_with_the_fixture_s_weights(name):
    """The drop-in on the reference's recorded input: held to the recorded float64 output, the recorded float32 output (the
    reference's own, on the CPU) as the yardstick."""
    g = np.load(GOLDEN)
    cfg = ref.FAMILIES[name]
    opa, S = bool(cfg["include_opa"]), cfg["semantic_dim"] or 0
    module = SparseGaussian3DEncoder(embed_dims=128, **cfg)
    module.load_state_dict(ref.fixed_weights(opa, S, seed=int(g[name + ".seed"])), strict=True)
    module.to(DEV)
    truth = torch.from_numpy(g[name + ".out64"]).to(DEV)
    with torch.no_grad():
        held(f"fixture {name}", module(torch.from_numpy(g[name + ".input"]).to(DEV)), truth,
             bound(max_error(g[name + ".out32"], g[name + ".out64"]), g[name + ".out64"]))


# ---- 2. invariants, bitwise -------------------------------------------------------------------------------------------------

def test_two_calls_agree():
    c = case("opa_s17")
    with torch.no_grad():
        assert torch.equal(anchor_embed(c.x, c.sd), c.native)


def test_permutation_of_rows():
    c = case("gs144000")
    perm = torch.randperm(N_FAMILY, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    with torch.no_grad():
        assert torch.equal(anchor_embed(c.x[perm], c.sd), c.native[perm])


def test_rows_do_not_depend_on_n():
    c = case("opa_s17")
    with torch.no_grad():
        assert torch.equal(anchor_embed(c.x[:129].contiguous(), c.sd), c.native[:129])


def test_nothing_is_written_beyond_row_n():
    c = case("opa_s17")
    for n in (1, 33, 129):
        out = torch.full((n + 200, 128), 12345.0, device=DEV)
        raw_call(c.x, c.sd, c.opa, c.S, out, n=n)
        assert torch.equal(out[:n], c.native[:n])
        assert bool((out[n:] == 12345.0).all())


def test_unread_columns_do_not_matter():
    c = case("opa_s17_da40")
    x = c.x.clone()
    x[:, 28:34] = float("nan")
    x[:, 34:37] = float("inf")
    x[:, 37:40] = float("-inf")
    with torch.no_grad():
        assert torch.equal(anchor_embed(x, c.sd), c.native)
    # without opacity column 10 is the first semantic column, with it and S = 0 nothing is read beyond it
    c0 = case("opa_s0")
    wide = torch.full((N_FAMILY, 20), float("nan"), device=DEV)
    wide[:, :11] = c0.x
    with torch.no_grad():
        assert torch.equal(anchor_embed(wide, c0.sd), c0.native)


@pytest.mark.parametrize("col", [0, 4, 9, 10, 11, 27])
def test_a_nan_stays_in_its_row(col):
    c = case("opa_s17")
    x = c.x.clone()
    x[77, col] = float("nan")
    with torch.no_grad():
        got = anchor_embed(x, c.sd)
    assert bool(torch.isnan(got[77]).all())
    keep = torch.arange(N_FAMILY, device=DEV) != 77
    assert torch.equal(got[keep], c.native[keep])


# ---- 3. module --------------------------------------------------------------------------------------------------------------

def _module(name="opa_s17", E=128, seed=0):
    opa, S, Da = FAMILIES[name]
    m = SparseGaussian3DEncoder(embed_dims=E, include_opa=bool(opa), semantics=S > 0, semantic_dim=S or None)
    m.load_state_dict(ref.fixed_weights(bool(opa), S, E=E, seed=seed), strict=True)
    return m.to(DEV)


def test_module_runs_native_without_grad(spy):
    c = case("opa_s17")
    m = _module()
    with torch.no_grad():
        out = m(c.x)
    assert spy == ["gf_anchor_embed_forward"]
    assert torch.equal(out, c.native)
    for p in m.parameters():
        p.requires_grad_(False)
    assert torch.equal(m(c.x), c.native) and len(spy) == 2      # grad mode on, nothing requires grad


def test_module_trains_through_torch(spy):
    c = case("opa_s17")
    m = _module()
    x = c.x[:129].clone().requires_grad_(True)
    out = m(x)
    assert spy == []
    (out * ref.output_weights(out.shape, torch.float32).to(DEV)).sum().backward()
    assert x.grad is not None and bool(x.grad.abs().sum() > 0)
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0), k
    held("torch route", out.detach(), c.truth[:129], c.bound)


def test_module_uses_the_current_weights():
    c = case("opa_s17")
    m = _module()
    with torch.no_grad():
        before = m(c.x)
        m.output_fc[3].weight[5, 7] += 0.5
        m.xyz_fc[0].bias[3] -= 0.25
        after = m(c.x)
        sd64 = ref.cast(m.state_dict(), torch.float64)
        truth = ref.anchor_embed_ref(c.x.double(), sd64)
    assert torch.equal(before, c.native) and not torch.equal(after, before)
    held("changed weights", after, truth, c.bound)


def test_graph_replay_equals_eager():
    c = case("opa_s17")
    m = _module()
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
    c = case("opa_s17")
    out = torch.empty(N_FAMILY, 128, device=DEV)
    with pytest.raises(RuntimeError, match=r"gf_anchor_embed_forward failed \(code -1\): .*128"):
        raw_call(c.x, c.sd, c.opa, c.S, out, E=256)
    with pytest.raises(RuntimeError, match=r"gf_anchor_embed_forward failed \(code -1\): .*S must be"):
        raw_call(c.x, c.sd, c.opa, 33, out)
    with pytest.raises(RuntimeError, match=r"gf_anchor_embed_forward failed \(code -1\): .*Da"):
        raw_call(c.x, c.sd, c.opa, c.S, out, Da=27)
    with pytest.raises(RuntimeError, match=r"gf_anchor_embed_forward failed \(code -1\): .*out is not 16-byte aligned"):
        raw_call(c.x, c.sd, c.opa, c.S, torch.empty(N_FAMILY * 128 + 1, device=DEV)[1:])
    raw_call(c.x, c.sd, c.opa, c.S, out, n=0)    # GF_OK, no launch


def test_other_widths_take_the_torch_route(spy):
    m = _module(E=256)
    x = make_input(129, 1, 17, 28, 11).to(DEV)
    with torch.no_grad():
        out = m(x)
        truth = ref.anchor_embed_ref(x.double(), ref.cast(m.state_dict(), torch.float64))
        y = max_error(ref.anchor_embed_ref(x, dict(m.state_dict())), truth)
    assert spy == [] and out.shape == (129, 256)
    held("embed_dims 256", out, truth, bound(y, truth))
