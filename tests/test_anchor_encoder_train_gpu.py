"""The anchor encoder's training step on the GPU: ``gf_anchor_embed_forward_train``, ``gf_anchor_embed_backward``,
``AnchorEmbedFunction`` / ``anchor_embed_autograd`` and ``SparseGaussian3DEncoder`` with ``native_training = True`` above them.

Gradients.  The truth is float64 autograd through the restatement (tests/anchor_embed_ref.py) of the scalar
``sum(out * output_weights)``, on rows that pass the kink filter (tests/anchor_embed_train_ref.py; its conditions are asserted
on the CPU, tests/test_anchor_encoder_train.py).  Every n of a family takes the first n survivors, so the rows of ``grad_anchor``
at n are a prefix of those at 1 000.  Per tensor ``max|native - truth| <= 2 Y + 4 eps32 max|truth|`` with Y from the float32
torch composition on the same GPU and rows: for ``grad_anchor`` the family's n = 1 000 value (rows are independent); for a
parameter, relative to the leaf's ``max|truth|``, the LARGEST relative error over the leaves of its kind (square weight, thin
weight, Linear bias, LN weight, LN bias) at the same n, so that one lucky 128-value leaf does not set its own yardstick.  The
measured ratios are printed (-s) and recorded in DESIGN.md §3.13b.

Invariants are bitwise.  Nothing here reads past a buffer's end or inspects code."""
import functools

import pytest
import torch

import anchor_embed_ref as ref
import anchor_embed_train_ref as tr
from gaussianformer_amd import _lib, anchor_encoder
from gaussianformer_amd.anchor_encoder import SparseGaussian3DEncoder, anchor_embed, anchor_embed_autograd, train_sizes
from anchor_embed_ref import LAYOUTS as FAMILIES, make_input
from row_ref import scalar_gradients
from row_judge import ROWS, Guarded, edge_rows, judge_leaves, max_error, ptr_table, spy  # noqa: F401  (spy is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N_FAMILY = 1000
B = _lib.GF_ANCHOR_EMBED_WGRAD_ROWS
EDGE_ROWS = edge_rows(B)


class Case:
    """A family's weights and filtered rows on the GPU, and per n the three sets of gradients (cached)."""

    def __init__(self, name, dead_branch=None, repeat=1):
        self.name, (self.opa, self.S, self.Da) = name, FAMILIES[name]
        rows, sd = tr.survivors(name, dead_branch=dead_branch)
        rows = rows.repeat(repeat, 1)     # (a survivor stays one wherever it stands)
        self.x, self.sd = rows.to(DEV), ref.cast(sd, device=DEV)
        self.sd64 = ref.cast(sd, torch.float64, DEV)

    @functools.lru_cache(maxsize=None)
    def grads(self, n):
        x = self.x[:n].contiguous()
        return (scalar_gradients(ref.anchor_embed_ref, {"anchor": x.double()}, self.sd64),
                scalar_gradients(ref.anchor_embed_ref, {"anchor": x}, self.sd), scalar_gradients(anchor_embed_autograd, {"anchor": x}, self.sd))

    def anchor_yardstick(self):
        truth, t32, _ = self.grads(N_FAMILY)
        return max_error(t32["anchor"], truth["anchor"])


@functools.lru_cache(maxsize=None)
def case(name, dead_branch=None, repeat=1):
    return Case(name, dead_branch, repeat)


def judged(c, n):
    """Every gradient of case ``c`` at ``n`` rows against the bound; returns the native gradients."""
    truth, t32, native = c.grads(n)
    judge_leaves(native, truth, t32, tr.kind, f"{c.name} n={n}", per_row=("anchor",), row_yardstick={"anchor": c.anchor_yardstick()})
    return native


# ---- raw calls on caller-made buffers ---------------------------------------------------------------------------------------

def _ptrs(sd):
    return ptr_table(anchor_encoder._param_list(sd), 48)


def raw_forward_train(x, sd, opa, S, out, saved, saved_bytes, n=None, E=128):
    n = x.shape[0] if n is None else n
    _lib.call("gf_anchor_embed_forward_train", x.device, n, x.shape[1], E, opa, S, x, _ptrs(sd), out, saved, saved_bytes)


def raw_backward(x, sd, opa, S, saved, go, ga, grads, work, work_bytes, n=None, E=128):
    n = x.shape[0] if n is None else n
    _lib.call("gf_anchor_embed_backward", x.device, n, x.shape[1], E, opa, S, x, _ptrs(sd), saved, go, ga, _ptrs(grads), work, work_bytes)


class Raw:
    """One forward_train + backward on buffers with ``pad`` sentinel bytes (0xA5) behind the queried sizes and ``pad_rows``
    sentinel rows behind grad_anchor."""

    def __init__(self, c, n, pad=512, pad_rows=3, fill=None):
        self.c, self.n = c, n
        self.x = c.x[:n].contiguous()
        self.sb, self.wb = train_sizes(n, c.opa, c.S)
        self.guarded = [Guarded(nbytes, DEV, pad, 0xA5, body=0xA5) for nbytes in (self.sb, self.wb)]
        self.saved, self.work = [g.buf for g in self.guarded]
        self.out = torch.empty(n, 128, device=DEV)
        self.go = ref.output_weights((n, 128), torch.float32).to(DEV)
        self.ga = torch.full((n + pad_rows, c.Da), 12345.0, device=DEV)
        self.grads = {k: torch.full_like(v, float("nan") if fill is None else fill) for k, v in c.sd.items()}

    def run(self):
        c = self.c
        raw_forward_train(self.x, c.sd, c.opa, c.S, self.out, self.saved, self.sb)
        raw_backward(self.x, c.sd, c.opa, c.S, self.saved, self.go, self.ga, self.grads, self.work, self.wb)
        return self


# ---- 1. the saving forward ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FAMILIES))
def test_saving_forward_is_bitwise_the_plain_forward(name):
    opa, S, Da = FAMILIES[name]
    sd = ref.cast(ref.fixed_weights(bool(opa), S, seed=0), device=DEV)
    x = make_input(N_FAMILY, opa, S, Da, 7).to(DEV)    # unfiltered, with the planted rows
    for n in ROWS:
        xn = x[:n].contiguous()
        with torch.no_grad():
            plain = anchor_embed(xn, sd)
        sb, _ = train_sizes(n, opa, S)
        out, saved = torch.empty(n, 128, device=DEV), torch.empty(sb, dtype=torch.uint8, device=DEV)
        raw_forward_train(xn, sd, opa, S, out, saved, sb)
        assert torch.equal(out, plain), (name, n)
        assert torch.equal(anchor_embed_autograd(xn.clone().requires_grad_(True), sd).detach(), plain), (name, n)


# ---- 2. gradients against float64 autograd -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FAMILIES))
def test_gradients(name):
    judged(case(name), N_FAMILY)


@pytest.mark.parametrize("n", EDGE_ROWS)
@pytest.mark.parametrize("name", ["opa_s17", "gs144000"])
def test_gradients_at_the_edges(name, n):
    judged(case(name), n)


def test_gradients_across_chunks():
    """More rows than one chunk of the backward: the second chunk has one whole weight-gradient block, a ragged one and a ragged
    tile.  The rows are the survivors over and over (their gradients differ: the scalar's weights go by position)."""
    n = _lib.GF_ANCHOR_EMBED_CHUNK_ROWS + B + 70
    c = case("opa_s17", repeat=-(-n // 1000))     # (the CPU suite asserts at least 1 000 survivors per family)
    assert c.x.shape[0] >= n, f"{c.x.shape[0]} rows from the repeated survivors, {n} needed"
    judged(c, n)


# ---- 3. exact zeros ----------------------------------------------------------------------------------------------------------

def test_unread_columns_get_exact_zeros():
    c = case("opa_s17_da40")
    _, _, native = c.grads(N_FAMILY)
    assert bool((native["anchor"][:, 28:] == 0).all()) and bool((native["anchor"][:, :28] != 0).any(dim=0).all())
    c0 = case("opa_s0")
    wide = torch.full((N_FAMILY, 20), float("nan"), device=DEV)
    wide[:, :11] = c0.x[:N_FAMILY]
    g = scalar_gradients(anchor_embed_autograd, {"anchor": wide}, c0.sd)
    assert bool((g["anchor"][:, 11:] == 0).all())
    assert torch.equal(g["anchor"][:, :11], c0.grads(N_FAMILY)[2]["anchor"])


@pytest.mark.parametrize("branch", ["xyz_fc", "semantics_fc"])
def test_dead_branch(branch):
    """The branch's first ReLU is 0 in every feature: its first stage's weight, bias and LayerNorm-weight gradients are exactly
    0, and so are the gradients of the anchor columns it reads; everything else meets the bound."""
    c = case("opa_s17", dead_branch=branch)
    native = judged(c, N_FAMILY)
    for slot in ("0.weight", "0.bias", "2.weight"):
        assert bool((native[f"{branch}.{slot}"] == 0).all()), slot
    cols = slice(0, 3) if branch == "xyz_fc" else slice(11, 28)
    assert bool((native["anchor"][:, cols] == 0).all())
    assert bool((native[f"{branch}.2.bias"] != 0).any())


# ---- 4. bitwise properties ---------------------------------------------------------------------------------------------------

def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_two_backward_calls_agree():
    c = case("opa_s17")
    r = Raw(c, N_FAMILY).run()
    first = {k: v.clone() for k, v in r.grads.items()}
    ga = r.ga.clone()
    for v in r.grads.values():
        v.fill_(7.0)          # stored, not accumulated: whatever the tensors held
    r.work.fill_(0x3C)
    raw_backward(r.x, c.sd, c.opa, c.S, r.saved, r.go, r.ga, r.grads, r.work, r.wb)
    _same(first, r.grads)
    assert torch.equal(ga, r.ga)
    # ... and they are the autograd function's, whose scalar has the same weights
    native = c.grads(N_FAMILY)[2]
    _same(first, {k: native[k] for k in first})
    assert torch.equal(ga[:N_FAMILY], native["anchor"])


def test_rows_under_a_permutation_and_a_prefix():
    c = case("gs144000")
    n = N_FAMILY
    x, go = c.x[:n].contiguous(), ref.output_weights((n, 128), torch.float32).to(DEV)

    def grad_anchor(x, go):
        x = x.clone().requires_grad_(True)
        anchor_embed_autograd(x, c.sd).backward(go)
        return x.grad
    base = grad_anchor(x, go)
    perm = torch.randperm(n, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    assert torch.equal(grad_anchor(x[perm].contiguous(), go[perm].contiguous()), base[perm])
    assert torch.equal(grad_anchor(x[:129].contiguous(), go[:129].contiguous()), base[:129])


@pytest.mark.parametrize("n", [1, 33, 129, B + 1])
def test_nothing_is_written_beyond_the_queried_sizes(n):
    c = case("opa_s17")
    r = Raw(c, n).run()
    assert all(g.intact() for g in r.guarded)
    assert bool((r.ga[n:] == 12345.0).all()) and bool(torch.isfinite(r.ga[:n]).all())
    native = c.grads(n)[2]
    assert torch.equal(r.ga[:n], native["anchor"])
    _same(r.grads, {k: native[k] for k in r.grads})


def test_unread_columns_do_not_matter():
    c = case("opa_s17_da40")
    x = c.x[:N_FAMILY].clone()
    x[:, 28:34] = float("nan")
    x[:, 34:37] = float("inf")
    x[:, 37:40] = float("-inf")
    _same(scalar_gradients(anchor_embed_autograd, {"anchor": x}, c.sd), c.grads(N_FAMILY)[2])


@pytest.mark.parametrize("col", [0, 4, 9, 10, 11, 27])
def test_a_nan_stays_in_its_row(col):
    c = case("opa_s17")
    x = c.x[:N_FAMILY].clone()
    x[77, col] = float("nan")
    got, t32 = scalar_gradients(anchor_embed_autograd, {"anchor": x}, c.sd), scalar_gradients(ref.anchor_embed_ref, {"anchor": x}, c.sd)
    assert bool(torch.isnan(got["anchor"][77, :28]).all())
    keep = torch.arange(N_FAMILY, device=DEV) != 77
    assert torch.equal(got["anchor"][keep], c.grads(N_FAMILY)[2]["anchor"][keep])
    for k in c.sd:     # the parameter gradients become NaN, as torch's do: all but the last LayerNorm's bias, the sum of grad_out
        assert bool(torch.isnan(got[k]).any()) == bool(torch.isnan(t32[k]).any()), k
        assert bool(torch.isnan(got[k]).any()) == (k != "output_fc.5.bias"), k


# ---- 5. autograd and module ----------------------------------------------------------------------------------------------------

def _module(name="opa_s17", native_training=True, E=128):
    opa, S, Da = FAMILIES[name]
    m = SparseGaussian3DEncoder(embed_dims=E, include_opa=bool(opa), semantics=S > 0, semantic_dim=S or None)
    m.native_training = native_training
    m.load_state_dict(ref.fixed_weights(bool(opa), S, E=E, seed=0), strict=True)
    return m.to(DEV)


def _module_grads(m, x):
    x = x.clone().requires_grad_(True)
    out = m(x)
    (out * ref.output_weights(out.shape, torch.float32).to(DEV)).sum().backward()
    return {"anchor": x.grad, **{k: p.grad for k, p in m.named_parameters()}}


@pytest.mark.parametrize("name", ["opa_s17", "noopa_s0"])
def test_module_trains_natively(name, spy):
    c = case(name)
    got = _module_grads(_module(name), c.x[:N_FAMILY])
    assert spy == ["gf_anchor_embed_forward_train", "gf_anchor_embed_backward"]
    _same(got, c.grads(N_FAMILY)[2])
    del spy[:]
    m = _module(name)
    with torch.no_grad():
        m(c.x[:N_FAMILY])
    assert spy == ["gf_anchor_embed_forward"]
    del spy[:]
    _module_grads(_module(name, native_training=False), c.x[:129])     # the default route: the module's torch layers
    _module_grads(_module(name, E=256), c.x[:129])                     # another width: torch, whatever the switch
    assert spy == []


def test_frozen_input_and_frozen_parameters():
    c = case("opa_s17")
    full = c.grads(N_FAMILY)[2]
    x = c.x[:N_FAMILY].contiguous()
    w = ref.output_weights((N_FAMILY, 128), torch.float32).to(DEV)
    leaves = {k: v.clone().requires_grad_(True) for k, v in c.sd.items()}
    (anchor_embed_autograd(x, leaves) * w).sum().backward()                 # a frozen input
    assert x.grad is None
    _same({k: v.grad for k, v in leaves.items()}, {k: full[k] for k in leaves})
    frozen = ("xyz_fc.0.weight", "rot_fc.5.bias", "output_fc.3.weight")
    leaves = {k: v.clone().requires_grad_(k not in frozen) for k, v in c.sd.items()}
    xg = x.clone().requires_grad_(True)
    (anchor_embed_autograd(xg, leaves) * w).sum().backward()
    assert all(leaves[k].grad is None for k in frozen) and torch.equal(xg.grad, full["anchor"])
    _same({k: v.grad for k, v in leaves.items() if k not in frozen}, {k: full[k] for k in leaves if k not in frozen})
    xg = x.clone().requires_grad_(True)                                       # every parameter frozen
    (anchor_embed_autograd(xg, c.sd) * w).sum().backward()
    assert torch.equal(xg.grad, full["anchor"])
    with torch.no_grad():                                                     # no_grad: the plain forward
        out = anchor_embed_autograd(xg, leaves)
    assert out.grad_fn is None and torch.equal(out, anchor_embed(x, c.sd))
    with pytest.raises(RuntimeError, match="without a native backward"):
        anchor_embed(xg, c.sd)


def test_leading_shape_and_a_non_contiguous_grad_out():
    c = case("opa_s17")
    full = c.grads(N_FAMILY)[2]
    x = c.x[:N_FAMILY].reshape(2, 500, c.Da).clone().requires_grad_(True)
    leaves = {k: v.clone().requires_grad_(True) for k, v in c.sd.items()}
    out = anchor_embed_autograd(x, leaves)
    assert out.shape == (2, 500, 128)
    go = ref.output_weights((N_FAMILY, 128), torch.float32).to(DEV).view(2, 500, 128).permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert not go.is_contiguous()
    out.backward(go)
    assert x.grad.shape == (2, 500, c.Da) and torch.equal(x.grad.view(N_FAMILY, c.Da), full["anchor"])
    _same({k: v.grad for k, v in leaves.items()}, {k: full[k] for k in leaves})


def test_graph_replay_equals_eager():
    c = case("opa_s17")
    m = _module()
    params = list(m.parameters())
    x = c.x[:N_FAMILY].clone().requires_grad_(True)
    w = ref.output_weights((N_FAMILY, 128), torch.float32).to(DEV)

    def step():
        return torch.autograd.grad((m(x) * w).sum(), [x] + params)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for flip in (False, True):
        rows = c.x[:N_FAMILY].flip(0) if flip else c.x[:N_FAMILY]
        with torch.no_grad():
            x.copy_(rows)
        graph.replay()
        eager = _module_grads(_module(), rows)
        assert torch.equal(captured[0], eager["anchor"])
        for g, (k, _) in zip(captured[1:], m.named_parameters()):
            assert torch.equal(g, eager[k]), k


def test_entry_points_refuse_what_they_do_not_support():
    c = case("opa_s17")
    n = 129
    r = Raw(c, n).run()
    fwd = lambda **kw: raw_forward_train(r.x, c.sd, c.opa, kw.pop("S", c.S), r.out, kw.pop("saved", r.saved), kw.pop("sb", r.sb), **kw)
    bwd = lambda **kw: raw_backward(r.x, c.sd, c.opa, kw.pop("S", c.S), kw.pop("saved", r.saved), kw.pop("go", r.go), r.ga, r.grads,
                                    kw.pop("work", r.work), kw.pop("wb", r.wb), **kw)
    F_, B_ = r"gf_anchor_embed_forward_train failed \(code -1\): .*", r"gf_anchor_embed_backward failed \(code -1\): .*"
    with pytest.raises(RuntimeError, match=F_ + "128"):
        fwd(E=256)
    with pytest.raises(RuntimeError, match=B_ + "128"):
        bwd(E=256)
    with pytest.raises(RuntimeError, match=F_ + "S must be"):
        fwd(S=33)
    with pytest.raises(RuntimeError, match=B_ + "S must be"):
        bwd(S=33)
    with pytest.raises(RuntimeError, match=r"gf_anchor_embed_forward_train failed \(code -\d+\): .*saved of \d+ bytes, \d+ needed"):
        fwd(sb=r.sb - 1)
    with pytest.raises(RuntimeError, match=r"gf_anchor_embed_backward failed \(code -\d+\): .*workspace of \d+ bytes, \d+ needed"):
        bwd(wb=r.wb - 1)
    with pytest.raises(RuntimeError, match=F_ + "saved is not 16-byte aligned"):
        fwd(saved=r.saved[4:])
    with pytest.raises(RuntimeError, match=B_ + "saved is not 16-byte aligned"):
        bwd(saved=r.saved[4:])
    with pytest.raises(RuntimeError, match=B_ + "workspace is not 16-byte aligned"):
        bwd(work=r.work[4:])
    with pytest.raises(RuntimeError, match=B_ + "grad_out is not 16-byte aligned"):
        bwd(go=torch.empty(n * 128 + 1, device=DEV)[1:])
    # n == 0: GF_OK, and the parameter gradients are zero-filled
    for v in r.grads.values():
        v.fill_(3.0)
    raw_forward_train(r.x, c.sd, c.opa, c.S, r.out, None, 0, n=0)
    raw_backward(r.x, c.sd, c.opa, c.S, None, None, None, r.grads, None, 0, n=0)
    assert all(bool((v == 0).all()) for v in r.grads.values())
