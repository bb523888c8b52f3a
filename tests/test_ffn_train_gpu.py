"""The feed-forward block's training step on the GPU: ``gf_ffn_forward_train`` / ``gf_ffn_backward`` under
``ffn_block_autograd``, and ``AsymmetricFFN.native_training``.

Values.  The truth is float64 autograd of ``sum(out * w)`` through the restatement with the SAME masks (tests/ffn_train_ref.py)
on rows that pass the kink filter.  Per tensor ``max|native - truth| <= 2 Y + 4 eps32 max|truth|``: for ``out``, ``grad_x`` and
``grad_residual`` Y is ``max|float32 torch composition with the same masks on this GPU - truth|`` over the variant's 1 000 rows
(every smaller n is a prefix of them) or over the case's own rows beyond; for a parameter, relative to the leaf's
``max|truth|``, the LARGEST relative error of the float32 composition over the leaves of its kind at the same n.  The measured
ratios are printed (-s) and recorded in DESIGN.md §3.13d.

Invariants are bitwise.  Nothing here reads past a buffer's end or inspects code."""
import functools

import pytest
import torch

import ffn_ref as ref
import ffn_train_ref as tr
from gaussianformer_amd import _lib, ffn as ffn_mod
from gaussianformer_amd.ffn import AsymmetricFFN, ffn_block, ffn_block_autograd, train_sizes
from ffn_ref import VARIANTS, parts
from row_ref import scalar_gradients
from row_judge import ROWS, Guarded, judge_leaves, max_error, ptr_table, spy  # noqa: F401  (spy is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N_VARIANT = 1000
P = 0.1
B, CHUNK = _lib.GF_FFN_WGRAD_ROWS, _lib.GF_FFN_CHUNK_ROWS
PER_ROW = ("out", "x", "residual")


def gradients(forward, x, res, sd):
    """``{"out": out, "x": d/dx, "residual": d/dresidual (where given), key: d/d sd[key]}`` of ``sum(forward(x, res, leaves) *
    output_weights)``; ``forward`` is the restatement (masks bound) or the native functional."""
    return scalar_gradients(forward, {"x": x, "residual": res}, sd, with_out=True)


class Case:
    """A variant's weights, its filtered rows, residual and masks on the GPU, and per n the three sets of results (cached)."""

    def __init__(self, name, masked=True, dead=False, count=tr.CANDIDATES):
        self.name, self.masked = name, masked
        self.cin, pre, ident, self.has_res, norm = VARIANTS[name]
        rows, sd = tr.survivors(self.cin, pre, ident, norm, 0, count, dead)
        self.x, self.sd, self.sd64 = rows.to(DEV), ref.cast(sd, device=DEV), ref.cast(sd, torch.float64, DEV)
        self.rows = rows.shape[0]
        self.res = ref.fixed_input(self.rows, 128, 200).to(DEV) if self.has_res else None
        self.kh, self.ko, _ = tr.masks(self.rows, P, 0, DEV)

    def masks(self, n):
        return (self.kh[:n], self.ko[:n], P) if self.masked else (None, None, 0.0)

    def native_forward(self, kh, ko, p):
        def forward(x, res, sd):
            module, norm = parts(sd)
            return ffn_block_autograd(x, module, norm=norm, residual=res, p_hidden=p, p_out=p, keep_hidden=kh, keep_out=ko)
        return forward

    def inputs(self, n):
        return self.x[:n].contiguous(), None if self.res is None else self.res[:n].contiguous()

    @functools.lru_cache(maxsize=None)
    def grads(self, n):
        x, res = self.inputs(n)
        kh, ko, p = self.masks(n)
        scale = 1.0 / (1.0 - p)

        def restated(x, res, sd):
            return tr.ffn_train_ref(x, sd, res, kh, scale, ko, scale)
        return (gradients(restated, x.double(), None if res is None else res.double(), self.sd64), gradients(restated, x, res, self.sd),
                gradients(self.native_forward(kh, ko, p), x, res, self.sd))


@functools.lru_cache(maxsize=None)
def case(name, masked=True, dead=False, count=tr.CANDIDATES):
    return Case(name, masked, dead, count)


def judged(c, n):
    """Every result of case ``c`` at ``n`` rows against its bound; returns the native results."""
    truth, t32, native = c.grads(n)
    ytruth, y32, _ = c.grads(max(n, N_VARIANT))
    judge_leaves(native, truth, t32, tr.kind, f"{c.name} masked={c.masked} n={n}", per_row=PER_ROW,
                 row_yardstick={k: max_error(y32[k], ytruth[k]) for k in PER_ROW if k in ytruth})
    return native


# ---- 1. values ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_values(name, masked, n):
    judged(case(name, masked), n)


@pytest.mark.parametrize("n", [B - 1, B, B + 1])
@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_values_at_the_weight_gradient_block_s_edges(name, n):
    judged(case(name), n)


def test_values_beyond_a_chunk():
    """n = GF_FFN_CHUNK_ROWS + 1: a second chunk of one row with a weight-gradient block of one row; and the tile kernel
    on the plain forward's side of the two kernels' switch."""
    c = case("base_norm", True, False, 36000)
    n = CHUNK + 1
    assert c.rows >= n
    native = judged(c, n)
    x, res = c.inputs(n)
    module, norm = parts(c.sd)
    with torch.no_grad():
        plain = ffn_block(x, module, norm=norm, residual=res)
        ones = torch.ones(n, 512, dtype=torch.uint8, device=DEV)
        assert torch.equal(ffn_block_autograd(x, module, norm=norm, residual=res, keep_hidden=ones, keep_out=ones[:, :128].contiguous()), plain)
    x = x.clone().requires_grad_(True)
    assert torch.equal(ffn_block_autograd(x, module, norm=norm, residual=res).detach(), plain)
    assert native["out"].shape == plain.shape


# ---- 2. exact ----------------------------------------------------------------------------------------------------------------

def _grads_with(c, n, kh, ko, sd=None):
    x, res = c.inputs(n)
    return gradients(c.native_forward(kh, ko, P), x, res, c.sd if sd is None else sd)


@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_all_dropped(name):
    c = case(name)
    n = 333
    other = dict(c.sd)
    other["layers.0.0.weight"] = torch.randn(c.sd["layers.0.0.weight"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    zeros_h, zeros_o = torch.zeros(n, 512, dtype=torch.uint8, device=DEV), torch.zeros(n, 128, dtype=torch.uint8, device=DEV)
    # keep_hidden all zero: nothing depends on W1, and nothing reaches it
    a, b = _grads_with(c, n, zeros_h, c.ko[:n]), _grads_with(c, n, zeros_h, c.ko[:n], other)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["x"], b["x"])
    for g in (a, b):
        for k in ("layers.0.0.weight", "layers.0.0.bias", "layers.1.weight"):
            assert bool((g[k] == 0).all()), k
        assert bool(g["layers.1.bias"].abs().sum() > 0) and bool(torch.isfinite(g["x"]).all())
    # keep_out all zero: the second layer's bias is dropped with its output
    g = _grads_with(c, n, c.kh[:n], zeros_o)
    for k in ("layers.0.0.weight", "layers.0.0.bias", "layers.1.weight", "layers.1.bias"):
        assert bool((g[k] == 0).all()), k
    assert bool(torch.isfinite(g["out"]).all())


@pytest.mark.parametrize("name", ["base_norm", "prob"])
def test_dead_hidden_layer(name):
    """``layers.0.0.bias = -1e6``: the hidden row is 0 in every feature, so are the three gradients behind it; the rest is held
    to the truth."""
    c = case(name, True, True)
    g = judged(c, 333)
    for k in ("layers.0.0.weight", "layers.0.0.bias", "layers.1.weight"):
        assert bool((g[k] == 0).all()), k


# ---- 3. bitwise --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ROWS + (B - 1, B, B + 1))
@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm", "base", "c128_pre"])
def test_out_is_the_plain_forward_s(name, n):
    c = case(name)
    x, res = c.inputs(n)
    module, norm = parts(c.sd)
    with torch.no_grad():
        plain = ffn_block(x, module, norm=norm, residual=res)
        ones_h, ones_o = torch.ones(n, 512, dtype=torch.bool, device=DEV), torch.ones(n, 128, dtype=torch.uint8, device=DEV)
        assert torch.equal(ffn_block_autograd(x, module, norm=norm, residual=res, keep_hidden=ones_h, keep_out=ones_o), plain)
    out = ffn_block_autograd(x.clone().requires_grad_(True), module, norm=norm, residual=res)
    assert out.requires_grad and torch.equal(out.detach(), plain)


@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_two_calls_agree(name):
    c = case(name)
    n = 2 * B + 77      # three weight-gradient blocks, the last ragged
    a, b = _grads_with(c, n, c.kh[:n], c.ko[:n]), _grads_with(c, n, c.kh[:n], c.ko[:n])
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_rows_do_not_depend_on_n_or_position(name):
    """``grad_x`` and ``grad_residual`` of a row: the same bits in a prefix, and under a permutation of the rows with their masks
    (the scalar's weights permuted with them)."""
    c = case(name)
    full = c.grads(N_VARIANT)[2]
    pre = c.grads(129)[2]
    # (the scalar's weights are cos(0.37 i) over the flattened output, so a prefix sees the same grad_out rows)
    for k in ("out", "x", "residual"):
        if k in full:
            assert torch.equal(pre[k], full[k][:129]), k
    perm = torch.randperm(N_VARIANT, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    x, res = c.inputs(N_VARIANT)
    xp = x[perm].clone().requires_grad_(True)
    rp = None if res is None else res[perm].clone().requires_grad_(True)
    module, norm = parts(c.sd)
    out = ffn_block_autograd(xp, module, norm=norm, residual=rp, p_hidden=P, p_out=P, keep_hidden=c.kh[:N_VARIANT][perm], keep_out=c.ko[:N_VARIANT][perm])
    w = tr.output_weights((N_VARIANT, 128), torch.float32).to(DEV)[perm]
    got = torch.autograd.grad((out * w).sum(), [xp] + ([] if rp is None else [rp]))
    assert torch.equal(out.detach(), full["out"][perm]) and torch.equal(got[0], full["x"][perm])
    if rp is not None:
        assert torch.equal(got[1], full["residual"][perm])


def test_graph_replay_equals_eager():
    c = case("base_norm")
    n = 777
    eager = _grads_with(c, n, c.kh[:n], c.ko[:n])
    x, _ = c.inputs(n)
    x = x.clone().requires_grad_(True)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in c.sd.items()}
    keys = list(leaves)
    w = tr.output_weights((n, 128), torch.float32).to(DEV)
    forward = c.native_forward(c.kh[:n].contiguous(), c.ko[:n].contiguous(), P)

    def step():
        out = forward(x, None, leaves)
        return out, torch.autograd.grad((out * w).sum(), [x] + [leaves[k] for k in keys])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, got = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), eager["out"]) and torch.equal(got[0], eager["x"])
    for k, g in zip(keys, got[1:]):
        assert torch.equal(g, eager[k]), k


def _raw_step(c, n, kh, ko, tail=4096, fill=12345.0):
    """Both launching entry points on caller-made buffers with ``tail`` sentinel elements behind ``out``, ``grad_x``,
    ``grad_residual``, ``saved`` and ``workspace``: returns the results and whether every sentinel survived."""
    x, res = c.inputs(n)
    module, norm = parts(c.sd)
    params = ffn_mod._param_list(module, norm)
    table = ptr_table(params)
    grads = [None if p is None else torch.empty_like(p) for p in params]
    saved_bytes, work_bytes = train_sizes(n, c.cin)
    out, gx, gres = [Guarded(4 * n * width, DEV, 4 * tail, fill, body=fill) for width in (128, c.cin, 128)]
    saved, work = [Guarded(nbytes, DEV, tail, 0x5A, body=0x5A) for nbytes in (saved_bytes, work_bytes)]
    scale = 1.0 / (1.0 - P)
    _lib.call("gf_ffn_forward_train", DEV, n, c.cin, 512, 128, x, table, res, kh, scale, ko, scale, out.buf, saved.buf, saved_bytes)
    go = tr.output_weights((n, 128), torch.float32).to(DEV)
    _lib.call("gf_ffn_backward", DEV, n, c.cin, 512, 128, x, table, kh, scale, ko, scale, saved.buf, go, gx.buf,
              gres.buf if res is not None else None, ptr_table(grads), work.buf, work_bytes)
    intact = all(g.intact() for g in (out, gx, gres, saved, work)) and (res is not None or bool((gres.floats(n, 128) == fill).all()))
    return out.floats(n, 128), gx.floats(n, c.cin), gres.floats(n, 128), grads, intact


@pytest.mark.parametrize("n", [1, 33, 129, B + 1])
@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_nothing_is_written_beyond_an_end_and_masks_need_no_alignment(name, n):
    """Sentinels behind every region the entry points write survive; the masks, placed at an odd address with the opposite
    value behind their last row, give the bits of the masks on their own and are not written."""
    c = case(name)
    kh, ko = c.kh[:n].contiguous(), c.ko[:n].contiguous()
    out, gx, gres, grads, intact = _raw_step(c, n, kh, ko)
    assert intact
    native = _grads_with(c, n, kh, ko)
    assert torch.equal(out, native["out"]) and torch.equal(gx, native["x"])
    if c.has_res:
        assert torch.equal(gres, native["residual"])
    module, norm = parts(c.sd)
    names = [k for k, p in zip(ffn_mod._KEYS + ref.NORM_KEYS, ffn_mod._param_list(module, norm)) if p is not None]
    for k, g in zip(names, [g for g in grads if g is not None]):
        assert torch.equal(g, native[k]), k
    # one byte in: an odd address; behind the last row the complement of its last byte
    big_h = torch.empty(1 + n * 512 + 64, dtype=torch.uint8, device=DEV)
    big_o = torch.empty(1 + n * 128 + 64, dtype=torch.uint8, device=DEV)
    for big, m in ((big_h, kh), (big_o, ko)):
        big[0] = 1 - m.view(-1)[0]
        big[1:1 + m.numel()] = m.view(-1)
        big[1 + m.numel():] = 1 - m.view(-1)[-1]
    before = (big_h.clone(), big_o.clone())
    odd_h, odd_o = big_h[1:1 + n * 512].view(n, 512), big_o[1:1 + n * 128].view(n, 128)
    assert odd_h.data_ptr() % 2 == 1 and odd_o.data_ptr() % 2 == 1
    out2, gx2, gres2, grads2, intact = _raw_step(c, n, odd_h, odd_o)
    assert intact and torch.equal(out2, out) and torch.equal(gx2, gx) and torch.equal(gres2, gres)
    assert all(torch.equal(a, b) for a, b in zip([g for g in grads if g is not None], [g for g in grads2 if g is not None]))
    assert torch.equal(big_h, before[0]) and torch.equal(big_o, before[1])


# ---- 4. NaN ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("col", [0, 100])
@pytest.mark.parametrize("name", ["base_norm", "prob_add_norm"])
def test_a_nan_stays_in_its_row(name, col):
    """A NaN in one row of x: exactly that row of out, grad_x and grad_residual is NaN, and the parameter gradients are NaN
    where the float32 torch composition's are."""
    c = case(name)
    n, bad = 300, 77
    x, res = c.inputs(n)
    x = x.clone()
    x[bad, col] = float("nan")
    kh, ko = c.kh[:n], c.ko[:n]
    scale = 1.0 / (1.0 - P)
    native = gradients(c.native_forward(kh, ko, P), x, res, c.sd)
    t32 = gradients(lambda x, res, sd: tr.ffn_train_ref(x, sd, res, kh, scale, ko, scale), x, res, c.sd)
    keep = torch.arange(n, device=DEV) != bad
    for k in PER_ROW:
        if k in native:
            assert bool(torch.isnan(native[k][bad]).all()), k
            assert bool(torch.isfinite(native[k][keep]).all()), k
    for k in native:
        if k not in PER_ROW:
            assert torch.equal(torch.isnan(native[k]), torch.isnan(t32[k])), k


# ---- 5. module ---------------------------------------------------------------------------------------------------------------

def _module(name="base", **over):
    m = AsymmetricFFN(**dict(ref.FAMILIES[name], **over))
    shapes = ref.family_shapes(name)
    if not over:
        m.load_state_dict(ref.module_state(ref.fixed_weights(shapes["layers.0.0.weight"][1], "pre_norm.weight" in shapes, "identity_fc.weight" in shapes,
                                                             norm=False, seed=0)), strict=True)
    m.native_training = True
    return m.to(DEV)


@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_module_trains_natively(spy, name):
    m = _module(name).train()                      # ffn_drop = 0.1
    c = case("base" if name == "base" else "prob")
    x = c.x[:333].clone().requires_grad_(True)
    torch.manual_seed(7)
    out = m(x)
    assert spy == ["gf_ffn_forward_train"] and out.requires_grad
    (out * tr.output_weights(out.shape, torch.float32).to(DEV)).sum().backward()
    assert spy == ["gf_ffn_forward_train", "gf_ffn_backward"]
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and bool(x.grad.abs().sum() > 0)
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0), k
    # stochastic, and reproducible from the generator
    again = m(x)
    torch.manual_seed(7)
    same = m(x)
    assert not torch.equal(again, out) and torch.equal(same, out)
    # eval mode under no_grad: the plain forward alone
    del spy[:]
    m.eval()
    with torch.no_grad():
        plain = m(x)
    assert spy == ["gf_ffn_forward"]
    # eval mode with autograd: no dropout, the plain forward's bits, the native backward
    del spy[:]
    out = m(x)
    assert spy == ["gf_ffn_forward_train"] and torch.equal(out.detach(), plain)


def test_module_sees_an_in_place_weight_change():
    m = _module().train()
    c = case("base")
    x = c.x[:129].clone().requires_grad_(True)

    def step():
        torch.manual_seed(3)
        out = m(x)
        grads = torch.autograd.grad((out * tr.output_weights(out.shape, torch.float32).to(DEV)).sum(), [x] + list(m.parameters()))
        return out.detach(), grads
    out0, g0 = step()
    with torch.no_grad():
        m.layers[1].weight[5, 7] += 0.5
        m.layers[0][0].bias[3] -= 0.25
    out1, g1 = step()
    assert not torch.equal(out0, out1) and not torch.equal(g0[0], g1[0])
    # the same masks (the generator was reset): the truth on the changed weights
    torch.manual_seed(3)
    kh = torch.empty(129, 512, dtype=torch.uint8, device=DEV).bernoulli_(1 - P)
    ko = torch.empty(129, 128, dtype=torch.uint8, device=DEV).bernoulli_(1 - P)
    sd64 = ref.cast(m.state_dict(), torch.float64)
    with torch.no_grad():
        truth = tr.ffn_train_ref(x.detach().double(), sd64, None, kh, 1 / (1 - P), ko, 1 / (1 - P))
    assert (out1.double() - truth).abs().max().item() <= 1e-4 * truth.abs().max().item()


def test_with_the_switch_set_other_configurations_take_the_torch_route(spy):
    x = ref.fixed_input(129, 256, 11).to(DEV).requires_grad_(True)
    for over in (dict(embed_dims=256, feedforward_channels=1024, pre_norm=None), dict(act_cfg=dict(type="GELU")),
                 dict(dropout_layer=dict(type="Dropout", drop_prob=0.2))):
        m = _module(**over).train()
        m(x).sum().backward()
    m = _module().train()
    m(x, ref.fixed_input(129, 256, 12).to(DEV)).sum().backward()        # an explicit identity
    assert spy == []


def test_drawn_masks_keep_their_share():
    """n = 4 096: the kept share of both drawn masks is within 4 sigma of 1 - p (sigma: the binomial's)."""
    n = 4096
    torch.manual_seed(0)
    for width, what in ((512, "p_hidden"), (128, "p_out")):
        keep, scale = ffn_mod._keep_mask(None, P, (n, width), DEV, what)
        assert keep.dtype == torch.uint8 and keep.shape == (n, width) and abs(scale - 1 / (1 - P)) < 1e-12 and int(keep.max()) == 1
        share = keep.float().mean().item()
        sigma = (P * (1 - P) / (n * width)) ** 0.5
        print(f"{what}: kept share {share:.5f}, 1 - p = {1 - P}, sigma = {sigma:.2e}")
        assert abs(share - (1 - P)) <= 4 * sigma
