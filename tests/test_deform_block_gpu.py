"""The deformable block's dense ends on the GPU -- ``gf_deform_logits_forward``, ``gf_deform_output_forward``, the functions
``deformable_logits`` / ``deformable_output`` -- and the drop-in ``DeformableFeatureAggregation`` above them.

Values.  The truth is the float64 restatement (tests/deform_block_ref.py) on the same inputs and weights.  Per case and output
``max|native - truth| <= 2 Y + 4 eps32 max|truth|`` with ``Y = max|float32 torch composition on this GPU - truth|`` taken at the
variant's n = 1 000 case (the project's rule: test_ffn_gpu.py).  Every n of a variant is a prefix of the variant's 1 000 rows,
so one truth and one yardstick per variant serve all its cases.  The variant's first four rows are planted (zeros, 1e-30, +-1e4)
and the +-1e4 rows set both sides of that bound, so the rule is applied a second time to the ordinary rows alone (rows 4 ..: the
bound from those rows' own Y and truth, a thousand times smaller); cases without planted rows are held to that one.  The measured
``max|native - truth| / bound`` per variant is printed (-s) and recorded in DESIGN.md §3.13e.

Invariants are bitwise.  Nothing here reads past an input's end or inspects code."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deform_block_ref as ref
from gaussianformer_amd import _lib, synthetic
from gaussianformer_amd.deformable_block import DeformableFeatureAggregation, deformable_logits, deformable_output
from gaussianformer_amd.deformable_prepare import deformable_fused
from row_judge import ROWS, TILE_EDGES, bound, held, max_error, ptr_table, spy  # noqa: F401  (spy is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caller_dfa.npz")

# name: (3K, Nw, with anchor_embed) -- the shipped widths (solid; base and prob; the two without the camera embedding), then both
# widths on a non-multiple of 32 with a single partial chunk, and Nw just past a chunk edge
FRONT = {"solid": (6, 144, True), "base": (18, 208, True), "nocam_solid": (0, 864, True), "nocam_base": (18, 1248, True),
         "narrow": (30, 16, False), "edge": (3, 132, True)}
# name: (residual_mode, residual, post norm)
BACK = {"none": ("none", False, False), "add": ("add", False, False), "cat": ("cat", False, False),
        "none_res_norm": ("none", True, True), "add_norm": ("add", False, True)}
N_VARIANT = 1000
SENTINEL = 12345.0
PLANTED = 4                                   # ref.planted()'s rows


def bound_of(truth, torch32):
    return bound(max_error(torch32, truth), truth)


def big_rows():
    """The least multiple of 128 rows that the 128-row kernels take (the 32-row ones run while n <= 32 x the CU count), plus a tile."""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    return (32 * cus + 127) // 128 * 128 + 128


class Front:
    """A variant's weights, its 1 000 rows, the float64 truth, the float32 torch composition and the native result of those."""

    def __init__(self, name, seed=0):
        self.k3, self.nw, with_e = FRONT[name]
        sd = ref.fixed_weights(ref.dense_shapes(self.k3, self.nw), seed=seed)
        self.sd, self.sd64 = ref.cast(sd, device=DEV), ref.cast(sd, torch.float64, DEV)
        self.f = ref.planted(ref.fixed_input(N_VARIANT, 128, 7 + seed)).to(DEV)
        self.e = ref.fixed_input(N_VARIANT, 128, 17 + seed).to(DEV) if with_e else None
        self.truth, self.torch32 = self.ref(self.f, self.e, self.sd64), self.ref(self.f, self.e, self.sd)
        self.native = self.run(self.f, self.e)
        self.bounds = [None if t is None else bound_of(t, y) for t, y in zip(self.truth, self.torch32)]
        self.ordinary = [None if t is None else bound_of(t[PLANTED:], y[PLANTED:]) for t, y in zip(self.truth, self.torch32)]

    def params(self, sd=None):
        sd = self.sd if sd is None else sd
        return (sd["weights_fc.weight"], sd["weights_fc.bias"]), (sd.get("kps_generator.learnable_fc.weight"), sd.get("kps_generator.learnable_fc.bias"))

    def ref(self, f, e, sd):
        (ww, bw), (wl, bl) = self.params(sd)
        with torch.no_grad():
            return ref.logits_ref(f.to(ww.dtype), None if e is None else e.to(ww.dtype), ww, bw, wl, bl)

    def run(self, f, e):
        wfc, lfc = self.params()
        with torch.no_grad():
            raw, learned = deformable_logits(f, e, wfc, lfc if self.k3 else None)
        return raw, None if learned is None else learned.flatten(-2)

    def rows(self, n):
        return self.f[:n].contiguous(), None if self.e is None else self.e[:n].contiguous()

    def raw_call(self, f, e, n, learned, raw):
        """The C entry point on caller-made buffers."""
        (ww, bw), (wl, bl) = self.params()
        _lib.call("gf_deform_logits_forward", DEV, n, 128, self.k3, self.nw, f, e, ptr_table((wl, bl, ww, bw)), learned, raw)

    def check(self, what, got, truth, planted=True):
        """``planted``: the rows are a prefix of the variant's own (all rows to the variant's bound, rows 4 .. to the ordinary
        rows' bound); otherwise all of them are ordinary."""
        for part, g, t, b, o in zip(("raw", "learned"), got, truth, self.bounds, self.ordinary):
            if t is None:
                continue
            if planted:
                held(f"{what} {part}", g, t, b)
            if not planted or t.shape[0] > PLANTED:
                skip = PLANTED if planted else 0
                held(f"{what} {part}, ordinary rows", g[skip:], t[skip:], o)
        assert (got[1] is None) == (self.k3 == 0)


class Back:
    def __init__(self, name, seed=0):
        self.mode, has_res, has_norm = BACK[name]
        sd = ref.fixed_weights(ref.dense_shapes(0, 16, norm=has_norm), seed=seed + 3)
        self.sd, self.sd64 = ref.cast(sd, device=DEV), ref.cast(sd, torch.float64, DEV)
        self.x = ref.planted(ref.fixed_input(N_VARIANT, 128, 27 + seed)).to(DEV)
        self.f = ref.fixed_input(N_VARIANT, 128, 37 + seed).to(DEV)
        self.res = ref.fixed_input(N_VARIANT, 128, 47 + seed).to(DEV) if has_res else None
        self.truth, self.torch32 = self.ref(self.x, self.f, self.res, self.sd64), self.ref(self.x, self.f, self.res, self.sd)
        self.native = self.run(self.x, self.f, self.res)
        self.bound = bound_of(self.truth, self.torch32)
        self.ordinary = bound_of(self.truth[PLANTED:], self.torch32[PLANTED:])
        self.width = 256 if self.mode == "cat" else 128

    def norm(self, sd):
        return (sd["norm.weight"], sd["norm.bias"]) if "norm.weight" in sd else None

    def ref(self, x, f, res, sd):
        dt = sd["output_proj.weight"].dtype
        with torch.no_grad():
            return ref.output_ref(x.to(dt), sd["output_proj.weight"], sd["output_proj.bias"], f.to(dt), self.mode,
                                  None if res is None else res.to(dt), self.norm(sd))

    def run(self, x, f, res):
        with torch.no_grad():
            return deformable_output(x, (self.sd["output_proj.weight"], self.sd["output_proj.bias"]), f, self.mode, res, self.norm(self.sd))

    def rows(self, n):
        return self.x[:n].contiguous(), self.f[:n].contiguous(), None if self.res is None else self.res[:n].contiguous()

    def check(self, what, got, truth):
        """Rows that are a prefix of the variant's own: all to the variant's bound, rows 4 .. to the ordinary rows' bound."""
        held(what, got, truth, self.bound)
        if truth.shape[0] > PLANTED:
            held(what + ", ordinary rows", got[PLANTED:], truth[PLANTED:], self.ordinary)

    def raw_call(self, x, f, res, n, out):
        sd = self.sd
        ps = (sd["output_proj.weight"], sd["output_proj.bias"], sd.get("norm.weight"), sd.get("norm.bias"))
        mode = {"none": 0, "add": 1, "cat": 2}[self.mode]
        _lib.call("gf_deform_output_forward", DEV, n, 128, mode, x, None if mode == 0 else f, ptr_table(ps), res, out)


@functools.lru_cache(maxsize=None)
def front(name):
    return Front(name)


@functools.lru_cache(maxsize=None)
def back(name):
    return Back(name)


def more_rows(t, count, seed):
    return torch.cat([t, ref.fixed_input(count - t.shape[0], 128, seed).to(DEV)])


@functools.lru_cache(maxsize=None)
def big_front(name):
    """The variant on big_rows() + 129 rows, whose first 1 000 are the variant's own: inputs, truth, native result (128-row kernel)."""
    c = front(name)
    n = big_rows() + 129
    f, e = more_rows(c.f, n, 91), None if c.e is None else more_rows(c.e, n, 92)
    return f, e, c.ref(f, e, c.sd64), c.run(f, e)


@functools.lru_cache(maxsize=None)
def big_back(name):
    c = back(name)
    n = big_rows() + 129
    x, f, res = more_rows(c.x, n, 93), more_rows(c.f, n, 94), None if c.res is None else more_rows(c.res, n, 95)
    return x, f, res, c.ref(x, f, res, c.sd64), c.run(x, f, res)


# ---- 1. values ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", list(FRONT))
def test_front_values(name, n):
    c = front(name)
    got = c.native if n == N_VARIANT else c.run(*c.rows(n))
    c.check(f"front {name} n={n}", got, [None if t is None else t[:n] for t in c.truth])


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", list(BACK))
def test_back_values(name, n):
    c = back(name)
    got = c.native if n == N_VARIANT else c.run(*c.rows(n))
    c.check(f"back {name} n={n}", got, c.truth[:n])


def test_values_many_tiles():
    """n = 40 000: 313 workgroups of 128 rows, more than the chip holds at once."""
    c = front("base")
    f, e = ref.fixed_input(40000, 128, 81).to(DEV), ref.fixed_input(40000, 128, 82).to(DEV)
    c.check("front base n=40000", c.run(f, e), c.ref(f, e, c.sd64), planted=False)
    b = back("none_res_norm")
    x, res = ref.fixed_input(40000, 128, 83).to(DEV), ref.fixed_input(40000, 128, 84).to(DEV)
    held("back none_res_norm n=40000", b.run(x, f, res), b.ref(x, f, res, b.sd64), b.ordinary)


@pytest.mark.parametrize("name", list(FRONT))
def test_front_two_kernels_give_the_same_bits(name):
    """Up to 32 rows per CU a workgroup owns 32 rows and its waves split the columns; beyond, a workgroup owns 128 rows.  Which one
    runs is a matter of speed: the variant's 1 000 rows alone (the first) and as a prefix of many (the second) agree bitwise."""
    c = front(name)
    f, e, truth, native = big_front(name)
    c.check(f"front {name} n={f.shape[0]}", native, truth)
    for got, want in zip(native, c.native):
        assert (got is None and want is None) or torch.equal(got[:N_VARIANT], want)


@pytest.mark.parametrize("name", list(BACK))
def test_back_two_kernels_give_the_same_bits(name):
    c = back(name)
    x, f, res, truth, native = big_back(name)
    c.check(f"back {name} n={x.shape[0]}", native, truth)
    assert torch.equal(native[:N_VARIANT], c.native)


@pytest.mark.parametrize("r", TILE_EDGES)
@pytest.mark.parametrize("name", ["solid", "nocam_base", "narrow"])
def test_front_tile_kernel_at_its_edges(name, r):
    """The 128-row kernel with r rows in its last tile: the prefix, and nothing written beyond n x width."""
    c = front(name)
    f, e, truth, native = big_front(name)
    n = big_rows() + r
    raw = torch.full((n * c.nw + 777,), SENTINEL, device=DEV)
    learned = torch.full((n * c.k3 + 777,), SENTINEL, device=DEV)
    c.raw_call(f, e, n, learned, raw)
    assert torch.equal(raw[:n * c.nw].view(n, c.nw), native[0][:n]) and bool((raw[n * c.nw:] == SENTINEL).all())
    assert torch.equal(learned[:n * c.k3].view(n, c.k3), native[1][:n]) and bool((learned[n * c.k3:] == SENTINEL).all())


@pytest.mark.parametrize("r", TILE_EDGES)
@pytest.mark.parametrize("name", ["cat", "none_res_norm"])
def test_back_tile_kernel_at_its_edges(name, r):
    c = back(name)
    x, f, res, truth, native = big_back(name)
    n = big_rows() + r
    out = torch.full((n * c.width + 777,), SENTINEL, device=DEV)
    c.raw_call(x, f, res, n, out)
    assert torch.equal(out[:n * c.width].view(n, c.width), native[:n]) and bool((out[n * c.width:] == SENTINEL).all())


def test_leading_shape():
    c = front("base")
    raw, learned = deformable_logits(c.f.view(2, 500, 128), c.e.view(2, 500, 128), *c.params())
    assert raw.shape == (2, 500, 208) and learned.shape == (2, 500, 6, 3)
    assert torch.equal(raw.view(1000, 208), c.native[0]) and torch.equal(learned.reshape(1000, 18), c.native[1])
    b = back("cat")
    out = deformable_output(b.x.view(4, 250, 128), (b.sd["output_proj.weight"], b.sd["output_proj.bias"]), b.f.view(4, 250, 128), "cat")
    assert out.shape == (4, 250, 256) and torch.equal(out.view(1000, 256), b.native)


def test_misaligned_inputs_are_cloned():
    c = front("solid")
    base = torch.zeros(N_VARIANT * 128 + 1, device=DEV)
    base[1:] = c.f.flatten()
    f = base[1:].view(N_VARIANT, 128)
    assert f.data_ptr() % 16 != 0
    got = c.run(f, c.e)
    assert torch.equal(got[0], c.native[0]) and torch.equal(got[1], c.native[1])


# ---- 2. invariants, bitwise -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["solid", "nocam_base"])
def test_front_two_calls_agree(name):
    c = front(name)
    again = c.run(c.f, c.e)
    assert torch.equal(again[0], c.native[0]) and (c.k3 == 0 or torch.equal(again[1], c.native[1]))


@pytest.mark.parametrize("name", ["cat", "none_res_norm"])
def test_back_two_calls_agree(name):
    c = back(name)
    assert torch.equal(c.run(c.x, c.f, c.res), c.native)


@pytest.mark.parametrize("i", [0, 127, 128, 999])
@pytest.mark.parametrize("name", ["base", "narrow"])
def test_front_a_row_alone_has_the_bits_it_has_among_many(name, i):
    """n = 1 against the row's place inside n = 1 000 and inside the 128-row kernel's many: first, last and a tile-edge position."""
    c = front(name)
    alone = c.run(c.f[i:i + 1].contiguous(), None if c.e is None else c.e[i:i + 1].contiguous())
    for got, small, big in zip(alone, c.native, big_front(name)[3]):
        assert torch.equal(got[0], small[i]) and torch.equal(got[0], big[i])


@pytest.mark.parametrize("i", [0, 127, 128, 999])
@pytest.mark.parametrize("name", ["add_norm", "cat"])
def test_back_a_row_alone_has_the_bits_it_has_among_many(name, i):
    c = back(name)
    alone = c.run(c.x[i:i + 1].contiguous(), c.f[i:i + 1].contiguous(), None if c.res is None else c.res[i:i + 1].contiguous())
    assert torch.equal(alone[0], c.native[i]) and torch.equal(alone[0], big_back(name)[4][i])


@pytest.mark.parametrize("name", list(FRONT))
def test_front_nothing_is_written_beyond_the_outputs(name):
    """Sentinel-filled tails behind ``raw[n Nw]`` and ``learned[n 3K]``, for every width."""
    c = front(name)
    for n in (1, 33, 129):
        raw = torch.full((n * c.nw + 777,), SENTINEL, device=DEV)
        learned = torch.full((n * c.k3 + 777,), SENTINEL, device=DEV)
        c.raw_call(c.f, c.e, n, learned, raw)
        assert torch.equal(raw[:n * c.nw].view(n, c.nw), c.native[0][:n]) and bool((raw[n * c.nw:] == SENTINEL).all())
        assert bool((learned[n * c.k3:] == SENTINEL).all())
        if c.k3:
            assert torch.equal(learned[:n * c.k3].view(n, c.k3), c.native[1][:n])


@pytest.mark.parametrize("name", list(BACK))
def test_back_nothing_is_written_beyond_the_output(name):
    c = back(name)
    for n in (1, 33, 129):
        out = torch.full((n * c.width + 777,), SENTINEL, device=DEV)
        c.raw_call(c.x, c.f, c.res, n, out)
        assert torch.equal(out[:n * c.width].view(n, c.width), c.native[:n]) and bool((out[n * c.width:] == SENTINEL).all())


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("where", ["f", "e"])
def test_front_a_nan_stays_in_its_row(where, big):
    c = front("base")
    f, e, _, native = big_front("base") if big else (c.f, c.e, None, c.native)
    f, e = f.clone(), e.clone()
    (f if where == "f" else e)[77, 100] = float("nan")
    raw, learned = c.run(f, e)
    keep = torch.arange(f.shape[0], device=DEV) != 77
    assert bool(torch.isnan(raw[77]).all()) and torch.equal(raw[keep], native[0][keep])
    assert torch.equal(learned[keep], native[1][keep])
    assert bool(torch.isnan(learned[77]).all()) if where == "f" else torch.equal(learned[77], native[1][77])    # learned reads f alone


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("name,where", [("none_res_norm", "x"), ("none_res_norm", "res"), ("add_norm", "f"), ("cat", "x"), ("cat", "f")])
def test_back_a_nan_stays_in_its_row(name, where, big):
    c = back(name)
    x, f, res, _, native = big_back(name) if big else (c.x, c.f, c.res, None, c.native)
    t = dict(x=x.clone(), f=f.clone(), res=None if res is None else res.clone())
    t[where][77, 5] = float("nan")
    got = c.run(t["x"], t["f"], t["res"])
    keep = torch.arange(x.shape[0], device=DEV) != 77
    assert torch.equal(got[keep], native[keep])
    if name == "cat":      # the NaN stays in its half of the row as well
        half = slice(0, 128) if where == "x" else slice(128, 256)
        assert bool(torch.isnan(got[77, half]).all() if where == "x" else torch.isnan(got[77, 128 + 5]))
    else:
        assert bool(torch.isnan(got[77]).all())


@pytest.mark.parametrize("big", [False, True])
def test_cat_right_half_is_the_instance_feature(big):
    c = back("cat")
    f, native = (big_back("cat")[1], big_back("cat")[4]) if big else (c.f, c.native)
    assert torch.equal(native[:, 128:], f)


def test_a_residual_of_zeros_changes_nothing():
    for name in ("none", "add"):
        c = back(name)
        assert torch.equal(c.run(c.x, c.f, torch.zeros_like(c.x)), c.native)


# ---- 3. graph capture -------------------------------------------------------------------------------------------------------

def test_graph_replay_equals_eager():
    """Both ops in one captured chain (front, then back on a slice of the front's output as a stand-in for the middle)."""
    c, b = front("base"), back("add_norm")
    f, e = c.f.clone(), c.e.clone()
    wfc, lfc = c.params()
    proj, norm = (b.sd["output_proj.weight"], b.sd["output_proj.bias"]), b.norm(b.sd)

    def chain():
        raw, learned = deformable_logits(f, e, wfc, lfc)
        return raw, learned, deformable_output(raw[:, :128].contiguous(), proj, f, "add", None, norm)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            chain()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = chain()
        for flip in (False, True):
            if flip:
                f.copy_(c.f.flip(0))
                e.copy_(c.e.flip(0))
            graph.replay()
            got = [o.clone() for o in outs]
            want = chain()
            assert all(torch.equal(g, w) for g, w in zip(got, want))
        assert torch.equal(got[0], c.native[0].flip(0))


# ---- 4. module --------------------------------------------------------------------------------------------------------------

PC_RANGE = [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0]
SHAPES = {
    "solid": dict(num_learnable_pts=2, residual_mode="cat", post=False),       # pts = 9
    "prob": dict(num_learnable_pts=6, residual_mode="none", post=True),        # pts = 13, "identity", "deformable", "add", "norm"
}


def _cameras(cams, wh=(1600.0, 864.0)):
    """A ring of pinhole cameras looking outwards: a point is seen by one or two of them."""
    pm = torch.eye(4).repeat(1, cams, 1, 1)
    K = torch.tensor([[1260.0, 0, wh[0] / 2], [0, 1260.0, wh[1] / 2], [0, 0, 1.0]])
    for c in range(cams):
        yaw = 2 * np.pi * c / cams
        R = torch.tensor([[-np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, -1.0], [np.cos(yaw), np.sin(yaw), 0.0]], dtype=torch.float32)
        pm[0, c, :3, :3] = K @ R
        pm[0, c, :3, 3] = K @ torch.tensor([0.0, 1.5, 0.0])
    return pm.to(DEV), torch.tensor([[list(wh)] * cams], device=DEV)


@functools.lru_cache(maxsize=None)
def scene(A=300, cams=6, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    maps = [torch.randn(1, cams, 128, h, w, generator=g).to(DEV) for h, w in synthetic.DAF_LEVELS]
    anchor = torch.randn(1, A, 28, generator=g)
    anchor[..., :3] *= 1.5
    inst, emb = torch.randn(1, A, 128, generator=g), torch.randn(1, A, 128, generator=g)
    pm, wh = _cameras(cams)
    return dict(maps=maps, anchor=anchor.to(DEV), inst=inst.to(DEV), emb=emb.to(DEV), pm=pm, wh=wh)


def module_of(name, seed=0):
    s = SHAPES[name]
    cfg = dict(embed_dims=128, num_groups=4, num_levels=4, num_cams=6, use_deformable_func=True, use_camera_embed=True,
               residual_mode=s["residual_mode"],
               kps_generator=dict(type="SparseGaussian3DKeyPointsGenerator", num_learnable_pts=s["num_learnable_pts"], fix_scale=ref.FIX7,
                                  pc_range=PC_RANGE, scale_range=[0.08, 0.64]))
    sd = ref.fixed_weights(ref.shapes(cfg, norm=s["post"]), seed=seed + 11)
    m = DeformableFeatureAggregation(**cfg)
    m.load_state_dict(ref.module_state(sd), strict=True)
    return m.to(DEV).eval(), cfg, sd


@pytest.mark.parametrize("name", list(SHAPES))
def test_module_native_route_against_the_truth(name, spy):
    """E = 128, A = 300 anchors on the synthetic pyramid: the native route held to the float64 module restatement, the module's
    own torch-dense route (``native_dense = False``) as the yardstick; with the prob shape the encoder's "add", "norm" are folded
    in through ``residual=`` / ``norm=``."""
    m, cfg, sd = module_of(name)
    s = scene()
    post = SHAPES[name]["post"]
    norm = (sd["norm.weight"].to(DEV), sd["norm.bias"].to(DEV)) if post else None
    kw = dict(residual=s["inst"], norm=norm) if post else {}
    metas = dict(projection_mat=s["pm"], image_wh=s["wh"])
    with torch.no_grad():
        native = m(s["inst"], s["anchor"], s["emb"], s["maps"], metas, **kw)
        assert spy == ["gf_feature_maps_format", "gf_deform_logits_forward", "gf_key_points", "gf_daf_fused_forward", "gf_deform_output_forward"]
        del spy[:]
        m.native_dense = False
        dense = m(s["inst"], s["anchor"], s["emb"], s["maps"], metas, **kw)
        assert "gf_deform_logits_forward" not in spy and "gf_deform_output_forward" not in spy
        d = lambda t: t.double()
        truth = ref.module_ref(ref.cast(sd, torch.float64, DEV), cfg, d(s["inst"]), d(s["anchor"]), d(s["emb"]), [d(f) for f in s["maps"]],
                               d(s["pm"]), d(s["wh"]), residual=d(s["inst"]) if post else None)
        # the formatted triple is taken as it is
        from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF
        m.native_dense = True
        assert torch.equal(m(s["inst"], s["anchor"], s["emb"], DAF.feature_maps_format(s["maps"]), metas, **kw), native)
    assert native.shape == (1, 300, 256 if cfg["residual_mode"] == "cat" else 128)
    held(f"module {name}", native, truth, bound_of(truth, dense))


def test_module_training_and_dropout_take_the_torch_layers(spy):
    m, cfg, sd = module_of("solid")
    s = scene()
    metas = dict(projection_mat=s["pm"], image_wh=s["wh"])
    out = m(s["inst"], s["anchor"], s["emb"], s["maps"], metas)               # grad mode on, parameters require grad
    assert out.requires_grad and "gf_deform_logits_forward" not in spy and "gf_daf_fused_forward_masked" in spy
    out.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    del spy[:]
    m.proj_drop.p = 0.1
    m.train()
    with torch.no_grad():
        m(s["inst"], s["anchor"], s["emb"], s["maps"], metas)
        assert "gf_deform_output_forward" not in spy
        del spy[:]
        m.eval()
        m(s["inst"], s["anchor"], s["emb"], s["maps"], metas)
        assert "gf_deform_output_forward" in spy


def test_module_at_the_fixture_s_width():
    """E = 32 is not native: the torch dense layers around the native middle reproduce what the reference's module computed,
    output and gradients (the bounds of tests/test_ref_callers.py)."""
    d = np.load(GOLDEN)
    t = lambda k, g=False: torch.from_numpy(d[k]).to(DEV).requires_grad_(g)
    cfg = dict(ref.FIXTURE_CONFIG, kps_generator=dict(ref.FIXTURE_CONFIG["kps_generator"]))
    m = DeformableFeatureAggregation(**cfg)
    m.load_state_dict({k[len("param_"):]: torch.from_numpy(d[k]) for k in d.files if k.startswith("param_")}, strict=True)
    m.to(DEV).eval()

    def rel(got, want, what, tol):
        got, want = got.detach().double().cpu().numpy(), np.asarray(want, np.float64)
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-6)
        print(f"{what}: {err:.3e} (tolerance {tol})")
        assert got.shape == want.shape and np.isfinite(got).all() and err <= tol, (what, err)
    metas = dict(projection_mat=t("projection_mat"), image_wh=t("image_wh"))
    maps = [t(f"feature_map{i}") for i in range(3)]
    with torch.no_grad():
        rel(m(t("instance_feature"), t("anchor"), t("anchor_embed"), maps, metas), d["output"], "output, no grad", 1e-4)
    inst, emb, anchor = t("instance_feature", True), t("anchor_embed", True), t("anchor", True)
    maps = [t(f"feature_map{i}", True) for i in range(3)]
    out = m(inst, anchor, emb, maps, metas)
    rel(out, d["output"], "output", 1e-4)
    (out * t("out_weight")).sum().backward()
    for k, leaf in (("instance_feature", inst), ("anchor_embed", emb), ("anchor", anchor)):
        rel(leaf.grad, d["grad_" + k], "grad_" + k, 2e-3)
    for i, f in enumerate(maps):
        rel(f.grad, d[f"grad_feature_map{i}"], f"grad_feature_map{i}", 2e-3)
    for k, p in m.named_parameters():
        rel(p.grad, d["grad_param_" + k], "grad_param_" + k, 2e-3)


def test_attention_dropout_draws_the_reference_s_mask():
    """Training with ``attn_drop > 0``: the output is ``deformable_fused`` with the mask ``torch.rand(...) > attn_drop`` drawn at the
    same generator state, between the module's own torch layers."""
    m, cfg, sd = module_of("solid")
    m.attn_drop = 0.15
    m.train()
    s = scene()
    metas = dict(projection_mat=s["pm"], image_wh=s["wh"])
    torch.manual_seed(5)
    out = m(s["inst"], s["anchor"], s["emb"], s["maps"], metas)
    torch.manual_seed(5)
    mask = torch.rand(1, 300, 6, 4, 9, 4, device=DEV) > 0.15
    from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF
    kp = m.kps_generator(s["anchor"], s["inst"])
    ra = m.weights_fc(s["inst"] + s["emb"]).reshape(1, 300, 4, 9, 4)
    rc = F.linear(m.camera_encoder(s["pm"][:, :, :3].reshape(1, 6, -1)), m.weights_fc.weight).reshape(1, 6, 4, 9, 4)
    feats = deformable_fused(kp, s["pm"], s["wh"], *DAF.feature_maps_format(s["maps"]), raw_anchor=ra, raw_cam=rc, weight_mask=mask)
    want = torch.cat([m.output_proj(feats), s["inst"]], dim=-1)
    assert not bool(mask.all()) and torch.equal(out, want)
    m.eval()
    with torch.no_grad():
        assert not torch.equal(m(s["inst"], s["anchor"], s["emb"], s["maps"], metas), out)      # no mask outside training


def test_entry_points_refuse_on_the_device_too():
    c, b = front("solid"), back("cat")
    fail = r"failed \(code -1\): .*"
    raw, learned = torch.empty(N_VARIANT * 144, device=DEV), torch.empty(N_VARIANT * 6, device=DEV)
    with pytest.raises(RuntimeError, match=fail + "raw aliases an input"):
        c.raw_call(c.f, c.e, N_VARIANT, learned, c.e)
    with pytest.raises(RuntimeError, match=fail + "out aliases an input"):
        b.raw_call(b.x, b.f, None, 500, b.f)
    c.raw_call(c.f, c.e, 0, learned, raw)      # GF_OK, no launch
    with pytest.raises(RuntimeError, match="without a native backward"):
        deformable_logits(c.f.clone().requires_grad_(True), c.e, *c.params())
