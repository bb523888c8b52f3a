"""The sparse convolution stage's training entries without a GPU (``gf_subm_stage_train_sizes``,
``gf_subm_conv_apply_epilogue_train``, ``gf_subm_stage_backward``, ``gf_subm_conv_apply_stage_backward``): every refusal comes
before any HIP call, on host buffers, names the offending value and leaves the outputs untouched; the size query; the block's
``native_training`` switch; and ``tests/subm_stage_ref.py`` pinned against torch's float64 autograd with its own masks."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import row_ref
import subm_stage_ref as ref
from gaussianformer_amd import _lib
from gaussianformer_amd.sparse_conv import SparseConv3D, subm_stage

GF_EINVAL, GF_EWORKSPACE = -1, -2
N, B, SHAPE, K, CIN, COUT, PAIRS = 8, 1, (4, 4, 4), 3, 32, 32, 8
SENTINEL = 12345.0
ENTRIES = ("gf_subm_conv_apply_epilogue_train", "gf_subm_stage_backward", "gf_subm_conv_apply_stage_backward")


def sizes(n, cout):
    return _lib.train_sizes("gf_subm_stage_train_sizes", n, cout)


class Host:
    """Host buffers of one call of each entry, every one its own allocation; the outputs hold a sentinel."""

    def __init__(self):
        lib = _lib.load()
        z, s = torch.zeros, lambda *shape: torch.full(shape, SENTINEL)
        self.feat, self.weight = z(N, CIN), z(K ** 3, CIN, COUT)
        self.tables = z(int(lib.gf_subm_tables_bytes(N, B, *SHAPE, K)), dtype=torch.uint8)
        self.pair_in, self.partial = z(PAIRS, dtype=torch.int32), z(PAIRS, COUT)
        self.nscratch = int(lib.gf_subm_apply_scratch_bytes(N, CIN))
        self.scratch = z(self.nscratch, dtype=torch.uint8)
        # (every input begins an allocation of at least [N, COUT] floats: an output pointed at it overlaps it and nothing else)
        self.bias, self.residual, self.ln_weight, self.ln_bias = z(N, COUT).view(-1)[:COUT + 4], z(N, COUT), z(N, COUT)[0], z(N, COUT)[0]
        self.pre, self.grad_out = z(N, COUT), z(N, COUT)
        self.nwork = sizes(N, COUT)[1]
        self.workspace = z(max(self.nwork, N * COUT * 4), dtype=torch.uint8)
        self.out, self.pre_out, self.grad_pre = s(N, COUT), s(N, COUT), s(N, COUT)
        self.grad_ln_weight, self.grad_ln_bias, self.grad_bias = s(COUT), s(COUT), s(COUT + 4)

    def call(self, entry, relu=0, **over):
        """``entry`` on the buffers' addresses; ``over``: an address (or ``None``) in place of a buffer's, or another size."""
        a = {k: v.data_ptr() for k, v in vars(self).items() if isinstance(v, torch.Tensor)}
        a.update(N=N, Cin=CIN, Cout=COUT, K=K, nscratch=self.nscratch, nwork=self.nwork)
        a.update(over)
        lib = _lib.load()
        conv = (a["N"], B, *SHAPE, a["K"], a["Cin"], a["Cout"], PAIRS, a["feat"], a["weight"], a["tables"], a["pair_in"], a["partial"])
        back = (a["ln_weight"], a["ln_bias"], relu, a["grad_pre"], a["grad_ln_weight"], a["grad_ln_bias"], a["grad_bias"], a["workspace"],
                a["nwork"], None)
        if entry == "gf_subm_conv_apply_epilogue_train":
            rc = lib.gf_subm_conv_apply_epilogue_train(*conv, a["out"], a["scratch"], a["nscratch"], a["bias"], a["residual"],
                                                       a["ln_weight"], a["ln_bias"], relu, a["pre_out"], None)
        elif entry == "gf_subm_stage_backward":
            rc = lib.gf_subm_stage_backward(a["N"], a["Cout"], a["pre"], a["grad_out"], *back)
        else:
            rc = lib.gf_subm_conv_apply_stage_backward(*conv, a["scratch"], a["nscratch"], a["pre"], *back)
        return rc, lib.gf_last_error().decode()

    def untouched(self):
        return all(bool((t == SENTINEL).all()) for t in (self.out, self.pre_out, self.grad_pre, self.grad_ln_weight, self.grad_ln_bias,
                                                         self.grad_bias))


def refused(h, entry, needle, code=GF_EINVAL, **kw):
    rc, msg = h.call(entry, **kw)
    assert rc == code, (entry, rc, msg)
    assert "subm" in msg and needle in msg, (entry, msg)
    assert h.untouched(), entry


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_or_half_present_norm_pair(entry):
    h = Host()
    refused(h, entry, "ln_bias", ln_bias=None)
    refused(h, entry, "ln_weight", ln_weight=None)
    refused(h, entry, "ln_weight", ln_weight=None, ln_bias=None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_relu_outside_0_1(entry):
    h = Host()
    refused(h, entry, "relu = 2", relu=2)
    refused(h, entry, "relu = -1", relu=-1)


MISALIGNED = {"gf_subm_conv_apply_epilogue_train": ["bias", "residual", "ln_weight", "ln_bias", "out", "pre_out"],
              "gf_subm_stage_backward": ["pre", "grad_out", "ln_weight", "ln_bias", "grad_pre", "grad_ln_weight", "grad_ln_bias", "grad_bias",
                                         "workspace"],
              "gf_subm_conv_apply_stage_backward": ["pre", "ln_weight", "ln_bias", "grad_pre", "grad_ln_weight", "grad_ln_bias", "grad_bias",
                                                    "workspace", "partial"]}


@pytest.mark.parametrize("entry,which", [(e, w) for e in ENTRIES for w in MISALIGNED[e]])
def test_a_misaligned_pointer(entry, which):
    h = Host()
    name = "pre" if which == "pre_out" else which
    refused(h, entry, f"{name} = ", **{which: getattr(h, which).data_ptr() + 4})
    assert "16-byte aligned" in h.call(entry, **{which: getattr(h, which).data_ptr() + 4})[1]


OVERLAPS = {"gf_subm_stage_backward": ["pre", "grad_out", "ln_weight", "ln_bias", "workspace"],
            "gf_subm_conv_apply_stage_backward": ["pre", "feat", "weight", "ln_weight", "ln_bias", "workspace", "partial", "scratch"]}


@pytest.mark.parametrize("entry,which", [(e, w) for e in OVERLAPS for w in OVERLAPS[e]])
def test_grad_pre_overlapping_an_input(entry, which):
    h = Host()
    name = "features" if which == "feat" else which
    refused(h, entry, f"aliases {name}", grad_pre=getattr(h, which).data_ptr())


def test_grad_pre_overlapping_the_tail_of_pre():
    h = Host()
    rows = torch.full((2 * N - 1, COUT), SENTINEL)       # grad_pre = rows[:N], pre = rows[N - 1:]: one row shared
    for entry in ENTRIES[1:]:
        rc, msg = h.call(entry, grad_pre=rows.data_ptr(), pre=rows[N - 1:].data_ptr())
        assert rc == GF_EINVAL and "aliases pre" in msg and bool((rows == SENTINEL).all())


@pytest.mark.parametrize("which", ["residual", "feat", "weight", "bias", "ln_weight", "ln_bias", "partial", "scratch"])
def test_the_saving_forwards_outputs_overlapping_an_input(which):
    h = Host()
    name = "features" if which == "feat" else which
    refused(h, ENTRIES[0], f"out = ", out=getattr(h, which).data_ptr())
    refused(h, ENTRIES[0], f"aliases {name}", pre_out=getattr(h, which).data_ptr())
    refused(h, ENTRIES[0], "aliases out", pre_out=h.out.data_ptr())
    refused(h, ENTRIES[0], "pre is null", pre_out=None)


@pytest.mark.parametrize("entry", ENTRIES[1:])
def test_a_short_workspace(entry):
    h = Host()
    assert h.nwork > 0
    refused(h, entry, "workspace", code=GF_EWORKSPACE, nwork=h.nwork - 16)
    refused(h, entry, "workspace", code=GF_EWORKSPACE, nwork=0)
    refused(h, entry, "workspace is null", workspace=None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_unsupported_channels_and_null_pointers(entry):
    h = Host()
    refused(h, entry, "channels", Cout=48)
    if entry != "gf_subm_stage_backward":
        refused(h, entry, "channels", Cin=48)
        refused(h, entry, "kernel size", K=4)
        refused(h, entry, "null pointer", feat=None)
        refused(h, entry, "scratch", scratch=None)
        refused(h, entry, "scratch", nscratch=h.nscratch - 16)
    if entry != ENTRIES[0]:
        refused(h, entry, "null pointer", pre=None)
        refused(h, entry, "grad_ln_weight", grad_ln_weight=None)
        refused(h, entry, "N = -1", N=-1)
    if entry == "gf_subm_stage_backward":
        refused(h, entry, "grad_out", grad_out=None)


def test_no_rows_is_ok_without_a_device():
    """The saving forward launches nothing for N == 0.  (The backward entries zero-fill the parameter gradients, which takes a
    device: tests/test_subm_stage_train_gpu.py.)"""
    h = Host()
    rc, _ = h.call(ENTRIES[0], N=0, relu=1)
    assert rc == 0 and h.untouched()


def test_train_sizes():
    assert sizes(0, 128) == (0, 0) and sizes(0, 32) == (0, 0)
    for cout in (32, 64, 128):
        rows = 256 // (cout // 4)
        last = (0, 0)
        for n in (1, rows - 1, rows, rows + 1, 300, 3001, 25600, 144000):
            saved, work = sizes(n, cout)
            assert saved >= n * cout * 4 and saved % 256 == 0
            assert work >= -(-n // rows) * 3 * cout * 4 and work % 256 == 0       # one partial triple per workgroup of `rows` rows
            assert saved >= last[0] and work >= last[1]
            last = (saved, work)
    lib = _lib.load()
    saved, work = ctypes.c_size_t(7), ctypes.c_size_t(7)
    ptrs = (ctypes.addressof(saved), ctypes.addressof(work))
    for args, needle in (((8, 48, *ptrs), "channels"), ((-1, 32, *ptrs), "N = -1"), ((8, 32, None, ptrs[1]), "null pointer"),
                         ((8, 32, ptrs[0], None), "null pointer")):
        assert lib.gf_subm_stage_train_sizes(*args) == GF_EINVAL and needle in lib.gf_last_error().decode()
        assert saved.value == 7 and work.value == 7


def test_native_training_is_an_attribute_off_by_default():
    kw = dict(pc_range=[-5.0, -5.0, -2.5, 5.0, 5.0, 2.5], grid_size=[2.0, 2.0, 1.0], kernel_size=3, use_multi_layer=True)
    assert SparseConv3D.native_training is False
    assert "native_training" not in inspect.signature(SparseConv3D.__init__).parameters
    m = SparseConv3D(32, 32, **kw)
    assert m.native_training is False
    m.native_training = True
    assert not any("native_training" in k for k in m.state_dict())
    assert SparseConv3D(32, 32, **kw).native_training is False and SparseConv3D.native_training is False
    assert SparseConv3D(32, 32, native_training=True, **kw).native_training is False      # (an unknown key, ignored like the others)
    # CPU tensors are not the native route's: the torch layers' own refusal of a CPU rulebook, not a stage entry's
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 4, 32, requires_grad=True), torch.zeros(1, 4, 11))


def test_what_subm_stage_refuses_itself():
    class RB:
        out_range, N = None, 4
    with pytest.raises(ValueError, match="norm is required"):
        subm_stage(torch.zeros(4, 32), RB(), torch.zeros(27, 32, 32))
    with pytest.raises(ValueError, match="norm must be"):
        subm_stage(torch.zeros(4, 32), RB(), torch.zeros(27, 32, 32), norm=nn.LayerNorm(32, eps=1e-6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        subm_stage(torch.zeros(4, 32), RB(), torch.zeros(27, 32, 32), norm=(torch.ones(32), torch.zeros(32)))
    RB.out_range = (0, 2)
    with pytest.raises(RuntimeError, match="inference-only"):
        subm_stage(torch.zeros(4, 32), RB(), torch.zeros(27, 32, 32), norm=(torch.ones(32), torch.zeros(32)))


# ---- the float64 restatement against torch's own float64 autograd ---------------------------------------------------------------

def _torch_stage(pre, gamma, beta, relu):
    y = F.layer_norm(pre, (pre.shape[1],), gamma, beta, 1e-5)
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("relu", [True, False])
def test_the_stage_restatement_is_torchs_on_a_kink_free_draw(relu):
    cout, n = 32, 65
    pre = row_ref.fixed_input(n, cout, 3).double() * 1.7 + 0.2
    sd = row_ref.fixed_weights({"ln.weight": (cout,), "ln.bias": (cout,)}, 700, dtype=torch.float64)
    gamma, beta = sd["ln.weight"], sd["ln.bias"]
    xhat, u = ref.stage_parts(pre, gamma, beta)
    keep = ref.outside_margin(u, xhat, gamma, beta, 1e-5).all(dim=1)
    assert int(keep.sum()) >= n - 2
    pre = pre[keep]
    cot = row_ref.output_weights(pre.shape)
    mask = "own" if relu else None
    mine = ref.stage_backward(pre, cot, gamma, beta, mask)
    given = ref.stage_backward(pre, cot, gamma, beta, (ref.stage_parts(pre, gamma, beta)[1] > 0).double() if relu else None)
    leaves = [t.clone().requires_grad_(True) for t in (pre, gamma, beta)]
    want = torch.autograd.grad((_torch_stage(*leaves, relu) * cot).sum(), leaves)
    for got in (mine, given):
        for k, w in zip(("g_pre", "ln_weight", "ln_bias"), want):
            assert torch.allclose(got[k], w, rtol=1e-10, atol=1e-11 * float(w.abs().max())), k
        assert torch.allclose(got["bias"], want[0].sum(0), rtol=1e-10, atol=1e-11 * float(want[0].abs().max()))
    if relu:   # a flipped mask entry is another function: the masks are inputs, not recomputed
        flipped = (ref.stage_parts(pre, gamma, beta)[1] <= 0).double()
        assert not torch.allclose(ref.stage_backward(pre, cot, gamma, beta, flipped)["g_pre"], want[0])


@pytest.mark.parametrize("multi,proj,last", [(True, True, False), (True, True, True), (False, False, False), (False, True, False)])
def test_the_block_restatement_is_torchs_layers(multi, proj, last):
    """The block with its own masks against the same layers written with torch's modules' functions, float64, 40 points."""
    from oracle.subm_ref import subm_conv3d_dense
    E, bs, g, shape, k = 32, 2, 20, (3, 3, 3), 3
    rng = np.random.default_rng(8)
    idx = torch.from_numpy(np.concatenate([np.repeat(np.arange(bs), g)[:, None], rng.integers(0, 3, (bs * g, 3))], 1).astype(np.int32))
    shapes = {key: ((k ** 3, E, E) if key.startswith("conv") and key.endswith("weight") else (E, E) if key == "proj.weight" else (E,))
              for key in ref.block_keys(multi, proj)}
    p = row_ref.fixed_weights(shapes, 800, dtype=torch.float64)
    for key in p:
        if key.startswith("conv") and key.endswith("weight"):
            p[key] = p[key] * 0.2
    x, res = row_ref.fixed_input(bs * g, E, 1).double().unflatten(0, (bs, g)), row_ref.fixed_input(bs * g, E, 2).double().unflatten(0, (bs, g))
    rep = None
    if last:
        key = (idx[:, 0] * 27 + idx[:, 1] * 9 + idx[:, 2] * 3 + idx[:, 3]).tolist()
        rep = torch.tensor([[float(all(key[j] != key[i] for j in range(i + 1, len(key))))] for i in range(len(key))], dtype=torch.float64)
        assert 0 < rep.sum() < len(key)

    def torch_block(x_, r_, q):
        out = x_.flatten(0, 1)
        for s in range(3 if multi else 1):
            out = subm_conv3d_dense(out * rep if last else out, idx, q[f"conv{s}.weight"], bs, shape, k)
            if multi:
                out = torch.relu(F.layer_norm(out + q[f"conv{s}.bias"], (E,), q[f"ln{s}.weight"], q[f"ln{s}.bias"], 1e-5))
        if proj:
            out = F.linear(out, q["proj.weight"], q["proj.bias"])
        return F.layer_norm(out.unflatten(0, (bs, g)) + r_, (E,), q["norm.weight"], q["norm.bias"], 1e-5)
    cot = row_ref.output_weights((bs, g, E), torch.float32).double()      # (block_gradients': the float32-rounded weights)
    want = row_ref.scalar_gradients(torch_block, {"x": x, "residual": res}, p, cotangent=cot)
    mine = ref.block_gradients(x, res, p, idx, bs, shape, k, "own", rep)
    _, seen = ref.block(x, res, p, idx, bs, shape, k, "own", rep, with_stages=True)
    given = ref.block_gradients(x, res, p, idx, bs, shape, k, [(u > 0).double() for _, u, _ in seen] if multi else None, rep)
    assert set(mine) == set(want) == set(given) and len(seen) == (3 if multi else 0)
    for got in (mine, given):
        for key, w in want.items():
            assert float(w.abs().max()) > 0, key
            assert torch.allclose(got[key], w, rtol=1e-9, atol=1e-10 * float(w.abs().max())), key
