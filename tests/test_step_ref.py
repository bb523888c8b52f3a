"""CPU pins of the new pieces of tests/step_ref.py (the float64 restatement of the chained training step, tools/bench_step.py):
the sparse evaluation of the submanifold convolution and the pair-list splat against the dense definitions of oracle/, and the
stage-wise reverse-mode step against plain autograd over the whole chain at a tiny size."""
import pytest
import torch

import step_ref
from oracle.dense_ref import splat_dense
from oracle.subm_ref import subm_conv3d_dense


def _close(got, want, tol=1e-12, what=""):
    scale = float(want.abs().max().clamp(min=1e-300))
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:g} x max|ref| {scale:.3e}"


# ---- subm_conv_sparse against subm_conv3d_dense -----------------------------------------------------------------------------

def _points(g, N, batch, shape, crowd):
    X, Y, Z = shape
    idx = torch.stack([torch.randint(0, batch, (N,), generator=g), torch.randint(0, X, (N,), generator=g),
                       torch.randint(0, Y, (N,), generator=g), torch.randint(0, Z, (N,), generator=g)], 1)
    dup = torch.randint(0, N, (int(N * crowd),), generator=g)
    idx[torch.randint(0, N, (dup.shape[0],), generator=g)] = idx[dup]              # crowded cells: several points share one
    idx[:3, 1] = torch.tensor([-1, X, X + 4])                                        # outside the grid (inactive)
    idx[3, 3] = Z
    idx[4, 0] = batch                                                                 # batch index outside [0, batch)
    return idx.to(torch.int32)


@pytest.mark.parametrize("K", [3, 5])
def test_subm_conv_sparse_matches_dense(K):
    g = torch.Generator().manual_seed(K)
    shape, batch, cin, cout = (7, 6, 5), 2, 6, 4
    idx = _points(g, 400, batch, shape, crowd=0.3)
    cells = idx[:, 0].long() * 1000 + idx[:, 1].long() * 100 + idx[:, 2].long() * 10 + idx[:, 3].long()
    assert int(torch.unique(cells, return_counts=True)[1].max()) >= 3            # some cell holds three points or more
    feat = torch.randn(400, cin, generator=g, dtype=torch.float64)
    weight = torch.randn(K ** 3, cin, cout, generator=g, dtype=torch.float64)
    gout = torch.randn(400, cout, generator=g, dtype=torch.float64)
    res = []
    for fn in (step_ref.subm_conv_sparse, subm_conv3d_dense):
        f, w = feat.clone().requires_grad_(True), weight.clone().requires_grad_(True)
        out = fn(f, idx, w, batch, shape, K)
        out.backward(gout)
        res.append((out.detach(), f.grad, w.grad))
    for a, b, what in zip(res[0], res[1], ("out", "grad feat", "grad weight")):
        _close(a, b, what=f"K={K} {what}")
    assert bool((res[0][0][:5] == 0).all()) and bool((res[0][1][:5] == 0).all())   # inactive points: zeros both ways


# ---- splat_pairs against splat_dense ------------------------------------------------------------------------------------------

H, W, D, CELL = 9, 8, 6, 0.5
PC_MIN = (-2.0, -2.0, -1.5)


def _grid():
    ax = [torch.arange(n, dtype=torch.float64) for n in (H, W, D)]
    pi = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    return (pi + 0.5) * CELL + torch.tensor(PC_MIN, dtype=torch.float64), pi.to(torch.int32)


def _gaussians(g, mode, uniform_cut):
    P = 40
    mi = torch.stack([torch.randint(0, n, (P,), generator=g) for n in (H, W, D)], 1)
    mi[:6] = torch.tensor([[0, 0, 0], [H - 1, W - 1, D - 1], [0, W - 1, 2], [H - 1, 0, D - 1], [4, 0, 0], [2, 3, D - 1]])
    means = (mi.double() + torch.rand(P, 3, generator=g, dtype=torch.float64)) * CELL + torch.tensor(PC_MIN, dtype=torch.float64)
    if mode == "per_axis":
        radii = torch.randint(0, 4, (P, 3), generator=g)
    else:
        radii = torch.randint(0 if mode == "scalar" else 1, 4, (P,), generator=g)
    radii[-1] = 40 if radii.dim() == 1 else 40                                       # a whole-grid Gaussian (the "empty" one)
    q = torch.randn(P, 4, generator=g, dtype=torch.float64)
    s = torch.rand(P, 3, generator=g, dtype=torch.float64) * 0.6 + 0.15
    s[-1] = torch.tensor([6.0, 6.0, 4.0])
    cov6 = step_ref.pack6(step_ref.covariance_inverse(s, q))
    opa = torch.rand(P, generator=g, dtype=torch.float64) * 0.9 + 0.1
    sem = torch.rand(P, 18, generator=g, dtype=torch.float64)
    if uniform_cut:
        # the voxels x >= 7 only the whole-grid Gaussian reaches, made faint: their probability sum is below the 1e-9 cut
        keep = (mi[:, 0] + radii.reshape(P, -1)[:, 0] <= 6) | (torch.arange(P) == P - 1)
        opa = torch.where(keep, opa, torch.zeros_like(opa))
        opa[-1] = 1e-12
    return means, mi.to(torch.int32), opa, sem, radii.to(torch.int32), cov6


@pytest.mark.parametrize("variant,mode", [("base", "scalar"), ("base", "per_axis"), ("prob", "clamped"), ("prob", "per_axis")])
def test_splat_pairs_matches_dense(variant, mode):
    g = torch.Generator().manual_seed(hash((variant, mode)) % 1000)
    pts, pi = _grid()
    means, mi, opa, sem, radii, cov6 = _gaussians(g, mode, uniform_cut=variant == "prob")
    lo, hi = step_ref.box_bounds(mi, radii, H, W, D)
    assert bool(((lo == 0) & (hi == torch.tensor([H, W, D]))).all(1)[-1])           # the whole-grid box
    assert bool((lo == 0).any(0).all()) and bool((hi == torch.tensor([H, W, D])).any(0).all())   # clipped at every face
    res = []
    for fn in (step_ref.splat_pairs, splat_dense):
        leaves = [t.clone().requires_grad_(True) for t in (means, opa, sem, cov6)]
        m, o, s, c = leaves
        out = fn(variant, pts, pi, m, mi, o, s, radii, c, H, W, D)
        outs = (out,) if variant == "base" else out
        gg = torch.Generator().manual_seed(1)
        loss = sum((x * torch.randn(x.shape, generator=gg, dtype=torch.float64)).sum() for x in outs[:3])
        loss.backward()
        res.append([x.detach() for x in outs] + [t.grad for t in leaves])
    if variant == "prob":
        ps = res[1][3]
        under = ps <= step_ref.CUT
        assert int(under.sum()) > 0 and int((~under).sum()) > 0                        # both sides of the cut are present
        assert bool((res[0][0][under] == step_ref.uniform_row(18, torch.float64, "cpu")).all())
    names = ["logits", "bin_logits", "density", "prob_sum"] if variant == "prob" else ["logits"]
    for a, b, what in zip(res[0], res[1], names + ["grad means", "grad opacity", "grad semantics", "grad cov6"]):
        _close(a, b, what=f"{variant}/{mode} {what}")


# ---- the restatement at a tiny step ---------------------------------------------------------------------------------------

def _bench_step():
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import bench_step
    return bench_step


def _tiny(head, A=64, C=16, seed=0):
    """bench_step.build's leaves and constants at a tiny size: a 10 x 10 x 4 m grid of 0.5 m cells, six cameras, two small maps."""
    bs = _bench_step()
    g = torch.Generator().manual_seed(seed)
    cams, L, pts, G = 6, 2, 9, 4
    levels = [(9, 16), (5, 8)]
    pc = [-5.0, -5.0, -2.0, 5.0, 5.0, 2.0]
    grid = (20, 20, 8)
    blocks = [dict(spconv=torch.randn(125, C, C, generator=g) * 0.05, fc_weight=torch.randn(cams * L * pts * G, C, generator=g) * 0.3,
                   fc_bias=torch.randn(cams * L * pts * G, generator=g) * 0.1, key_offsets=torch.randn(pts, 3, generator=g) * 0.5)
              for _ in range(2)]
    named = dict(anchor=torch.randn(1, A, 11, generator=g), sem_raw=torch.randn(1, A, 18 if head == "plain" else 17, generator=g),
                 feat0=torch.randn(1, A, C, generator=g), maps=[torch.randn(1, cams, C, h, w, generator=g) for h, w in levels],
                 blocks=blocks)
    empty = None
    if head == "empty":
        named["empty_scalar"] = torch.tensor([10.0])
        empty = dict(mean=[0.0, 0.0, 0.0], scale=[10.0, 10.0, 4.0])
    pm, wh = bs.cameras("cpu")
    N = grid[0] * grid[1] * grid[2]
    ax = [torch.arange(n, dtype=torch.float32) for n in grid]
    pts_ = ((torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3) + 0.5) * 0.5 + torch.tensor(pc[:3]))[None]
    targets = [torch.randn(N, 18, generator=g)] + ([torch.randn(N, generator=g), torch.randn(N, generator=g)] if head == "prob" else [])
    const = dict(head=head, pm=pm, wh=wh, pts=pts_, targets=targets, grid=grid, cell=0.5, pc_range=pc, levels=levels,
                 scale_multiplier=3, kernel_size=5, groups=G, key_pts=pts, empty_args=empty)
    return named, const


def _flat(grads):
    out = [("anchor", grads["anchor"]), ("sem_raw", grads["sem_raw"]), ("feat0", grads["feat0"])]
    out += [(f"map{i}", m) for i, m in enumerate(grads["maps"])]
    for bi, b in enumerate(grads["blocks"]):
        out += [(f"block{bi}.{k}", v) for k, v in b.items()]
    if "empty_scalar" in grads:
        out.append(("empty_scalar", grads["empty_scalar"]))
    return out


@pytest.mark.parametrize("head", ["plain", "empty", "prob"])
def test_stagewise_step_matches_whole_chain_autograd(head):
    named, const = _tiny(head)
    dec = step_ref.decisions(named, const)
    # the tiny step must reach every stage: visible key points, occupied neighbours, covered voxels
    out, grads = step_ref.step(named, const, dec, torch.float64, chunk=100)          # several slices per stage
    want, wgrads = step_ref.step_autograd(named, const, dec, torch.float64)
    _close(out["loss"], want["loss"], 1e-12, f"{head}: loss")
    for k in ("logits", "bin_logits", "density"):
        if k in want:
            _close(out[k], want[k], 1e-12, f"{head}: {k}")
    for (name, a), (_, b) in zip(_flat(grads), _flat(wgrads)):
        assert float(b.abs().max()) > 0, f"{head}: {name} has no gradient at the tiny size"
        _close(a, b, 1e-10, f"{head}: grad {name}")
    # the same code in float32: loosely the same step (the stage-wise backward is consistent across dtypes)
    out32, grads32 = step_ref.step(named, const, dec, torch.float32, chunk=100)
    _close(out32["loss"].double(), out["loss"], 1e-4, f"{head}: loss float32")
    for (name, a), (_, b) in zip(_flat(grads32), _flat(grads)):
        _close(a.double(), b, 2e-3, f"{head}: grad {name} float32")
