"""DCNv2 on the MI355X (csrc/deform_conv.hip) against the float64 restatement of tests/dcn_ref.py: the full backbone shapes,
odd shapes, adversarial offsets, reproducibility, checkpointing, graph capture and a training step."""
import pytest
import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

import dcn_ref
from gaussianformer_amd.deform_conv import DCNv2, modulated_deform_conv2d

pytestmark = pytest.mark.gpu

FWD_REL = 2.0 ** -20   # |out - ref| <= FWD_REL (sum |w| |col| + |bias|) + FWD_ABS
FWD_ABS = 1e-7
GRAD_RTOL = 1e-4       # per row: max |got - ref| <= GRAD_RTOL max(max |ref row|, 1e-3 max |ref|)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def make_case(dev, N, C, H, W, Co, kh, kw, stride=1, padding=0, dilation=1, dg=1, bias=True, offsets="real", seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    x = torch.randn(N, C, H, W, generator=g)
    w = (torch.rand(Co, C, kh, kw, generator=g) * 2 - 1) / (C * kh * kw) ** 0.5
    b = torch.randn(Co, generator=g) if bias else None
    oshape = (N, 2 * dg * kh * kw, Ho, Wo)
    if offsets == "zero":
        off = torch.zeros(oshape)
    elif offsets == "real":
        off = torch.randn(oshape, generator=g) * 1.5
    elif offsets == "integer":
        off = torch.randint(-3, 4, oshape, generator=g).float()
    elif offsets == "edges":
        # a mix: exact integers, samples exactly at -1 and at H / W (outside), far outside, and fractional ones
        kind = torch.randint(0, 5, oshape, generator=g)
        o = off_fr = torch.randn(oshape, generator=g) * 2
        base_y = torch.zeros(oshape)
        i = torch.arange(kh).repeat_interleave(kw)
        j = torch.arange(kw).repeat(kh)
        by = (torch.arange(Ho)[None, :] * sh - ph + i[:, None] * dh).float()     # [kk, Ho]
        bx = (torch.arange(Wo)[None, :] * sw - pw + j[:, None] * dw).float()     # [kk, Wo]
        v = base_y.view(N, dg, kh * kw, 2, Ho, Wo)
        v[:, :, :, 0] = by[None, None, :, :, None]
        v[:, :, :, 1] = bx[None, None, :, None, :]
        lim = torch.zeros(oshape).view(N, dg, kh * kw, 2, Ho, Wo)
        lim[:, :, :, 0], lim[:, :, :, 1] = float(H), float(W)
        lim = lim.view(oshape)
        o = torch.where(kind == 0, torch.round(off_fr), o)
        o = torch.where(kind == 1, -1.0 - base_y, o)          # sample exactly at -1
        o = torch.where(kind == 2, lim - base_y, o)           # sample exactly at H (rows) / W (columns)
        o = torch.where(kind == 3, torch.full(oshape, 1e3), o)   # far outside
        off = o
    elif offsets == "outside":
        off = torch.full(oshape, -1e4)
    else:
        raise ValueError(offsets)
    m = torch.rand(N, dg * kh * kw, Ho, Wo, generator=g)
    t = lambda a: None if a is None else a.to(dev).contiguous()
    return dict(x=t(x), off=t(off), m=t(m), w=t(w), b=t(b), stride=stride, padding=padding, dilation=dilation, dg=dg)


def native(c, gout=None, grads=True):
    leaves = [c[k].clone().requires_grad_(grads) if c[k] is not None else None for k in ("x", "off", "m", "w", "b")]
    out = modulated_deform_conv2d(*leaves, c["stride"], c["padding"], c["dilation"], 1, c["dg"])
    res = {"out": out.detach()}
    if gout is not None:
        out.backward(gout)
        for k, t in zip(("x", "off", "m", "w", "b"), leaves):
            res["g" + k] = None if t is None else t.grad
    return res


def reference(c, gout):
    leaves = [c[k].double().requires_grad_(True) if c[k] is not None else None for k in ("x", "off", "m", "w", "b")]
    x, off, m, w, b = leaves
    out = dcn_ref.modulated_deform_conv2d(x, off, m, w, b, c["stride"], c["padding"], c["dilation"], 1, c["dg"])
    out.backward(gout.double())
    res = {"out": out.detach(), "bound": dcn_ref.abs_bound(c["x"], c["off"], c["m"], c["w"], c["stride"], c["padding"],
                                                           c["dilation"], c["dg"])}
    for k, t in zip(("x", "off", "m", "w", "b"), leaves):
        res["g" + k] = None if t is None else t.grad
    return res


def assert_rows(got, ref, rows, what):
    assert got.shape == ref.shape, what
    assert torch.isfinite(got).all(), f"{what}: non-finite"
    g = got.double().reshape(rows, -1)
    r = ref.reshape(rows, -1)
    scale = torch.clamp(r.abs().amax(1), min=1e-3 * float(r.abs().max()) + 1e-30)
    err = (g - r).abs().amax(1) / scale
    worst = int(err.argmax())
    assert float(err.max()) <= GRAD_RTOL, f"{what}: row {worst} err {float(err.max()):.3e} > {GRAD_RTOL}"


def check_case(c, seed=7):
    dev = c["x"].device
    N, Co = c["x"].shape[0], c["w"].shape[0]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    sh, sw = _pair(c["stride"])
    out0 = native(c, grads=False)["out"]
    gout = torch.randn(out0.shape, generator=gen).to(dev)
    got = native(c, gout)
    ref = reference(c, gout)
    err = (got["out"].double() - ref["out"]).abs()
    bound = ref["bound"] if c["b"] is None else ref["bound"] + c["b"].double().abs()[None, :, None, None]   # bias: one more term
    lim = FWD_REL * bound + FWD_ABS
    assert bool((err <= lim).all()), f"forward: worst err / bound {float((err / lim).max()):.3f}"
    C = c["x"].shape[1]
    assert_rows(got["gx"], ref["gx"], N * C, "grad_input")
    assert_rows(got["goff"], ref["goff"], c["off"].shape[0] * c["off"].shape[1], "grad_offset")
    assert_rows(got["gm"], ref["gm"], c["m"].shape[0] * c["m"].shape[1], "grad_mask")
    assert_rows(got["gw"], ref["gw"], Co, "grad_weight")
    if c["b"] is not None:
        assert_rows(got["gb"], ref["gb"], 1, "grad_bias")
    return got


@pytest.mark.parametrize("name,N,C,H,W,Co", [("layer3", 6, 256, 54, 100, 256), ("layer4", 6, 512, 27, 50, 512)])
@pytest.mark.parametrize("offsets", ["zero", "real"])
def test_backbone_shapes(gpu, name, N, C, H, W, Co, offsets):
    c = make_case(gpu, N, C, H, W, Co, 3, 3, 1, 1, 1, 1, bias=False, offsets=offsets, seed=C + H)
    check_case(c)
    torch.cuda.empty_cache()


ODD = [
    # N, C, H, W, Co, kh, kw, stride, padding, dilation, dg, bias
    (2, 32, 7, 9, 32, 3, 3, 1, 1, 1, 1, True),
    (1, 64, 13, 11, 96, 1, 1, 1, 0, 1, 2, False),
    (3, 64, 10, 12, 64, 3, 5, (2, 1), (1, 2), 1, 2, True),
    (2, 128, 9, 17, 32, 3, 3, 2, 2, 2, 4, True),
    (1, 32, 5, 6, 64, 3, 3, 1, 0, (2, 1), 1, False),
    (2, 96, 21, 19, 160, 3, 3, 1, 1, 1, 1, True),
    (1, 64, 8, 8, 32, 7, 7, 1, 3, 1, 1, True),
]


@pytest.mark.parametrize("case", ODD)
@pytest.mark.parametrize("offsets", ["real", "integer", "edges"])
def test_odd_shapes(gpu, case, offsets):
    N, C, H, W, Co, kh, kw, s, p, d, dg, bias = case
    check_case(make_case(gpu, N, C, H, W, Co, kh, kw, s, p, d, dg, bias, offsets=offsets, seed=N * 31 + C + H))


def test_samples_outside_give_bias_only(gpu):
    c = make_case(gpu, 2, 64, 9, 10, 64, 3, 3, 1, 1, 1, 2, True, offsets="outside")
    got = check_case(c)
    assert torch.equal(got["out"], c["b"][None, :, None, None].expand_as(got["out"]))
    assert not got["gx"].any() and not got["goff"].any() and not got["gm"].any() and not got["gw"].any()


def test_empty_batch(gpu):
    c = make_case(gpu, 0, 64, 9, 10, 32, 3, 3, 1, 1, 1, 1, True)
    got = native(c, torch.zeros(0, 32, 9, 10, device=gpu))
    assert got["out"].shape == (0, 32, 9, 10)
    assert got["gw"].shape == c["w"].shape and not got["gw"].any() and not got["gb"].any()


def test_reproducible(gpu):
    c = make_case(gpu, 2, 128, 27, 30, 128, 3, 3, 1, 1, 1, 2, True, offsets="real", seed=5)
    gout = torch.randn(2, 128, 27, 30, device=gpu)
    a, b = native(c, gout), native(c, gout)
    for k in ("out", "goff", "gm", "gw", "gb"):
        assert torch.equal(a[k], b[k]), k
    assert torch.allclose(a["gx"], b["gx"], rtol=1e-5, atol=1e-6)


def _pack(dev, C=64, Co=64, seed=3):
    torch.manual_seed(seed)
    mod = DCNv2(C, Co, 3, padding=1, bias=True).to(dev)
    with torch.no_grad():
        mod.conv_offset.weight.normal_(0, 0.05)
        mod.conv_offset.bias.normal_(0, 0.5)
        mod.bias.normal_()
    return mod


def test_pack_inside_checkpoint(gpu):
    mod = _pack(gpu)
    x = torch.randn(2, 64, 15, 17, device=gpu)
    grads = []
    for use_cp in (False, True):
        mod.zero_grad()
        xi = x.clone().requires_grad_(True)
        y = checkpoint(mod, xi, use_reentrant=False) if use_cp else mod(xi)
        (y * y).sum().backward()
        grads.append([xi.grad] + [p.grad.clone() for p in mod.parameters()])
    for a, b in zip(*grads):   # grad_input (atomics) and MIOpen's conv_offset backward need not repeat bit for bit
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    assert torch.equal(grads[0][1], grads[1][1])   # the weight gradient is bitwise reproducible


def test_graph_capture_replays_eager_bits(gpu):
    c = make_case(gpu, 2, 64, 20, 24, 64, 3, 3, 1, 1, 1, 1, True, offsets="real", seed=9)
    args = (c["x"], c["off"], c["m"], c["w"], c["b"], 1, 1, 1, 1, 1)
    with torch.no_grad():
        eager = modulated_deform_conv2d(*args)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                modulated_deform_conv2d(*args)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = modulated_deform_conv2d(*args)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)


class _Frozen(nn.BatchNorm2d):
    def train(self, mode=True):
        return super().train(False)


def test_bottleneck_trains_one_step(gpu):
    torch.manual_seed(11)
    net = nn.Sequential(nn.Conv2d(64, 32, 1, bias=False), _Frozen(32), nn.ReLU(), DCNv2(32, 32, 3, padding=1, bias=False),
                        nn.BatchNorm2d(32), nn.ReLU(), nn.Conv2d(32, 64, 1, bias=False)).to(gpu)
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    x = torch.randn(2, 64, 16, 20, device=gpu)
    loss = (net(x) - x).square().mean()
    loss.backward()
    dcn = net[3]
    for p in (dcn.conv_offset.weight, dcn.conv_offset.bias, dcn.weight):
        assert torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
    before = dcn.conv_offset.weight.detach().clone()
    opt.step()
    assert not torch.equal(before, dcn.conv_offset.weight)
    assert torch.isfinite((net(x) - x).square().mean())


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_launches_go_to_the_tensors_device_not_the_current_one(gpu):
    """DCNv2 and the occupancy loss, forward and backward, on tensors of device 1 while device 0 is current, against the same
    calls with device 1 current: the same bits, except ``grad_input`` (fp32 atomics), which is held to this file's row bound."""
    from gaussianformer_amd.occupancy_loss import occupancy_loss
    other = torch.device("cuda:1")
    gen = torch.Generator(device="cpu").manual_seed(11)
    c = make_case(other, 2, 32, 9, 11, 32, 3, 3, padding=1, seed=5)
    gout = torch.randn(2, 32, 9, 11, generator=gen).to(other)
    n = 4096
    pred = [torch.randn(1, n, 18, generator=gen).to(other) for _ in range(2)]
    label = torch.randint(0, 18, (1, n), generator=gen).to(other)
    mask = (torch.rand(1, n, generator=gen) < 0.8).to(other)
    weights = (torch.rand(18, generator=gen) + 0.5).to(other)

    def run():
        res = native(c, gout)
        leaves = [p.clone().requires_grad_(True) for p in pred]
        loss = occupancy_loss([t.transpose(1, 2) for t in leaves], label, mask, class_weights=weights, lovasz_ignore=17)
        loss.backward()
        torch.cuda.synchronize(other)
        return res, [loss.detach()] + [t.grad for t in leaves]

    with torch.cuda.device(1):
        want_dcn, want_loss = run()
    with torch.cuda.device(0):
        got_dcn, got_loss = run()
    for k in ("out", "goff", "gm", "gw", "gb"):
        assert torch.equal(got_dcn[k], want_dcn[k]), k
    assert_rows(got_dcn["gx"], want_dcn["gx"].double(), 2 * 32, "grad_input")
    for g, w in zip(got_loss, want_loss):
        assert g.device == other and torch.equal(g, w)
