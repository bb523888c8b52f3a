"""The drop-in ``GaussianOccEncoder`` on the GPU: two encoders of two decoder blocks each (so the refine -> anchor encoder -> next
block hand-over runs), built from the recorded settings of a prob/ config (multi-layer sparse block, ``residual_mode="none"``,
every ``"identity", X, "add", "norm"`` folded) and of the solid config (``"cat"``, single-layer sparse block with ``output_proj``).

Routing is held at ZERO tolerance: the library repeats bit for bit, so with ``fold = True`` the predictions equal a sequence
written out here from the public functions, and with ``fold = False`` the reference's loop written out op by op on the same
modules; any difference is a routing error.  Each fused call is held to float64 truth by its own op's tests, so no end-to-end
tolerance is invented here."""
import functools
import json

import pytest
import torch
import torch.nn as nn

from gaussianformer_amd import GaussianOccEncoder
from gaussianformer_amd.ffn import ffn_block
from row_judge import spy  # noqa: F401  (a fixture)
from test_deform_block_gpu import _cameras
from test_encoder import FIRST, GOLDEN, LATER, PROB_BLOCK

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
A, CAMS = 301, 6
LEVELS = [(8, 16), (4, 8), (2, 4), (1, 2)]
STYLES = {"prob": ("prob/nuscenes_gs6400", PROB_BLOCK * 2), "solid": ("nuscenes_gs25600_solid", FIRST + LATER)}

DEFORM = ["gf_deform_logits_forward", "gf_key_points", "gf_daf_fused_forward", "gf_deform_output_forward"]
SPCONV_BUILD = ["gf_subm_voxelize", "gf_subm_rulebook_build"]
PROB_BLOCK_LAUNCHES = (DEFORM + ["gf_ffn_forward"] + SPCONV_BUILD + ["gf_subm_conv_apply_epilogue"] * 3 + ["gf_deform_output_forward"]
                       + ["gf_ffn_forward", "gf_refine_forward"])
LAUNCHES = {
    "prob": ["gf_feature_maps_format", "gf_anchor_embed_forward"] + PROB_BLOCK_LAUNCHES + ["gf_anchor_embed_forward"] + PROB_BLOCK_LAUNCHES,
    "solid": (["gf_feature_maps_format", "gf_anchor_embed_forward"] + DEFORM + ["gf_ffn_forward", "gf_refine_forward"]
              + ["gf_anchor_embed_forward"] + SPCONV_BUILD + ["gf_subm_conv_apply_scratch", "gf_deform_output_forward"] + DEFORM
              + ["gf_ffn_forward", "gf_refine_forward"]),
}


@functools.lru_cache(maxsize=None)
def encoder(style):
    family, order = STYLES[style]
    with open(GOLDEN) as f:
        s = json.load(f)[family]
    cfg = {k: v for k, v in s.items() if k != "operation_order"}
    cfg["spconv_layer"] = dict(cfg["spconv_layer"], pairs_per_point=64)       # nothing is read back: capturable
    torch.manual_seed(3)
    enc = GaussianOccEncoder(operation_order=order, **cfg)
    enc.init_weights()
    with torch.no_grad():      # (init_weights zeroes weights_fc and leaves every LayerNorm at identity: make them count)
        for m in enc.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_(1 + 0.3 * torch.randn(m.weight.shape))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape))
        for m, op in zip(enc.layers, order):
            if op == "deformable":
                m.weights_fc.weight.copy_(0.05 * torch.randn(m.weights_fc.weight.shape))
    return enc.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def scene():
    g = torch.Generator().manual_seed(100)
    maps = [torch.randn(1, CAMS, 128, h, w, generator=g).to(DEV) for h, w in LEVELS]
    anchor = torch.randn(1, A, 28, generator=g)
    anchor[..., :3] *= 1.5
    feats = torch.randn(1, A, 128, generator=g)
    pm, wh = _cameras(CAMS)
    return dict(maps=maps, anchor=anchor.to(DEV), feats=feats.to(DEV), metas=dict(projection_mat=pm, image_wh=wh))


def run(enc, s, feats=None):
    """``(predictions as a flat list of tensors, the anchor the last refinement returned)``."""
    got = {}
    last = [m for m, op in zip(enc.layers, enc.operation_order) if "refine" in op][-1]
    handle = last.register_forward_hook(lambda mod, a, out: got.__setitem__("anchor", out[0]))
    try:
        out = enc(s["anchor"], s["feats"] if feats is None else feats, s["maps"], s["metas"])
    finally:
        handle.remove()
    preds = out["representation"]
    assert list(out) == ["representation"] and all(list(p) == ["gaussian"] for p in preds)
    return [t for p in preds for t in p["gaussian"] if t is not None], got["anchor"]


def same(a, b):
    (pa, aa), (pb, ab) = a, b
    assert len(pa) == len(pb) and len(pa) >= 10
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), i
    assert torch.equal(aa.view(torch.int32), ab.view(torch.int32))


def folded_by_hand(enc, s, feats=None):
    """The folded frame from the public functions: ``ffn_block``, the deformable module and ``SparseConv3D`` with ``residual=`` /
    ``norm=``, the refinement module, the anchor encoder."""
    from gaussianformer_amd.deformable_aggregation import DeformableAggregationFunction as DAF
    L, order = enc.layers, enc.operation_order
    anchor, x, metas = s["anchor"], s["feats"] if feats is None else feats, s["metas"]
    fm = DAF.feature_maps_format(s["maps"])
    emb = enc.anchor_encoder(anchor)
    preds = []
    if "identity" in order:                              # prob: every X takes its "add" and "norm"
        for o in range(0, len(order), 17):
            x = L[o + 1](x, anchor, emb, fm, metas, residual=x, norm=L[o + 3])
            x = ffn_block(x, L[o + 5], L[o + 7], residual=x)
            x = L[o + 9](x, anchor, residual=x, norm=L[o + 11])
            x = ffn_block(x, L[o + 13], L[o + 15], residual=x)
            anchor, g = L[o + 16](x, anchor, emb)
            preds.append(g)
            if o + 17 < len(order):
                emb = enc.anchor_encoder(anchor)
    else:                                                # solid: "cat" takes nothing; "ffn", "norm" and "spconv", "norm" fold
        x = L[0](x, anchor, emb, fm, metas)
        x = ffn_block(x, L[1], L[2])
        anchor, g = L[3](x, anchor, emb)
        preds.append(g)
        emb = enc.anchor_encoder(anchor)
        x = L[4](x, anchor, norm=L[5])
        x = L[6](x, anchor, emb, fm, metas)
        x = ffn_block(x, L[7], L[8])
        anchor, g = L[9](x, anchor, emb)
        preds.append(g)
    return [t for g in preds for t in g if t is not None], anchor


def loop_by_hand(enc, s, feats=None):
    """The reference's loop (gaussian_encoder.py:88-121), op by op on the same module objects."""
    anchor, instance_feature, metas = s["anchor"], s["feats"] if feats is None else feats, s["metas"]
    feature_maps = s["maps"]
    anchor_embed = enc.anchor_encoder(anchor)
    preds, identity = [], None
    for i, op in enumerate(enc.operation_order):
        if op == "spconv":
            instance_feature = enc.layers[i](instance_feature, anchor)
        elif op == "norm" or op == "ffn":
            instance_feature = enc.layers[i](instance_feature)
        elif op == "identity":
            identity = instance_feature
        elif op == "add":
            instance_feature = instance_feature + identity
        elif op == "deformable":
            instance_feature = enc.layers[i](instance_feature, anchor, anchor_embed, feature_maps, metas)
        else:
            anchor, gaussian = enc.layers[i](instance_feature, anchor, anchor_embed)
            preds.append(gaussian)
            if i != len(enc.operation_order) - 1:
                anchor_embed = enc.anchor_encoder(anchor)
    return [t for g in preds for t in g if t is not None], anchor


@pytest.mark.parametrize("style", list(STYLES))
def test_folded_routing_and_launches(style, spy):
    enc, s = encoder(style), scene()
    norms = [m for m, op in zip(enc.layers, enc.operation_order) if op == "norm"]
    ran = []
    handles = [m.register_forward_hook(lambda *a: ran.append(1)) for m in norms]
    with torch.no_grad():
        del spy[:]
        got = run(enc, s)
        assert spy == LAUNCHES[style]
        assert spy.count("gf_feature_maps_format") == 1 and not ran          # formatted once; no "norm" ran as a torch layer
        for h in handles:
            h.remove()
        same(got, folded_by_hand(enc, s))
        assert all(bool(torch.isfinite(t).all()) for t in got[0])
        # the frame depends on every op: another input, other predictions
        other = run(enc, s, s["feats"].flip(1).contiguous())
        assert not torch.equal(other[0][0], got[0][0])


@pytest.mark.parametrize("style", list(STYLES))
def test_unfolded_is_the_references_loop(style, spy):
    enc, s = encoder(style), scene()
    norms = [m for m, op in zip(enc.layers, enc.operation_order) if op == "norm"]
    ran = []
    handles = [m.register_forward_hook(lambda *a: ran.append(1)) for m in norms]
    enc.fold = False
    try:
        with torch.no_grad():
            del spy[:]
            got = run(enc, s)
            # every "norm" ran as the layer it is (each module still takes its own route inside: the sparse block's stages)
            assert spy.count("gf_feature_maps_format") == 1 and len(ran) == len(norms)
            same(got, loop_by_hand(enc, s))
    finally:
        del enc.fold
        for h in handles:
            h.remove()
    assert enc.fold is True


@pytest.mark.parametrize("style", list(STYLES))
def test_training_walks_the_order_op_by_op(style, spy):
    enc, s = encoder(style), scene()
    enc.train()
    try:
        feats = s["feats"].clone().requires_grad_()
        torch.manual_seed(9)
        del spy[:]
        got = run(enc, s, feats)
        assert "gf_ffn_forward" not in spy and "gf_subm_conv_apply_epilogue" not in spy and "gf_deform_output_forward" not in spy
        torch.manual_seed(9)                      # (the same dropout masks: the loop makes the same module calls in the same order)
        want = loop_by_hand(enc, s, s["feats"].clone().requires_grad_())
        same(([t.detach() for t in got[0]], got[1].detach()), ([t.detach() for t in want[0]], want[1].detach()))
        sum(t.square().mean() for t in got[0]).backward()
        assert feats.grad is not None and bool(torch.isfinite(feats.grad).all()) and float(feats.grad.abs().max()) > 0
    finally:
        enc.eval()
        enc.zero_grad(set_to_none=True)


@pytest.mark.parametrize("style", list(STYLES))
def test_folded_frame_as_one_graph(style):
    enc, s = encoder(style), scene()
    feats = s["feats"].clone()
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run(enc, s, feats)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            preds, anchor = run(enc, s, feats)
        for flip in (False, True):
            if flip:
                feats.copy_(s["feats"].flip(1))
            graph.replay()
            got = ([t.clone() for t in preds], anchor.clone())
            same(got, run(enc, s, feats))
