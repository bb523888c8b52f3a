"""CPU checks of the training form of the fused deformable aggregation (gf_daf_fused_forward_masked / gf_daf_fused_backward,
gaussianformer_amd.deformable_prepare.deformable_fused): the float64 restatement its GPU tests compare against
(tests/daf_fused_ref.py) is pinned to outputs of the reference's own code, and the new C entry points refuse bad arguments
before any HIP call."""
import os

import numpy as np
import torch

import daf_fused_ref as ref
from gaussianformer_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "daf_ref.npz")


def test_restatement_sampling_matches_reference_golden():
    """The restatement's projection + bilinear DAF + key-point rows against tests/golden/daf_ref.npz (the reference's
    feature_sampling + multi_view_level_fusion, run unchanged by tools/make_golden_daf_ref.py), forward and gradients."""
    d = np.load(GOLDEN)
    t = lambda k, g=False: torch.tensor(d[k], dtype=torch.float64, requires_grad=g)
    levels = [tuple(int(v) for v in row) for row in d["levels"]]
    maps = [t(f"feature_map{i}", True) for i in range(len(levels))]
    kp = t("key_points", True)
    w6 = t("weights", True)                                         # [bs, A, cams, L, K, G]
    bs, A, cams, L, K, G = w6.shape
    uv, visible = ref.project(kp, t("projection_mat"), t("image_wh"))
    assert np.array_equal(visible.permute(0, 3, 1, 2).numpy(), d["visible"])
    w = w6.permute(0, 1, 4, 2, 3, 5).reshape(bs, A * K, cams, L, G)
    out = ref.daf(maps, uv.reshape(bs, A * K, cams, 2), w).reshape(bs, A, K, -1)
    want = d["output_f64"]
    assert np.abs(want).max() > 0.1
    assert np.abs(out.detach().numpy() - want).max() <= 1e-6 * np.abs(want).max()
    out.backward(t("grad_output"))
    for i in range(len(levels)):
        want = d[f"grad_feature_map{i}_f64"]
        assert np.abs(maps[i].grad.numpy() - want).max() <= 1e-6 * max(np.abs(want).max(), 1.0), i
    # the reference's fallback zero-pads locations outside (0, 1)^2 where the kernel skips them: weights where the gate is open
    gate = visible.permute(0, 1, 3, 2)[:, :, :, None, :, None].expand(w6.shape).numpy()
    want = d["grad_weights_f64"]
    assert gate.mean() > 0.2
    assert np.abs(w6.grad.numpy() - want)[gate].max() <= 1e-6 * np.abs(want).max()
    want = d["grad_key_points_f64"]
    assert np.abs(kp.grad.numpy() - want).max() <= 1e-6 * np.abs(want).max()


def test_restatement_softmax_rules():
    """all_miss per group, dropped entries weigh 0, weights of a live group sum to 1."""
    g = torch.Generator().manual_seed(0)
    b, A, pts, cams, L, G = 1, 3, 2, 2, 2, 2
    visible = torch.ones(b, A, pts, cams, dtype=torch.bool)
    visible[0, 1] = False                                           # anchor 1: nobody sees it
    raw = torch.randn(b, A, cams, L, pts, G, generator=g, dtype=torch.float64)
    keep = torch.ones_like(raw, dtype=torch.bool)
    keep[0, 2, ..., 0] = False                                      # anchor 2: group 0 dropped entirely
    keep[0, 0, 0, 0, 0, 1] = False                                  # anchor 0: one entry of group 1 dropped
    w = ref.softmax_weights(visible, raw, keep)
    assert float(w[0, 1].abs().max()) == 0.0
    assert float(w[0, 2, ..., 0].abs().max()) == 0.0
    assert torch.allclose(w[0, 2, ..., 1].sum(), torch.tensor(1.0, dtype=torch.float64))
    assert float(w[0, 0, 0, 0, 0, 1]) == 0.0
    assert torch.allclose(w[0, 0].sum(dim=(0, 1, 2)), torch.ones(G, dtype=torch.float64))


def test_new_entry_points_refuse_bad_arguments_without_gpu():
    lib = _lib.load()
    p = 4096   # an address that is never dereferenced: every call below fails a check before any HIP call
    def fwd(B=1, A=4, pts=9, cams=6, L=4, G=4, C=128, nf=100, ptrs=None):
        kp, pm, wh, raw, ra, rc, wm, feat, ss, st, out = ptrs or [p, p, None, p, None, None, None, p, p, p, p]
        return lib.gf_daf_fused_forward_masked(B, A, pts, cams, L, G, C, nf, kp, pm, wh, raw, ra, rc, wm, feat, ss, st, out, None)
    def bwd(B=1, A=4, pts=9, cams=6, L=4, G=4, C=128, nf=100, **over):
        args = dict(kp=p, pm=p, wh=None, raw=None, ra=p, rc=p, wm=None, feat=p, ss=p, st=p, go=p, gfeat=p, gkp=p, graw=None,
                    gra=p, grc=p, ws=p, wsb=1 << 30)
        args.update(over)
        a = args
        return lib.gf_daf_fused_backward(B, A, pts, cams, L, G, C, nf, a["kp"], a["pm"], a["wh"], a["raw"], a["ra"], a["rc"],
                                         a["wm"], a["feat"], a["ss"], a["st"], a["go"], a["gfeat"], a["gkp"], a["graw"], a["gra"],
                                         a["grc"], a["ws"], a["wsb"], None)
    for kw, msg in ((dict(G=3), b"power of two"), (dict(pts=65, cams=4), b"pts * cams"), (dict(L=17, G=4), b"L * G"),
                    (dict(C=100), b"channels"), (dict(A=-1), b"bad size")):
        assert fwd(**kw) == -1 and msg in lib.gf_last_error(), kw
        assert bwd(**kw) == -1 and msg in lib.gf_last_error(), kw
    assert fwd(ptrs=[None, p, None, p, None, None, None, p, p, p, p]) == -1 and b"null" in lib.gf_last_error()
    assert fwd(ptrs=[p, p, None, p, p, p, None, p, p, p, p]) == -1 and b"raw_weights" in lib.gf_last_error()
    for name in ("kp", "pm", "feat", "ss", "st", "go"):
        assert bwd(**{name: None}) == -1 and b"null" in lib.gf_last_error(), name
    assert bwd(ra=None) == -1 and b"raw_anchor" in lib.gf_last_error()
    assert bwd(raw=p, ra=None, rc=None) == -1 and b"raw_anchor" in lib.gf_last_error()      # grad_raw_anchor with full logits
    assert bwd(graw=p) == -1 and b"grad_raw_weights" in lib.gf_last_error()                  # grad_raw_weights with split logits
    need = lib.gf_daf_fused_backward_workspace_bytes(1, 4, 9, 6, 4, 4)
    assert need >= 4 * 6 * 4 * 9 * 4
    assert bwd(wsb=need - 1) == -1 and b"workspace" in lib.gf_last_error()
    assert bwd(ws=None) == -1 and b"workspace" in lib.gf_last_error()
    assert lib.gf_daf_fused_backward_workspace_bytes(-1, 4, 9, 6, 4, 4) == 0
    # empty problems are fine and touch nothing
    assert fwd(A=0) == 0 and bwd(A=0) == 0
