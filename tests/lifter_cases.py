"""Shared by test_lifter_cases.py (CPU: the conditions each case must meet under the restatement alone) and
test_lifter_shapes_gpu.py (the kernels against the restatement): the lifter's inputs at every entries-per-lane instantiation
``R = ceil(bins / 64)`` of csrc/lifter.hip, at both sides of every 64-entry chunk edge, and the pixel loss's ragged rows, upstream
gradients, clamp and floor.  Everything is numpy and seeded; lifter_ref.py is the truth for all of it."""
import functools

import numpy as np

import lifter_ref as ref

# ---- 1. lifting ---------------------------------------------------------------------------------------------------------------
B, N, H, W = 2, 3, 4, 6                     # 72 pixels per element: one full workgroup of 64 and a tail wave of 8.  h and w even:
#                                             an odd size puts a pixel centre on the optical axis, so z = 1.5 and y = 0 lie on faces
PC = [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0]
VS = 0.5
RES = (200, 200, 16)
EMPTY = 17
GRID = dict(pc_range=PC, voxel_size=VS, occ_resolution=RES)
# not symmetric, another voxel size, another resolution (80.4 / 0.4, 80 / 0.4, 8 / 0.4)
OTHER_GRID = dict(pc_range=[-40.0, -32.0, -3.0, 40.4, 48.0, 5.0], voxel_size=0.4, occ_resolution=(201, 200, 20))
# wide enough to hold the last bin's points (71.7 m out, up to 18 m above or below the camera), which the largest uniform picks
FAR_GRID = dict(pc_range=[-80.0, -80.0, -32.0, 80.0, 80.0, 32.0], voxel_size=2.0, occ_resolution=(80, 80, 32))
IMAGE_WH = [(1600.0, 864.0), (1408.0, 768.0), (1920.0, 1056.0)]
YAW1, HEIGHT1 = 17.0, 1.9                   # element 1: the ring turned by 17 degrees, cameras 0.4 m higher
MAX_EXEMPT_SHARE = 0.01

LIFT_S = (1, 62, 63, 64, 127, 191, 192, 255)        # bins 2, 63 | 64 | 65, 128, 192 | 193, 256
LIFT_CASES = [(S, a, st) for S in LIFT_S for a in ((1, 2) if S == 1 else (1, 3, 8)) for st in (False, True)]
NO_GT_CASES = [(64, 3, True), (255, 3, False)]      # R = 2 and R = 4 without an occupancy table
OTHER_GRID_CASE = (127, 3, True)
EDGE_UNIFORM_CASE = (127, 3)
ONE_BELOW_1 = np.nextafter(np.float32(1), np.float32(0))


def ring(whs, yaw0=0.0, height=1.5):
    """lidar2img of ``len(whs)`` cameras on a ring (test_lifter_gpu.lidar2img's, with a starting yaw, a camera height and an
    image size per camera).  [n, 4, 4] fp32."""
    mats = []
    for (W_img, H_img), yaw in zip(whs, np.deg2rad(yaw0 + np.linspace(0.0, 360.0, len(whs), endpoint=False))):
        f = 0.79 * W_img
        K = np.array([[f, 0, W_img / 2, 0], [0, f, H_img / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        c2l = np.eye(4)
        c2l[:3, 0] = [np.sin(yaw), -np.cos(yaw), 0.0]
        c2l[:3, 1] = [0.0, 0.0, -1.0]
        c2l[:3, 2] = [np.cos(yaw), np.sin(yaw), 0.0]
        c2l[:3, 3] = [0.0, 0.0, height]
        mats.append(K @ np.linalg.inv(c2l))
    return np.stack(mats).astype(np.float32)


def cameras():
    """``(projection_mat [B, N, 4, 4], image_wh [B, N, 2])``: no two cameras of the two elements share a matrix or a size."""
    wh = [IMAGE_WH, IMAGE_WH[1:] + IMAGE_WH[:1]]
    proj = np.stack([ring(wh[0]), ring(wh[1], YAW1, HEIGHT1)])
    return proj, np.asarray(wh, np.float32)


@functools.lru_cache(maxsize=None)
def occupancy(res=RES):
    """``(occ_label [B, X, Y, Z] int64, occ_cam_mask bool)``: about 30 % of the voxels hold a class 0..16 (the rest EMPTY), the
    camera mask keeps about 80 %.  Built once per resolution; callers do not write to it."""
    rng = np.random.default_rng(20)
    shape = (B,) + tuple(res)
    label = np.where(rng.random(shape) < 0.3, rng.integers(0, 17, shape), EMPTY).astype(np.int64)
    mask = rng.random(shape) < 0.8
    return label, mask


def packed(label, mask):
    return ((label != EMPTY) & mask).astype(np.uint8)


def depth_bins(S):
    """Off the voxel lattice (with 1.0 .. 72.0 the only bin of S = 1 sits on a face)."""
    return np.linspace(1.3, 71.7, S).astype(np.float32)


def lift_inputs(S, a, stochastic, grid=None, seed=None):
    """Everything ``lift_pixels`` and ``lifter_ref.lift`` take, as numpy arrays."""
    grid = GRID if grid is None else grid
    rng = np.random.default_rng(1000 * S + 10 * a + stochastic if seed is None else seed)
    logits = (2.0 * rng.standard_normal((B, N, H, W, S + 1))).astype(np.float32)
    logits[..., S] += np.float32(1.5)
    proj, wh = cameras()
    label, mask = occupancy(tuple(grid["occ_resolution"]))
    u = rng.random((B, N, H, W, a), dtype=np.float32) if stochastic else None
    return dict(logits=logits, proj=proj, wh=wh, depth=depth_bins(S), u=u, occ_label=label, occ_cam_mask=mask, a=a, grid=grid)


def edge_uniform_inputs():
    """A stochastic case whose uniforms hold exactly 0.0 (eight slots) and the largest float below 1 (eight slots)."""
    S, a = EDGE_UNIFORM_CASE
    inp = lift_inputs(S, a, True, grid=FAR_GRID, seed=77)
    flat = inp["u"].reshape(-1)
    flat[3:3 + 8 * 23:23] = 0.0
    flat[11:11 + 8 * 23:23] = ONE_BELOW_1
    return inp


def sure_top_uniform_slots(inp, r):
    """``(element, slot)`` of the uniforms ``ONE_BELOW_1`` whose answer does not depend on rounding although ``lift`` marks them
    (they are within its cdf tolerance of the last step's end): where ``cdf[S - 1] = 1 - p_S`` is at least 1e-4 below the
    uniform the count is S or S + 1, both clipped to S, so the candidate is bin S - 1's point; slots whose point lies near a
    range face are left out."""
    g = inp["grid"]["pc_range"]
    u = inp["u"].reshape(B, -1)
    p_last = np.repeat(ref.softmax64(inp["logits"])[..., -1].reshape(B, -1), inp["a"], axis=-1)
    out = []
    for i in range(B):
        for s in np.nonzero((u[i] == ONE_BELOW_1) & (p_last[i] > 1e-4))[0]:
            if not ref._near_face(r["cand"][i][s][None], np.asarray(g[:3]), None, np.asarray(g[3:]), 2e-4)[0]:
                out.append((i, int(s)))
    return out


def oracle(inp, img2lidar=None, with_gt=True, **tol):
    """``lifter_ref.lift`` of ``lift_inputs``' dict; ``img2lidar`` is the inverse the op used (numpy's where not given)."""
    if img2lidar is None:
        img2lidar = np.linalg.inv(inp["proj"].astype(np.float64)).astype(np.float32)
    g = inp["grid"]
    return ref.lift(inp["logits"], img2lidar, inp["wh"], inp["depth"], g["pc_range"], g["voxel_size"], g["occ_resolution"],
                    inp["a"], uniforms=inp["u"], occ=packed(inp["occ_label"], inp["occ_cam_mask"]) if with_gt else None, **tol)


def exempt_share(r):
    """``(marked, compared)`` of a ``lift`` result: the entries it marks as rounding-dependent, of those ``check_lift`` compares."""
    marked, compared = int(r["slot_exempt"].sum()), r["slot_exempt"].size
    if r["pixel_gt"] is not None:
        marked += int(r["gt_exempt"].sum())
        compared += r["pixel_gt"].size
    return marked, compared


# ---- 2. ties across chunks ----------------------------------------------------------------------------------------------------
TIE_S, TIE_A = 191, 4                       # 192 bins: three full chunks, entry S is lane 63's third
TIE_PC = [-1000.0, -1000.0, -1000.0, 1000.0, 1000.0, 1000.0]
TIE_RES = (4, 4, 4)


def tie_inputs():
    """``(inputs, expected [24, 4] entries or None per pixel)``: one camera, 4 x 6 pixels, identity projection and
    ``image_wh = (w, h)``, so bin k's point is ``((j + 0.5) d_k, (i + 0.5) d_k, d_k)`` and z names the bin.  Logits are
    multiples of 0.5 in [-3, 4] (or one +120): equal logits give equal pdf entries in fp32 and in float64, different ones are
    apart by a factor of 1.6 or underflow to exactly 0 together.  The first rows are hand-made, the rest random half-integers
    (ties everywhere).  ``expected[q]`` is None for a disabled pixel, otherwise the top-4 entries, lower index first."""
    S, nb = TIE_S, TIE_S + 1
    x = np.zeros((H * W, nb), np.float32)
    expected = {}
    x[0, [5, 69, 133, 70, 10]] = 3.0                         # five exact maxima: one lane in three chunks, two other lanes
    expected[0] = [5, 10, 69, 70]
    x[1, 133], x[1, [69, 5, 70]] = 4.0, 3.0                  # the maximum in the last chunk, then a lane's two entries, then a neighbour
    expected[1] = [133, 5, 69, 70]
    x[2, 100] = 120.0                                        # every other probability is exactly 0: index order alone
    expected[2] = [100, 0, 1, 2]
    x[3, 1] = 120.0
    expected[3] = [1, 0, 2, 3]
    x[4, 0] = 120.0
    expected[4] = [0, 1, 2, 3]
    x[5, S] = 120.0                                          # the "no surface" bin wins: disabled
    expected[5] = None
    x[6, [63, 127, 191, 0]] = 2.5                            # lane 63's three entries (the last is bin S) and lane 0
    expected[6] = [0, 63, 127, 191]
    x[7, [64, 128]], x[7, [0, 191]] = 1.5, 1.0               # lane 0 in chunks 1, 2 before its own chunk-0 entry; S ties with 0
    expected[7] = [64, 128, 0, 191]
    x[8, :] = -1.0                                           # everything equal
    expected[8] = [0, 1, 2, 3]
    x[9, [191, 190]] = 2.0                                   # S ties with S - 1 for the argmax: the lower index, not disabled
    expected[9] = [190, 191, 0, 1]
    rng = np.random.default_rng(5)
    first_random = 10
    x[first_random:] = 0.5 * rng.integers(-6, 7, (H * W - first_random, nb))
    for q in range(first_random, H * W):
        order = np.argsort(-x[q].astype(np.float64), kind="stable")
        expected[q] = None if order[0] == S else order[:TIE_A].tolist()
    inp = dict(logits=x.reshape(1, 1, H, W, nb), proj=np.eye(4, dtype=np.float32)[None, None],
               wh=np.array([[[float(W), float(H)]]], np.float32), depth=depth_bins(S), u=None, a=TIE_A,
               grid=dict(pc_range=TIE_PC, voxel_size=0.5, occ_resolution=TIE_RES))
    return inp, [expected[q] for q in range(H * W)]


def tie_oracle(inp, img2lidar=None):
    """``lift`` with nothing exempted for closeness (a negative ``tie_tol``)."""
    g = inp["grid"]
    return ref.lift(inp["logits"], inp["proj"] if img2lidar is None else img2lidar, inp["wh"], inp["depth"], g["pc_range"],
                    g["voxel_size"], g["occ_resolution"], inp["a"], tie_tol=-1.0)


def bins_of(scan_z, depth):
    """The depth bin each z coordinate names (identity projection: z is the bin's depth)."""
    return np.abs(np.asarray(scan_z, np.float64)[:, None] - np.asarray(depth, np.float64)[None]).argmin(-1)


# ---- 3. pixel loss ------------------------------------------------------------------------------------------------------------
LOSS_BINS = (1, 2, 3, 63, 64, 65, 128, 192, 193, 255, 256)
LOSS_ROWS = (1, 17, 70, 130)                # below a wave's 16 rows, a partial workgroup, just over two workgroups
UPSTREAM = 3.5
MODULE_WEIGHT = 0.25
LOSS_RTOL = 1e-5                            # the project's number, for the loss and per element x y for the gradient
PROBE_ULP = 4
PROBE_RTOL = 1e-6                           # what the 4-ulp probe of p may move: a tenth of the tolerance
# Logits are uniform in [-hw, hw], as narrow as the 4-ulp probe needs (test_lifter_cases.py prints what it measures):
# * sigmoid, hw = 1, narrower than the +-2.2 first tried: with t = 1 the gradient is (p - 1) / numel, 4 ulp of a p in [0.5, 1)
#   are 2.4e-7, and at p = 0.9 that is 2.4e-6 of 1 - p (measured 2.39e-6), over the probe's 1e-6.  At +-1, p <= 0.731: 8.9e-7.
# * softmax, hw = 1 from 63 bins on (measured 4.6e-7 of y).  At 2 and 3 bins +-1 gives p up to 0.88 and the probe moved an
#   element by 2.05e-6 and 1.08e-6 of y (the same 1 / (1 - p)), so these two get hw = 0.4: p <= 0.69 at 2 bins.
def logit_half_width(bins, use_sigmoid):
    return 0.4 if not use_sigmoid and bins <= 3 else 1.0


def loss_inputs(rows, bins, use_sigmoid):
    rng = np.random.default_rng(100000 * use_sigmoid + 1000 * bins + rows)
    hw = logit_half_width(bins, use_sigmoid)
    x = rng.uniform(-hw, hw, (rows, bins)).astype(np.float32)
    gt = rng.random((rows, bins)) < 0.15
    return x, gt


# ---- 4. the clamp and the floor -----------------------------------------------------------------------------------------------
SAT_ROWS, SAT_BINS = 70, 129


def saturated_inputs(use_sigmoid):
    """Every saturated p is exactly 0 or 1 in fp32 under any faithful expf, or sits near 9e-14 where the 1e-12 floor acts; no p
    is within a few ulp of 1 or denormal (logits about -104 to -87 are never used)."""
    rng = np.random.default_rng(400 + use_sigmoid)
    x = rng.uniform(-1.0, 1.0, (SAT_ROWS, SAT_BINS)).astype(np.float32)
    gt = rng.random((SAT_ROWS, SAT_BINS)) < 0.15
    if use_sigmoid:
        kind = rng.integers(0, 5, x.shape)
        for k, v in ((1, 30.0), (2, -30.0), (3, 110.0), (4, -110.0)):   # p = 1, 9.4e-14 (floor), 1, 0
            x[kind == k] = v
        return x, gt
    for q in range(SAT_ROWS):
        e = int(rng.integers(0, SAT_BINS))
        if q % 3 == 0:          # p_e rounds to exactly 1, the others sit near 9e-14 with the floor active
            x[q, e] += 30.0
            # true: gp_e = 0 and the row is well conditioned; false: the loss takes the -100 clamp at e
            gt[q, e] = (q // 3) % 2 == 0
        elif q % 3 == 1:        # the others underflow to exactly 0
            x[q, e] += 120.0
    return x, gt


def moved(p, ulps):
    """fp32 ``p`` with every ``0 < p < 1`` moved by ``ulps`` (an int or an int array) representable numbers."""
    p = np.asarray(p, np.float32)
    inside = (p > 0) & (p < 1)
    bits = p.view(np.int32) + np.where(inside, ulps, 0).astype(np.int32)
    return bits.view(np.float32)


def probe(x, gt, use_sigmoid):
    """The restatement at p moved by +4, -4 and a random +-4 ulp against itself: ``(worst relative move of the loss, worst move of
    a gradient element in units of its y)``.  An element with y == 0 must not move at all (reported as inf)."""
    p = ref.pixel_probs(x, use_sigmoid)
    loss, g, y = ref.pixel_loss_terms(x, gt, use_sigmoid)
    signs = np.where(np.random.default_rng(9).random(p.shape) < 0.5, -PROBE_ULP, PROBE_ULP)
    dl = dg = 0.0
    for ulps in (PROBE_ULP, -PROBE_ULP, signs):
        l2, g2, _ = ref.pixel_loss_terms(x, gt, use_sigmoid, p=moved(p, ulps))
        dl = max(dl, abs(l2 - loss) / abs(loss) if loss else (0.0 if l2 == loss else np.inf))
        d = np.abs(g2 - g)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(y > 0, d / y, np.where(d > 0, np.inf, 0.0))
        dg = max(dg, float(rel.max()))
    return dl, dg


def check_grad(got, g, y, what, scale=1.0):
    """Every element within ``LOSS_RTOL x y`` of the truth (both scaled by the upstream gradient); exactly 0 where y is 0.
    Prints and returns the worst error in units of y."""
    got = np.asarray(got, np.float64)
    g, y = g * scale, y * abs(scale)
    assert got.shape == g.shape
    zero = y == 0
    assert (got[zero] == 0).all(), f"{what}: {int((got[zero] != 0).sum())} elements with no term to form them from are not 0"
    err = np.abs(got - g)
    worst = float((err[~zero] / y[~zero]).max()) if (~zero).any() else 0.0
    print(f"{what}: worst gradient error {worst:.2e} of y, {int(zero.sum())} exact zeros")
    bad = err > LOSS_RTOL * y
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off, first {np.argwhere(bad)[0].tolist()}: {worst:.3e} of y"
    return worst


# ---- 5. the module at its default --------------------------------------------------------------------------------------------
MODULE_C = 32                               # secondfpn_out channels = 4 x embed_dims


def module_feats():
    return (0.5 * np.random.default_rng(50).standard_normal((B, N, MODULE_C, H, W))).astype(np.float32)
