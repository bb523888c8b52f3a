// The encoder's Gaussian refinement step: what SparseGaussian3DRefinementModule.forward (version 1,
// model/encoder/gaussian_encoder/refine_module.py:72-123) and SparseGaussian3DRefinementModuleV2.forward (version 2,
// refine_module_v2.py:62-107) compute after their MLP, in one launch forward and one backward.
//
// The reference strings 30-40 slices, stacks, cats, clamps, sigmoids and logs over an [n, D] tensor; autograd doubles that.
// Here one wave takes 64 consecutive rows.  A row is 4 D bytes (112 at D = 28), so a lane reading its own row from memory
// would touch 64 cache lines per instruction; instead the 64 rows -- contiguous in memory -- cross between memory and an
// LDS tile as one run of dwords (a wave instruction moves 256 contiguous bytes), and each lane reads its row from the tile.
// The tile's row pitch is odd, so the 64 lanes of a column read hit 64 different banks.  (An LDS-DMA load lands lane-linear
// and cannot write a padded pitch, so the tile is filled through registers.)  Every output leaves the same way: the lane
// writes its row into a tile, the wave stores the tile as one run.
//
// Arithmetic: fp32, unfused (contract(off)) and in the reference's operation order, with ocml's expf / logf / log1pf -- the
// inverse sigmoid of version 2 amplifies a rounding of its argument by up to 1e4 near its clamp, so this op stays within the
// error of torch's own fp32 evaluation rather than a v_exp_f32's 1e-6.  The backward recomputes the forward's values from
// (output, anchor) with the same code, so it needs no forward result.
//
// HBM traffic per row, forward: 4 (2 D + Da + 10 + opa + S [+ 6]) bytes.
#include "gf_common.hpp"

namespace gf {

constexpr int kRefMaxS = 32;              // semantic columns
// columns of the narrow tile: means 3, scales 3, rotations 4, opacity 1, original 3, delta 3, semantics S
constexpr int kNMeans = 0, kNScales = 3, kNRot = 6, kNOpa = 10, kNOrig = 11, kNDelta = 14, kNSem = 17;
constexpr float kUnitLo = 1e-6f, kUnitHi = (float)(1.0 - 1e-6);        // .clamp(min=1e-6, max=1-1e-6), the bounds as torch rounds them
constexpr float kLogitLo = (float)(1.0 - 0.9999), kLogitHi = 0.9999f;  // safe_inverse_sigmoid, model/utils/safe_ops.py:11-13
constexpr float kNormEps = 1e-12f;                                     // F.normalize

struct RefineArgs {
    const float *output, *anchor;
    float *anchor_out, *means, *scales, *rotations, *opacities, *semantics, *original_means, *delta_means;
    // backward: gradients of the forward's outputs (each may be null = zero), then what it writes
    const float *g_anchor_out, *g_means, *g_scales, *g_rotations, *g_opacities, *g_semantics, *g_original, *g_delta;
    float *grad_output, *grad_anchor;
    float lo[3], span[3], unit[3];
    float scale_lo, scale_span;
    int n, D, Da, R, S, C;  // C: anchor columns read (and grad_anchor columns that can be non-zero): R, or 3 in version 2
    int po, pa, pn;         // LDS pitches (odd) of the [64, D] tiles, the anchor tile (C columns) and the narrow tile
    int flags;
};

// `rows` rows of `w` floats, `gpitch` apart in memory, from row `row0` of g on, into columns col0 .. col0 + w of an LDS tile;
// g null = zeros.  With gpitch == w the rows are one contiguous run and lane i of step s reads dword 64 s + i of it.  The loads
// go out kTileBatch at a time before the first of them is written to the tile: one memory round trip per batch, where a
// load-then-write loop would pay one per step (28 in a row at D = 28).  All 64 lanes call.
constexpr int kTileBatch = 16;
__device__ __forceinline__ void tile_load(const float *g, size_t row0, int gpitch, float *tile, int pitch, int col0, int w, int rows)
{
    if (w <= 0) return;
    if (g) g += row0 * gpitch;
    int r = lane_id() / w, c = lane_id() % w;
    const int dq = 64 / w, dr = 64 % w, total = rows * w;
    for (int i0 = lane_id(); i0 < total; i0 += 64 * kTileBatch) {
        float v[kTileBatch];
        int at[kTileBatch];
#pragma unroll
        for (int j = 0; j < kTileBatch; ++j) {
            const bool live = i0 + 64 * j < total;
            at[j] = live ? r * pitch + col0 + c : -1;
            v[j] = live && g ? g[(size_t)r * gpitch + c] : 0.f;
            c += dr; r += dq;
            if (c >= w) { c -= w; ++r; }
        }
#pragma unroll
        for (int j = 0; j < kTileBatch; ++j)
            if (at[j] >= 0) tile[at[j]] = v[j];
    }
}
// The way back: columns col0 .. col0 + w of the tile to `rows` contiguous rows of `w` floats from row `row0` of g on; columns
// from `wvalid` on are written as zero (grad_anchor beyond the columns the op reads).
__device__ __forceinline__ void tile_store(float *g, size_t row0, const float *tile, int pitch, int col0, int w, int wvalid, int rows)
{
    if (w <= 0) return;
    g += row0 * w;
    int r = lane_id() / w, c = lane_id() % w;
    const int dq = 64 / w, dr = 64 % w;
    for (int i = lane_id(); i < rows * w; i += 64) {
        g[i] = c < wvalid ? tile[r * pitch + col0 + c] : 0.f;
        c += dr; r += dq;
        if (c >= w) { c -= w; ++r; }
    }
}

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
// torch.clamp's gradient mask: bounds included
__device__ __forceinline__ bool passes(float x, float lo, float hi) { return x >= lo && x <= hi; }

template <int VERSION, bool BACKWARD>
__global__ __launch_bounds__(64) void gf_refine_kernel(RefineArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ float lds[];
    const int po = a.po, pa = a.pa, pn = a.pn;
    float *t_o = lds;                  // output rows; forward: becomes anchor_out, backward: grad_output
    float *t_a = t_o + 64 * po;        // anchor columns < C; backward: becomes grad_anchor
    float *t_n = t_a + 64 * pa;        // the narrow outputs, or their gradients
    float *t_g = t_n + 64 * pn;        // backward: grad of anchor_out
    const int base = blockIdx.x * 64, rows = min(64, a.n - base), lane = lane_id();
    const int opa = (a.flags & GF_REFINE_OPACITY) ? 1 : 0, sem0 = 10 + opa;
    const bool sig = !(a.flags & GF_REFINE_XYZ_IDENTITY), restrict_xyz = (a.flags & GF_REFINE_RESTRICT_XYZ) != 0;
    const bool softmax = (a.flags & GF_REFINE_SEM_SOFTMAX) != 0, softplus = (a.flags & GF_REFINE_SEM_SOFTPLUS) != 0;

    const size_t b = base;
    tile_load(a.output, b, a.D, t_o, po, 0, a.D, rows);
    tile_load(a.anchor, b, a.Da, t_a, pa, 0, a.C, rows);
    if (BACKWARD) {
        tile_load(a.g_anchor_out, b, a.D, t_g, po, 0, a.D, rows);
        tile_load(a.g_means, b, 3, t_n, pn, kNMeans, 3, rows);
        tile_load(a.g_scales, b, 3, t_n, pn, kNScales, 3, rows);
        tile_load(a.g_rotations, b, 4, t_n, pn, kNRot, 4, rows);
        tile_load(a.g_opacities, b, opa, t_n, pn, kNOpa, opa, rows);
        tile_load(a.g_semantics, b, a.S, t_n, pn, kNSem, a.S, rows);
        if (VERSION == 2) {
            tile_load(a.g_original, b, 3, t_n, pn, kNOrig, 3, rows);
            tile_load(a.g_delta, b, 3, t_n, pn, kNDelta, 3, rows);
        }
    }
    __syncthreads();

    if (lane < rows) {
        float *ro = t_o + lane * po, *ra = t_a + lane * pa, *rn = t_n + lane * pn;
        float o[10], av[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            o[k] = ro[k];
            av[k] = k < a.C ? ra[k] : 0.f;
        }
        // ---- the forward's values (both directions)
        float x[10];       // the columns after the refinement, before the clamp of xyz and the normalisation
        float s0[3] = {0.f, 0.f, 0.f};        // safe_sigmoid of the xyz output columns (restrict_xyz, version 2)
        float xyz[3], c0[3] = {0.f, 0.f, 0.f}, u[3] = {0.f, 0.f, 0.f}, t[3] = {0.f, 0.f, 0.f}, orig[3], delta[3];
#pragma unroll
        for (int k = 3; k < 10; ++k) x[k] = o[k];
        if (VERSION == 1) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (restrict_xyz) {                                        // :72-80
                    s0[i] = safe_sigmoid(o[i]);
                    x[i] = (2.f * s0[i] - 1.f) * a.unit[i];
                } else {
                    x[i] = o[i];
                }
            }
#pragma unroll
            for (int k = 0; k < 10; ++k)
                if (k < a.R) x[k] += av[k];                                // :82-84
            for (int k = 10; k < a.R; ++k) ro[k] += ra[k];
#pragma unroll
            for (int i = 0; i < 3; ++i) xyz[i] = sig ? x[i] : clampf(x[i], kUnitLo, kUnitHi);  // :86-89
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                s0[i] = safe_sigmoid(o[i]);
                delta[i] = (2.f * s0[i] - 1.f) * a.unit[i];                // v2 :65
                c0[i] = sig ? safe_sigmoid(av[i]) : clampf(av[i], kUnitLo, kUnitHi);
                orig[i] = c0[i] * a.span[i] + a.lo[i];                     // :66, cartesian (utils.py:26-36)
                u[i] = ((orig[i] + delta[i]) - a.lo[i]) / a.span[i];       // :67-68, reverse_cartesian (utils.py:38-47)
                if (sig) {
                    t[i] = clampf(u[i], kLogitLo, kLogitHi);
                    xyz[i] = logf(t[i] / (1.f - t[i]));
                } else {
                    xyz[i] = clampf(u[i], kUnitLo, kUnitHi);
                }
            }
        }
        float act[3], ssc[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            act[i] = sig ? safe_sigmoid(xyz[i]) : (VERSION == 2 ? clampf(xyz[i], kUnitLo, kUnitHi) : xyz[i]);
            ssc[i] = safe_sigmoid(x[3 + i]);
        }
        const float norm = sqrtf(x[6] * x[6] + x[7] * x[7] + x[8] * x[8] + x[9] * x[9]);
        const UnitQuat q = unit_quat(x[6], x[7], x[8], x[9]);
        const float qv[4] = {q.w, q.x, q.y, q.z};
        const float sopa = opa ? safe_sigmoid(ro[10]) : 0.f;

        if (!BACKWARD) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                ro[i] = xyz[i];
                rn[kNMeans + i] = act[i] * a.span[i] + a.lo[i];
                rn[kNScales + i] = a.scale_lo + a.scale_span * ssc[i];
                if (VERSION == 2) {
                    rn[kNOrig + i] = orig[i];
                    rn[kNDelta + i] = delta[i];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) ro[6 + j] = rn[kNRot + j] = qv[j];
            if (opa) rn[kNOpa] = sopa;
            if (softmax) {
                float m = -INFINITY, sum = 0.f;
                for (int j = 0; j < a.S; ++j) m = fmaxf(m, ro[sem0 + j]);
                for (int j = 0; j < a.S; ++j) {
                    const float e = expf(ro[sem0 + j] - m);
                    rn[kNSem + j] = e;
                    sum += e;
                }
                for (int j = 0; j < a.S; ++j) rn[kNSem + j] = rn[kNSem + j] / sum;
            } else {
                for (int j = 0; j < a.S; ++j) {
                    const float v = ro[sem0 + j];
                    rn[kNSem + j] = softplus && !(v > 20.f) ? log1pf(expf(v)) : v;   // F.softplus: beta 1, threshold 20
                }
            }
        } else {
            // ---- gradients, in autograd's order: the heads of the prediction first, then anchor_out's own gradient joins
            float gx[10];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float dact = sig ? safe_sigmoid_grad(xyz[i], act[i])
                                       : (VERSION == 2 && !passes(xyz[i], kUnitLo, kUnitHi) ? 0.f : 1.f);
                gx[i] = t_g[lane * po + i] + rn[kNMeans + i] * a.span[i] * dact;
                gx[3 + i] = t_g[lane * po + 3 + i] + rn[kNScales + i] * a.scale_span * safe_sigmoid_grad(x[3 + i], ssc[i]);
            }
            float gq[4], dot = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                gq[j] = t_g[lane * po + 6 + j] + rn[kNRot + j];
                dot += gq[j] * qv[j];
            }
            // x / max(||x||, eps): below eps the divisor is a constant
#pragma unroll
            for (int j = 0; j < 4; ++j) gx[6 + j] = (norm >= kNormEps ? gq[j] - qv[j] * dot : gq[j]) * q.inv_norm;
            // columns from 10 on: the tile's own row takes the gradient (and the anchor's tile where it was added)
            if (opa) {
                const float g = t_g[lane * po + 10] + rn[kNOpa] * safe_sigmoid_grad(ro[10], sopa);
                ro[10] = g;
                if (10 < a.C) ra[10] = g;
            }
            if (softmax) {
                float m = -INFINITY, sum = 0.f, gy = 0.f;
                for (int j = 0; j < a.S; ++j) m = fmaxf(m, ro[sem0 + j]);
                for (int j = 0; j < a.S; ++j) {
                    const float e = expf(ro[sem0 + j] - m);
                    ro[sem0 + j] = e;
                    sum += e;
                }
                for (int j = 0; j < a.S; ++j) {
                    ro[sem0 + j] = ro[sem0 + j] / sum;
                    gy += rn[kNSem + j] * ro[sem0 + j];
                }
                for (int j = 0; j < a.S; ++j) {
                    const float g = t_g[lane * po + sem0 + j] + ro[sem0 + j] * (rn[kNSem + j] - gy);
                    ro[sem0 + j] = g;
                    if (sem0 + j < a.C) ra[sem0 + j] = g;
                }
            } else {
                for (int j = 0; j < a.S; ++j) {
                    const float v = ro[sem0 + j];
                    float g = rn[kNSem + j];
                    if (softplus && !(v > 20.f)) {
                        const float z = expf(v);
                        g = g * z / (z + 1.f);
                    }
                    g += t_g[lane * po + sem0 + j];
                    ro[sem0 + j] = g;
                    if (sem0 + j < a.C) ra[sem0 + j] = g;
                }
            }
            if (VERSION == 1) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (!sig && !passes(x[i], kUnitLo, kUnitHi)) gx[i] = 0.f;
                }
#pragma unroll
                for (int k = 0; k < 10; ++k) {
                    if (k < a.C) ra[k] = gx[k];
                    ro[k] = (k < 3 && restrict_xyz) ? gx[k] * a.unit[k] * 2.f * safe_sigmoid_grad(o[k], s0[k]) : gx[k];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    float gu;   // through reverse_cartesian: the clamp, then log(t / (1 - t))
                    if (sig) gu = passes(u[i], kLogitLo, kLogitHi) ? gx[i] / (t[i] * (1.f - t[i])) : 0.f;
                    else gu = passes(u[i], kUnitLo, kUnitHi) ? gx[i] : 0.f;
                    const float gm = gu / a.span[i];
                    const float g_delta = gm + rn[kNDelta + i], g_orig = gm + rn[kNOrig + i];
                    ro[i] = g_delta * a.unit[i] * 2.f * safe_sigmoid_grad(o[i], s0[i]);
                    ra[i] = g_orig * a.span[i] * (sig ? safe_sigmoid_grad(av[i], c0[i]) : (passes(av[i], kUnitLo, kUnitHi) ? 1.f : 0.f));
                }
#pragma unroll
                for (int k = 3; k < 10; ++k) ro[k] = gx[k];
            }
        }
    }
    __syncthreads();

    if (!BACKWARD) {
        tile_store(a.anchor_out, b, t_o, po, 0, a.D, a.D, rows);
        tile_store(a.means, b, t_n, pn, kNMeans, 3, 3, rows);
        tile_store(a.scales, b, t_n, pn, kNScales, 3, 3, rows);
        tile_store(a.rotations, b, t_n, pn, kNRot, 4, 4, rows);
        tile_store(a.opacities, b, t_n, pn, kNOpa, opa, opa, rows);
        tile_store(a.semantics, b, t_n, pn, kNSem, a.S, a.S, rows);
        if (VERSION == 2) {
            tile_store(a.original_means, b, t_n, pn, kNOrig, 3, 3, rows);
            tile_store(a.delta_means, b, t_n, pn, kNDelta, 3, 3, rows);
        }
    } else {
        tile_store(a.grad_output, b, t_o, po, 0, a.D, a.D, rows);
        tile_store(a.grad_anchor, b, t_a, pa, 0, a.Da, a.C, rows);
    }
}

static size_t lds_bytes(const RefineArgs &a, bool backward) { return (size_t)64 * 4 * (a.po * (backward ? 2 : 1) + a.pa + a.pn); }

// the checks both entry points share, and the constants; 0 or GF_EINVAL (message set)
static int fill_args(RefineArgs &a, const char *who, int n, int D, int Da, int version, int flags, int R, int S, const double *consts)
{
    const int all = GF_REFINE_RESTRICT_XYZ | GF_REFINE_XYZ_IDENTITY | GF_REFINE_OPACITY | GF_REFINE_SEM_SOFTMAX | GF_REFINE_SEM_SOFTPLUS;
    const int opa = (flags & GF_REFINE_OPACITY) ? 1 : 0;
    const char *bad = nullptr;
    if (n < 0 || (version != 1 && version != 2)) bad = "bad n or version (1 or 2)";
    else if ((flags & ~all) || ((flags & GF_REFINE_SEM_SOFTMAX) && (flags & GF_REFINE_SEM_SOFTPLUS))) bad = "bad flags";
    else if (S < 0 || S > kRefMaxS) bad = "S must be in 0 .. 32";
    else if (D != 10 + opa + S) bad = "D must be 10 + opacity + S";
    else if (R < 0 || R > D) bad = "R must be in 0 .. D";
    else if (Da < (version == 1 ? R : 3)) bad = "Da is smaller than the anchor columns read (R, or 3 in version 2)";
    else if (!consts) bad = "null consts";
    if (bad) {
        set_error("%s: %s", who, bad);
        return GF_EINVAL;
    }
    a.n = n; a.D = D; a.Da = Da; a.S = S; a.flags = flags;
    a.R = version == 1 ? R : 0;
    a.C = version == 1 ? R : 3;
    for (int k = 0; k < 3; ++k) {
        a.lo[k] = (float)consts[k];
        a.span[k] = (float)(consts[3 + k] - consts[k]);   // the difference in double, as the reference's Python floats
        a.unit[k] = (float)consts[8 + k];
    }
    a.po = D | 1; a.pa = a.C | 1; a.pn = (kNSem + S) | 1;
    a.scale_lo = (float)consts[6];
    a.scale_span = (float)(consts[7] - consts[6]);
    return GF_OK;
}

}  // namespace gf

extern "C" int gf_refine_forward(int n, int D, int Da, int version, int flags, int R, int S, const double *consts, const float *output,
                                 const float *anchor, float *anchor_out, float *means, float *scales, float *rotations,
                                 float *opacities, float *semantics, float *original_means, float *delta_means, void *stream_)
{
    using namespace gf;
    RefineArgs a{};
    if (int rc = fill_args(a, __func__, n, D, Da, version, flags, R, S, consts)) return rc;
    if (n == 0) return GF_OK;
    GF_CHECK_ARG(output && (anchor || a.C == 0) && anchor_out && means && scales && rotations && (opacities || !(flags & GF_REFINE_OPACITY)) &&
                     (semantics || S == 0) && (version == 1 || (original_means && delta_means)), "null pointer");
    a.output = output; a.anchor = anchor; a.anchor_out = anchor_out; a.means = means; a.scales = scales; a.rotations = rotations;
    a.opacities = opacities; a.semantics = semantics; a.original_means = original_means; a.delta_means = delta_means;
    const dim3 grid((n + 63) / 64), block(64);
    if (version == 1) hipLaunchKernelGGL((gf_refine_kernel<1, false>), grid, block, lds_bytes(a, false), (hipStream_t)stream_, a);
    else hipLaunchKernelGGL((gf_refine_kernel<2, false>), grid, block, lds_bytes(a, false), (hipStream_t)stream_, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_refine_backward(int n, int D, int Da, int version, int flags, int R, int S, const double *consts, const float *output,
                                  const float *anchor, const float *grad_anchor_out, const float *grad_means, const float *grad_scales,
                                  const float *grad_rotations, const float *grad_opacities, const float *grad_semantics,
                                  const float *grad_original_means, const float *grad_delta_means, float *grad_output,
                                  float *grad_anchor, void *stream_)
{
    using namespace gf;
    RefineArgs a{};
    if (int rc = fill_args(a, __func__, n, D, Da, version, flags, R, S, consts)) return rc;
    if (n == 0) return GF_OK;
    GF_CHECK_ARG(output && (anchor || a.C == 0) && grad_output && (grad_anchor || Da == 0), "null pointer");
    a.output = output; a.anchor = anchor;
    a.g_anchor_out = grad_anchor_out; a.g_means = grad_means; a.g_scales = grad_scales; a.g_rotations = grad_rotations;
    a.g_opacities = grad_opacities; a.g_semantics = grad_semantics; a.g_original = grad_original_means; a.g_delta = grad_delta_means;
    a.grad_output = grad_output; a.grad_anchor = grad_anchor;
    const dim3 grid((n + 63) / 64), block(64);
    if (version == 1) hipLaunchKernelGGL((gf_refine_kernel<1, true>), grid, block, lds_bytes(a, true), (hipStream_t)stream_, a);
    else hipLaunchKernelGGL((gf_refine_kernel<2, true>), grid, block, lds_bytes(a, true), (hipStream_t)stream_, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
