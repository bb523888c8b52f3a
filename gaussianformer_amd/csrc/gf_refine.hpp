// gf_refine.hpp -- what the refinement step's translation units share (refine.hip: the tail alone, forward and backward;
// refine_mlp.hip: the modules' MLP and the tail in one launch, plain and saving; refine_mlp_train.hip: the modules' backward;
// DESIGN.md §3.12, §3.12b, §3.12c): the constants, the arguments, the moves between memory and the LDS tiles, a row's forward
// values and the forward tail on them, the argument checks, the tail's backward launch and the saved region's layout.
#pragma once
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
    int po, pa, pn;         // LDS pitches (odd) of the [rows, D] tiles, the anchor tile (C columns) and the narrow tile
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

// What the forward computes of one row before it writes anything, and what the backward recomputes: the row's first ten output
// and anchor columns and every intermediate value a gradient needs.
struct RefineRow {
    float o[10], av[10];
    float x[10];       // the columns after the refinement, before the clamp of xyz and the normalisation
    float s0[3];       // safe_sigmoid of the xyz output columns (restrict_xyz, version 2)
    float xyz[3], c0[3], u[3], t[3], orig[3], delta[3];
    float act[3], ssc[3];
    float norm, inv_norm, qv[4];
    float sopa;
};

// ro, ra: the row in the output tile and in the anchor tile.  Version 1 adds the anchor's columns from 10 on into the tile's
// row here (:82-84); the first ten stay in registers.
template <int VERSION>
__device__ __forceinline__ void refine_row_values(const RefineArgs &a, float *ro, const float *ra, RefineRow &v)
{
#pragma clang fp contract(off)
    const int opa = (a.flags & GF_REFINE_OPACITY) ? 1 : 0;
    const bool sig = !(a.flags & GF_REFINE_XYZ_IDENTITY), restrict_xyz = (a.flags & GF_REFINE_RESTRICT_XYZ) != 0;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        v.o[k] = ro[k];
        v.av[k] = k < a.C ? ra[k] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) v.s0[i] = v.c0[i] = v.u[i] = v.t[i] = v.orig[i] = v.delta[i] = 0.f;
#pragma unroll
    for (int k = 3; k < 10; ++k) v.x[k] = v.o[k];
    if (VERSION == 1) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (restrict_xyz) {                                        // :72-80
                v.s0[i] = safe_sigmoid(v.o[i]);
                v.x[i] = (2.f * v.s0[i] - 1.f) * a.unit[i];
            } else {
                v.x[i] = v.o[i];
            }
        }
#pragma unroll
        for (int k = 0; k < 10; ++k)
            if (k < a.R) v.x[k] += v.av[k];                            // :82-84
        for (int k = 10; k < a.R; ++k) ro[k] += ra[k];
#pragma unroll
        for (int i = 0; i < 3; ++i) v.xyz[i] = sig ? v.x[i] : clampf(v.x[i], kUnitLo, kUnitHi);  // :86-89
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            v.x[i] = 0.f;
            v.s0[i] = safe_sigmoid(v.o[i]);
            v.delta[i] = (2.f * v.s0[i] - 1.f) * a.unit[i];            // v2 :65
            v.c0[i] = sig ? safe_sigmoid(v.av[i]) : clampf(v.av[i], kUnitLo, kUnitHi);
            v.orig[i] = v.c0[i] * a.span[i] + a.lo[i];                 // :66, cartesian (utils.py:26-36)
            v.u[i] = ((v.orig[i] + v.delta[i]) - a.lo[i]) / a.span[i]; // :67-68, reverse_cartesian (utils.py:38-47)
            if (sig) {
                v.t[i] = clampf(v.u[i], kLogitLo, kLogitHi);
                v.xyz[i] = logf(v.t[i] / (1.f - v.t[i]));
            } else {
                v.xyz[i] = clampf(v.u[i], kUnitLo, kUnitHi);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v.act[i] = sig ? safe_sigmoid(v.xyz[i]) : (VERSION == 2 ? clampf(v.xyz[i], kUnitLo, kUnitHi) : v.xyz[i]);
        v.ssc[i] = safe_sigmoid(v.x[3 + i]);
    }
    v.norm = sqrtf(v.x[6] * v.x[6] + v.x[7] * v.x[7] + v.x[8] * v.x[8] + v.x[9] * v.x[9]);
    const UnitQuat q = unit_quat(v.x[6], v.x[7], v.x[8], v.x[9]);
    v.qv[0] = q.w; v.qv[1] = q.x; v.qv[2] = q.y; v.qv[3] = q.z;
    v.inv_norm = q.inv_norm;
    v.sopa = opa ? safe_sigmoid(ro[10]) : 0.f;
}

// The forward tail of one row: ro, its row of the output tile (the MLP's result after Scale), becomes its row of anchor_out;
// rn, its row of the narrow tile, receives the prediction's columns (kN*).  ra: its row of the anchor tile (C columns).
template <int VERSION>
__device__ __forceinline__ void refine_row_forward(const RefineArgs &a, float *ro, const float *ra, float *rn)
{
#pragma clang fp contract(off)
    const int opa = (a.flags & GF_REFINE_OPACITY) ? 1 : 0, sem0 = 10 + opa;
    const bool softmax = (a.flags & GF_REFINE_SEM_SOFTMAX) != 0, softplus = (a.flags & GF_REFINE_SEM_SOFTPLUS) != 0;
    RefineRow v;
    refine_row_values<VERSION>(a, ro, ra, v);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ro[i] = v.xyz[i];
        ro[3 + i] = v.x[3 + i];     // (the refined scale column, :82-84: other than o's only where refine_manual reaches it, R > 3)
        rn[kNMeans + i] = v.act[i] * a.span[i] + a.lo[i];
        rn[kNScales + i] = a.scale_lo + a.scale_span * v.ssc[i];
        if (VERSION == 2) {
            rn[kNOrig + i] = v.orig[i];
            rn[kNDelta + i] = v.delta[i];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) ro[6 + j] = rn[kNRot + j] = v.qv[j];
    if (opa) rn[kNOpa] = v.sopa;
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
            const float x = ro[sem0 + j];
            rn[kNSem + j] = softplus && !(x > 20.f) ? log1pf(expf(x)) : x;   // F.softplus: beta 1, threshold 20
        }
    }
}

// a wave's `rows` finished rows from its tiles to the forward's outputs, each as one contiguous run
template <int VERSION>
__device__ __forceinline__ void refine_store_forward(const RefineArgs &a, size_t b, const float *t_o, const float *t_n, int rows)
{
    const int opa = (a.flags & GF_REFINE_OPACITY) ? 1 : 0;
    tile_store(a.anchor_out, b, t_o, a.po, 0, a.D, a.D, rows);
    tile_store(a.means, b, t_n, a.pn, kNMeans, 3, 3, rows);
    tile_store(a.scales, b, t_n, a.pn, kNScales, 3, 3, rows);
    tile_store(a.rotations, b, t_n, a.pn, kNRot, 4, 4, rows);
    tile_store(a.opacities, b, t_n, a.pn, kNOpa, opa, opa, rows);
    tile_store(a.semantics, b, t_n, a.pn, kNSem, a.S, a.S, rows);
    if (VERSION == 2) {
        tile_store(a.original_means, b, t_n, a.pn, kNOrig, 3, 3, rows);
        tile_store(a.delta_means, b, t_n, a.pn, kNDelta, 3, 3, rows);
    }
}

// the checks every entry point shares, and the constants; 0 or GF_EINVAL (message set)
inline int refine_fill_args(RefineArgs &a, const char *who, int n, int D, int Da, int version, int flags, int R, int S, const double *consts)
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
// the forward's pointers that must be there; false (message set) = GF_EINVAL
inline bool refine_forward_outputs_present(int version, int flags, int S, const float *anchor_out, const float *means, const float *scales,
                                           const float *rotations, const float *opacities, const float *semantics,
                                           const float *original_means, const float *delta_means)
{
    return anchor_out && means && scales && rotations && (opacities || !(flags & GF_REFINE_OPACITY)) && (semantics || S == 0) &&
           (version == 1 || (original_means && delta_means));
}

// The tail's backward launch on filled arguments (refine.hip): gf_refine_backward's, and the first step of
// gf_refine_mlp_backward.  0 or GF_ELAUNCH, reported under `who`
int refine_launch_backward(const char *who, const RefineArgs &a, int version, hipStream_t stream);

// ---- the MLP's entry points (refine_mlp.hip, refine_mlp_train.hip) -----------------------------------------------------------
constexpr int kRmE = 128;
constexpr int kRmYPitch = 64;     // floats per row of the saved pre-Scale value: the last product's two accumulators

static const char *const kRmName[GF_REFINE_MLP_PARAMS] = {
    "layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias", "layers.4.weight", "layers.4.bias", "layers.5.weight", "layers.5.bias",
    "layers.7.weight", "layers.7.bias", "layers.9.weight", "layers.9.bias", "layers.10.weight", "layers.10.bias", "layers.11.scale"};

// what every launching entry point of the MLP refuses of its inputs once n > 0, in gf_refine_mlp_forward's order and words,
// under the name of the one that was called
inline int refine_mlp_check_inputs(const char *fn, const void *const *params, const float *instance_feature, const float *anchor_embed,
                                   const float *anchor)
{
    GF_REFUSE_AS(fn, params, "null params");
    for (int i = 0; i < GF_REFINE_MLP_PARAMS; ++i) {
        GF_REFUSE_AS(fn, params[i], "params[%d] (%s) is null", i, kRmName[i]);
        GF_REFUSE_AS(fn, !misaligned16(params[i]), "params[%d] (%s) = %p is not 16-byte aligned", i, kRmName[i], params[i]);
    }
    GF_REFUSE_AS(fn, instance_feature, "null instance_feature");
    GF_REFUSE_AS(fn, anchor_embed, "null anchor_embed");
    GF_REFUSE_AS(fn, anchor, "null anchor");
    GF_REFUSE_AS(fn, !misaligned16(instance_feature), "instance_feature = %p is not 16-byte aligned", (const void *)instance_feature);
    GF_REFUSE_AS(fn, !misaligned16(anchor_embed), "anchor_embed = %p is not 16-byte aligned", (const void *)anchor_embed);
    return GF_OK;
}

// What the saving forward keeps for the backward, sized and carved by one function (a null base: the size only): the four
// post-ReLU rows [4][n][128], the two LayerNorms' (mean, rstd) [2][n][2], the last Linear's result before Scale [n][64] (zero
// from D on) and the MLP's result o [n][D]
struct RefineMlpSaved { float *rows, *stat, *y, *o; size_t bytes; };
inline RefineMlpSaved refine_mlp_carve_saved(void *base, int n, int D)
{
    Carver c(base);
    RefineMlpSaved s;
    s.rows = c.take<float>((size_t)4 * n * kRmE);
    s.stat = c.take<float>((size_t)4 * n);
    s.y = c.take<float>((size_t)n * kRmYPitch);
    s.o = c.take<float>((size_t)n * D);
    s.bytes = c.bytes();
    return s;
}

}  // namespace gf
