// gf_rows_bwd.hpp -- what the native training backwards share on gf_rows.hpp's layout (anchor_embed.hip, ffn_train.hip,
// refine_mlp_train.hip, deform_dense_train.hip; the organisation: DESIGN.md §3.13b): the sum of a per-lane value over a tile's rows, the transposed
// product dX^T = W^T dZ^T through LDS, the LayerNorm's data backward on registers, the weight gradient's row loop and the
// fixed-order sum of the partials.  Every order of additions here is part of the results' bits
// (tests/test_train_step_digests_gpu.py).
#pragma once
#include "gf_rows.hpp"

namespace gf {

// dst[0 .. 32 NB) = the sum over the tile's rows of f(b, r), the lane's value at feature(b, r, h) of its row (rows past n add
// 0): sum32_last over a wave's 32 rows, then the four waves in their order.  Every wave calls it together (two barriers)
template <int NB, class F>
__device__ __forceinline__ void tile_sum(F f, bool valid, float (*s_part)[128], float *dst, int t, int wv, int j, int h)
{
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float s = sum32_last(valid ? f(b, r) : 0.f);
            if (j == 31) s_part[wv][32 * b + 8 * (r >> 2) + 4 * h + (r & 3)] = s;
        }
    __syncthreads();
    if (t < 32 * NB) dst[t] = (s_part[0][t] + s_part[1][t]) + (s_part[2][t] + s_part[3][t]);
    __syncthreads();
}

// acc[fb] += (W^T g)'s features 32 fb ..: w points at W[o0][k0] of a row-major matrix with rows of ld floats, g holds the
// features o0 .. o0 + 32 NC of the wave's rows, acc the features k0 .. k0 + 128.  W goes through LDS (buf0, buf1: 32 x
// kRowTPitch floats each) in NC chunks of 32 rows o (the features of g's register block c) x 128 floats, double buffered; step
// (c, r) sums over o = feature(c, r, 0 / 1) with g's register as the B operand as it stands and W[o][32 fb + j] read along the
// row.  MASK_ROWS: W has only nrows rows from w on, the others are supplied as zero -- the row index is clamped and the value
// masked, nothing beyond the tensor is loaded.  Every wave of the workgroup calls it together; it ends behind a barrier
constexpr int kRowTPitch = 136;    // floats per staged row: rows 4 apart lie 32 banks apart
template <int NC, bool MASK_ROWS>
__device__ __forceinline__ void product_t(f32x16 (&acc)[4], const f32x16 (&g)[NC], const float *w, size_t ld, int nrows, float *buf0,
                                          float *buf1, int t, int j, int h)
{
    constexpr int P = kRowTPitch;
    const int rr = t >> 3, fq = t & 7;
    float4 pre[4];
    auto fetch = [&](int c) {
        const int o = 32 * c + rr;
        const float *src = w + (size_t)(MASK_ROWS ? min(o, nrows - 1) : o) * ld;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 v = ld4(src + 4 * (fq + 8 * i));
            pre[i] = !MASK_ROWS || o < nrows ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stash = [&](float *buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4 *>(buf + rr * P + 4 * (fq + 8 * i)) = pre[i];
    };
    fetch(0);
    stash(buf0);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float *cur = c & 1 ? buf1 : buf0;
        if (c + 1 < NC) fetch(c + 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float *wrow = cur + (8 * (r >> 2) + 4 * h + (r & 3)) * P + j;
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[32 * fb], g[c][r], acc[fb], 0, 0, 0);
        }
        if (c + 1 < NC) stash(c & 1 ? buf0 : buf1);
        __syncthreads();
    }
}

// The LayerNorm's data backward on registers: g, the gradient behind the norm, becomes the gradient before it,
//     dn = g gamma,  g <- rstd (dn - mean(dn) - n^ mean(dn n^))
// over the 32 NB features of the lane's row; nhat: the normalised row n^ = (x - mean) rstd, gam: the norm's weight in memory.
// One exchange with lane ^ 32 completes each mean
template <int NB>
__device__ __forceinline__ void ln_bwd_rows(f32x16 (&g)[NB], const f32x16 (&nhat)[NB], const float *gam, float rstd, int h)
{
    float p1[NB], p2[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 gg = ld4(gam + 32 * b + 8 * m + 4 * h);
            const float gv[4] = {gg.x, gg.y, gg.z, gg.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dn = g[b][4 * m + i] * gv[i];
                s1 += dn;
                s2 += dn * nhat[b][4 * m + i];
                g[b][4 * m + i] = dn;
            }
        }
        p1[b] = s1;
        p2[b] = s2;
    }
    const float m1 = wave_xor_reduce_strided(tree_sum<NB>(p1), 32, Sum()) * (1.f / (32 * NB));
    const float m2 = wave_xor_reduce_strided(tree_sum<NB>(p2), 32, Sum()) * (1.f / (32 * NB));
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) g[b][r] = rstd * (g[b][r] - m1 - nhat[b][r] * m2);
}

// The weight gradient's row loop: acc[cb] += left^T right over the rows rb .. re of a block that ends at r1, a 128 x 128 piece
// with A = left[row][o] and B = right[row][32 cb + j], two rows a step (lanes 0-31 one, lanes 32-63 the other), loaded from the
// row-major arrays as they lie, four steps' loads out together.  left and right point at the lane's column of their arrays'
// first rows, which are the rows lsub and rsub (a chunk's array starts at the chunk's first row; ldl, ldr: floats a row).  A
// lane beyond r1 supplies 0 (a select) and loads row r1 - 1.  How the right operand is formed:
//     kWgAsIs  right as it lies
//     kWgSum   right + right2 (the same pitch)
//     kWgNorm  the LayerNorm of right from the saved (mean, rstd) at stat[2 row], in the saving forward's expression, with the
//              lane's four weights gv and biases ev
// One call is one fp32 chain; who needs shorter chains calls it per run of rows (refine_mlp_train.hip's flush into double)
enum { kWgAsIs, kWgSum, kWgNorm };
template <int KIND>
__device__ __forceinline__ void wgrad_rows(f32x16 (&acc)[4], const float *left, size_t ldl, int lsub, const float *right, const float *right2,
                                           size_t ldr, int rsub, const float *stat, const float (&gv)[4], const float (&ev)[4], int rb, int re,
                                           int r1, int h)
{
    for (int r = rb; r < re; r += 8) {
        float av[4], xv[4][4];
        float2 ms[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = min(r + 2 * q + h, r1 - 1);
            av[q] = left[(size_t)(row - lsub) * ldl];
            if constexpr (KIND == kWgNorm) ms[q] = *reinterpret_cast<const float2 *>(stat + (size_t)row * 2);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                xv[q][cb] = right[(size_t)(row - rsub) * ldr + 32 * cb];
                if constexpr (KIND == kWgSum) xv[q][cb] = xv[q][cb] + right2[(size_t)(row - rsub) * ldr + 32 * cb];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool live = r + 2 * q + h < r1;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                float bv = xv[q][cb];
                if constexpr (KIND == kWgNorm) bv = __builtin_fmaf((bv - ms[q].x) * ms[q].y, gv[cb], ev[cb]);
                acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(live ? av[q] : 0.f, live ? bv : 0.f, acc[cb], 0, 0, 0);
            }
        }
    }
}
// the lane's 64 values of a finished 128 x 128 piece, v(cb, r), to dst[o][k] (ldd floats a row): o = 32 wv + feature(0, r, h),
// k = 32 cb + j
template <class V>
__device__ __forceinline__ void wgrad_store(float *dst, size_t ldd, V v, int wv, int j, int h)
{
    dst += j;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(size_t)(32 * wv + 8 * (r >> 2) + 4 * h + (r & 3)) * ldd + 32 * cb] = v(cb, r);
}

// dst[e] = the sum over `count` partials, `stride` floats apart, in a fixed order, accumulated in Acc and rounded once to
// float.  slots == 1: a thread per element, four interleaved running sums, then their tree.  slots == kRowsSumSlots (few
// elements, many partials; built for Acc = double only, a float job is taken with slots == 1): 16 threads per element, thread k
// takes the partials k, k + 16, .. the same way, and the 16 results meet in a tree.  K > 0: dst is a thin weight [len / K][K]
// and its partials are rows of 32.  count == 0 stores zeros.
// Launched with (the longest job's workgroups, NJ jobs) x 256 threads; a job of len 0 does nothing
constexpr int kRowsSumSlots = 16;
struct RowsSumJob { const float *src; float *dst; size_t stride; int count, len, K, slots; };
template <int NJ> struct RowsSumArgs { RowsSumJob job[NJ]; };
template <class Acc, int NJ>
__global__ __launch_bounds__(256) void rows_sum_kernel(RowsSumArgs<NJ> a)
{
    constexpr bool kTwoLevel = sizeof(Acc) == sizeof(double);
    const RowsSumJob &jb = a.job[blockIdx.y];
    const int slots = kTwoLevel ? jb.slots : 1, per = 256 / slots;          // elements of a workgroup
    if ((int)blockIdx.x * per >= jb.len) return;            // (the whole workgroup)
    const int el = threadIdx.x % per, slot = threadIdx.x / per, e = blockIdx.x * per + el;
    Acc s[4] = {0, 0, 0, 0};
    if (e < jb.len) {
        const float *src = jb.src + (jb.K ? (e / jb.K) * 32 + e % jb.K : e);
        int i = slot;
        for (; i + 3 * slots < jb.count; i += 4 * slots) {
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += (Acc)src[(size_t)(i + q * slots) * jb.stride];
        }
        for (; i < jb.count; i += slots) s[0] += (Acc)src[(size_t)i * jb.stride];
    }
    const Acc v = (s[0] + s[1]) + (s[2] + s[3]);
    if constexpr (kTwoLevel) {
        if (slots > 1) {     // (the whole workgroup)
            __shared__ Acc s_sum[256];
            s_sum[threadIdx.x] = v;
            __syncthreads();
            if (slot == 0 && e < jb.len) {
                Acc p[kRowsSumSlots];
#pragma unroll
                for (int k = 0; k < kRowsSumSlots; ++k) p[k] = s_sum[k * per + el];
#pragma unroll
                for (int w = kRowsSumSlots / 2; w > 0; w >>= 1)
#pragma unroll
                    for (int k = 0; k < w; ++k) p[k] = p[2 * k] + p[2 * k + 1];
                jb.dst[e] = (float)p[0];
            }
            return;
        }
    }
    if (e < jb.len) jb.dst[e] = (float)v;
}

}  // namespace gf
