// gf_rows.hpp -- what the row-wise MFMA kernels share (anchor_embed.hip, ffn.hip, ffn_train.hip, refine_mlp.hip, refine_mlp_train.hip,
// deform_dense.hip / gf_deform.hpp; the training backwards' parts on the same layout: gf_rows_bwd.hpp;
// DESIGN.md §3.12b, §3.12c, §3.13, §3.13c, §3.13e): the register layout in which a wave holds 32 rows of 128-feature blocks, the LayerNorm on it, the staging of a
// weight chunk through LDS, the chunk's 64 MFMAs and the store of a finished tile.
//
// The layout.  A workgroup of four waves owns 128 rows, a wave 32 of them.  Every product is Y^T = W X^T on
// v_mfma_f32_32x32x2_f32: the accumulator's columns are the wave's rows, its rows features, four accumulators hold a block of
// 128 features.  Lane (j = lane % 32, h = lane / 32) holds 64 features of row j per block:
//     feature(b, r, h) = 32 b + 8 (r >> 2) + 4 h + (r & 3)         b: accumulator, r: its register
// and MFMA step (b, r) sums over k = feature(b, r, 0) and feature(b, r, 1), so a product's accumulators are the next product's
// B operands as they stand.
#pragma once
#include "gf_common.hpp"

namespace gf {

constexpr int kRowTile = 128;      // rows per workgroup, 32 per wave
constexpr int kRowPitch4 = 9;      // float4 per staged weight row: 32 floats + 4 of padding (ds_read_b128 of 16 lanes: all 64 banks)
constexpr int kRowOutPitch = 68;   // floats per row of the output staging tile: 64 features + 4 of padding
constexpr float kRowLnEps = 1e-5f;

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

template <int N> __device__ __forceinline__ float tree_sum(const float *p)
{
    if constexpr (N == 1) return p[0];
    else return tree_sum<N / 2>(p) + tree_sum<N / 2>(p + N / 2);
}

// v <- LayerNorm(v) over the 32 NB features of the lane's row (biased variance, two passes), given the lane's own sum of its
// 16 NB values; gam, bet: the LayerNorm's weight and bias in LDS, 8 NB float4 each.  One exchange with lane ^ 32 completes
// each sum.  SAVE: (mean, rstd) go to st2 (null: not stored)
template <bool SAVE, int NB>
__device__ __forceinline__ void ln_rows(f32x16 (&v)[NB], float lane_sum, const float4 *gam, const float4 *bet, int h, float *st2 = nullptr)
{
    float part[NB];
    const float mean = wave_xor_reduce_strided(lane_sum, 32, Sum()) * (1.f / (32 * NB));
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        float s = 0.f, d0 = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float d = v[b][r] - mean;
            v[b][r] = d;
            // SAVE spells out the fusions the plain forward's build makes -- d0 d0 + (d1 d1) rounds the SECOND product, every
            // later term is one FMA -- because its stores change what gets vectorised, and a packed multiply followed by a
            // scalar add is not contracted.  The plain forward keeps the expressions its instruction stream was built from:
            // spelled out there too, the same bits come 5 % slower (another register allocation: 470.7 against 448.0 us at
            // A = 144 000, 96.2 against 93.4 at 6 400).  tests/test_anchor_encoder_train_gpu.py holds the two together
            if constexpr (SAVE) {
                if (r == 0) d0 = d;
                else if (r == 1) s = __builtin_fmaf(d0, d0, d * d);
                else s = __builtin_fmaf(d, d, s);
            } else {
                s += d * d;
            }
        }
        part[b] = s;
    }
    const float var = wave_xor_reduce_strided(tree_sum<NB>(part), 32, Sum()) * (1.f / (32 * NB));
    const float rstd = 1.f / sqrtf(var + kRowLnEps);
    if constexpr (SAVE) {
        if (st2 && h == 0) *reinterpret_cast<float2 *>(st2) = make_float2(mean, rstd);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 gg = gam[8 * b + 2 * m + h], ee = bet[8 * b + 2 * m + h];
            const float gv[4] = {gg.x, gg.y, gg.z, gg.w}, ev[4] = {ee.x, ee.y, ee.z, ee.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (SAVE) v[b][4 * m + i] = __builtin_fmaf(v[b][4 * m + i] * rstd, gv[i], ev[i]);
                else v[b][4 * m + i] = v[b][4 * m + i] * rstd * gv[i] + ev[i];
            }
        }
    }
}

// ln_rows<true, 4> of a row whose four blocks are held by the four waves of a workgroup, one each (the 32-row kernels): y is
// wave wv's block, lane_sum the lane's sum of it; the four blocks' sums meet in s_sum, so every wave of the workgroup calls it
// together (it holds barriers).  vec(which, m): the float4 of the LayerNorm's weight (which = 0) or bias (1) at the lane's
// features 32 wv + 8 m + 4 h .., from wherever the caller keeps them.  The same bits as ln_rows<true, 4> on the whole row
template <class Vec>
__device__ __forceinline__ void ln_rows_split(f32x16 &y, float lane_sum, float (&s_sum)[2][4][64], int wv, int l, Vec &&vec)
{
    auto total = [&](int which, float mine) {
        s_sum[which][wv][l] = mine;
        __syncthreads();
        const float part[4] = {s_sum[which][0][l], s_sum[which][1][l], s_sum[which][2][l], s_sum[which][3][l]};
        return wave_xor_reduce_strided(tree_sum<4>(part), 32, Sum()) * (1.f / 128);
    };
    const float mean = total(0, lane_sum);
    float sq = 0.f, d0 = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float d = y[r] - mean;
        y[r] = d;
        if (r == 0) d0 = d;
        else if (r == 1) sq = __builtin_fmaf(d0, d0, d * d);
        else sq = __builtin_fmaf(d, d, sq);
    }
    const float rstd = 1.f / sqrtf(total(1, sq) + kRowLnEps);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float4 gg = vec(0, m), ee = vec(1, m);
        const float gv[4] = {gg.x, gg.y, gg.z, gg.w}, ev[4] = {ee.x, ee.y, ee.z, ee.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) y[4 * m + i] = __builtin_fmaf(y[4 * m + i] * rstd, gv[i], ev[i]);
    }
}

// v <- LayerNorm(relu(v + bias)) over the 128 features of the lane's row (biased variance, two passes); p: the stage's
// three vectors in LDS (32 float4 each: bias, LayerNorm weight, LayerNorm bias).  SAVE: the lane also stores its 64 post-ReLU
// values to rrow (its row of the stage's saved rows, null for a row past n) as float4s from the registers, and (mean, rstd)
// to st2
template <bool SAVE>
__device__ __forceinline__ void relu_ln(f32x16 (&v)[4], const float4 *p, int h, float *rrow = nullptr, float *st2 = nullptr)
{
    float part[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 bb = p[8 * b + 2 * m + h];
            const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float x = v[b][4 * m + i] + bv[i];
                x = x < 0.f ? 0.f : x;     // (not fmaxf: a NaN stays a NaN, as torch's relu keeps it)
                v[b][4 * m + i] = x;
                s += x;
            }
            if constexpr (SAVE) {
                if (rrow)
                    *reinterpret_cast<float4 *>(rrow + 32 * b + 8 * m + 4 * h) =
                        make_float4(v[b][4 * m], v[b][4 * m + 1], v[b][4 * m + 2], v[b][4 * m + 3]);
            }
        }
        part[b] = s;
    }
    ln_rows<SAVE, 4>(v, (part[0] + part[1]) + (part[2] + part[3]), p + 32, p + 64, h, rrow ? st2 : nullptr);
}

// A weight chunk: 128 rows x 32 floats of a matrix w in torch's layout from column col0 on, ld = the matrix's row length.
// Thread t of 256 takes rows t / 8 + 32 i, float4 t % 8: fetched from L2 into registers, then written to an LDS buffer of
// 128 x kRowPitch4 float4 (the two halves of the double buffering: fetch before a chunk's MFMAs, stash after them)
__device__ __forceinline__ void chunk_fetch(float4 (&pre)[4], const float *w, size_t ld, int col0, int t)
{
    const int ff = t >> 3, fq = t & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) pre[i] = ld4(w + (size_t)(ff + 32 * i) * ld + col0 + 4 * fq);
}
// ... of a matrix that has only `rows` rows from w on (any number, <= 0 included): a row past them is staged as zeros and
// never loaded
__device__ __forceinline__ void chunk_fetch_rows(float4 (&pre)[4], const float *w, size_t ld, int col0, int t, int rows)
{
    const int ff = t >> 3, fq = t & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        pre[i] = ff + 32 * i < rows ? ld4(w + (size_t)(ff + 32 * i) * ld + col0 + 4 * fq) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void chunk_stash(float4 *buf, const float4 (&pre)[4], int t)
{
    const int ff = t >> 3, fq = t & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) buf[(ff + 32 * i) * kRowPitch4 + fq] = pre[i];
}
// acc += W_chunk xb^T: the staged chunk's 32 input columns against the 32 features that xb, one register block, holds; NFB
// accumulators take the chunk's first 32 NFB rows
template <int NFB>
__device__ __forceinline__ void chunk_mfma(f32x16 (&acc)[NFB], const f32x16 &xb, const float4 *buf, int j, int h)
{
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int fb = 0; fb < NFB; ++fb) {
            const float4 w4 = buf[(32 * fb + j) * kRowPitch4 + 2 * m + h];
            acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w4.x, xb[4 * m + 0], acc[fb], 0, 0, 0);
            acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w4.y, xb[4 * m + 1], acc[fb], 0, 0, 0);
            acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w4.z, xb[4 * m + 2], acc[fb], 0, 0, 0);
            acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w4.w, xb[4 * m + 3], acc[fb], 0, 0, 0);
        }
    }
}

// The wave's 32 finished rows of 128 features, x, to out[row0 + ..][128] through its LDS tile so (32 x kRowOutPitch floats),
// 64 features at a time: the lane writes its row's float4s, the wave reads four rows per instruction back and stores runs of
// 256 bytes.  Rows from n on are not stored.  Every wave of the workgroup calls it together (it holds barriers)
__device__ __forceinline__ void store_rows(float *so, const f32x16 (&x)[4], float *out, int row0, int n, int l, int j, int h)
{
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const f32x16 &v = x[2 * half + bb];
                *reinterpret_cast<float4 *>(so + j * kRowOutPitch + 32 * bb + 8 * m + 4 * h) =
                    make_float4(v[4 * m], v[4 * m + 1], v[4 * m + 2], v[4 * m + 3]);
            }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = 4 * i + (l >> 4), col = 4 * (l & 15);
            const float4 v = *reinterpret_cast<const float4 *>(so + r * kRowOutPitch + col);
            if (row0 + r < n) *reinterpret_cast<float4 *>(out + (size_t)(row0 + r) * 128 + 64 * half + col) = v;
        }
        __syncthreads();
    }
}
static_assert(4 * 32 * kRowOutPitch <= 2 * 128 * kRowPitch4 * 4, "the output staging tiles fit the two weight buffers");

// store_rows for NFB <= 4 blocks and a matrix of `pitch` floats per row: the first ncols (a multiple of 4, <= 32 NFB) of the
// blocks' features go to columns col0 .. col0 + ncols of out's rows; nothing else is written
template <int NFB>
__device__ __forceinline__ void store_cols(float *so, const f32x16 (&x)[NFB], float *out, size_t pitch, int col0, int ncols, int row0, int n,
                                           int l, int j, int h)
{
#pragma unroll
    for (int half = 0; half < (NFB + 1) / 2; ++half) {
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            if (2 * half + bb >= NFB) continue;
            const f32x16 &v = x[2 * half + bb < NFB ? 2 * half + bb : 0];
#pragma unroll
            for (int m = 0; m < 4; ++m)
                *reinterpret_cast<float4 *>(so + j * kRowOutPitch + 32 * bb + 8 * m + 4 * h) =
                    make_float4(v[4 * m], v[4 * m + 1], v[4 * m + 2], v[4 * m + 3]);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = 4 * i + (l >> 4), col = 64 * half + 4 * (l & 15);
            const float4 v = *reinterpret_cast<const float4 *>(so + r * kRowOutPitch + 4 * (l & 15));
            if (row0 + r < n && col < ncols) *reinterpret_cast<float4 *>(out + (size_t)(row0 + r) * pitch + col0 + col) = v;
        }
        __syncthreads();
    }
}

// The lane's 16 NB values of NB blocks of its row, in the layout above, from / to the row at p (32 NB floats, 16-byte aligned)
// as float4s
template <int NB>
__device__ __forceinline__ void load_row(f32x16 (&x)[NB], const float *p, int h)
{
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 v = ld4(p + 32 * b + 8 * m + 4 * h);
            x[b][4 * m] = v.x; x[b][4 * m + 1] = v.y; x[b][4 * m + 2] = v.z; x[b][4 * m + 3] = v.w;
        }
}
template <int NB>
__device__ __forceinline__ void store_row_regs(float *p, const f32x16 (&x)[NB], int h)
{
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int m = 0; m < 4; ++m)
            *reinterpret_cast<float4 *>(p + 32 * b + 8 * m + 4 * h) = make_float4(x[b][4 * m], x[b][4 * m + 1], x[b][4 * m + 2], x[b][4 * m + 3]);
}
template <int NB>
__device__ __forceinline__ void zero_rows(f32x16 (&x)[NB])
{
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) x[b][r] = 0.f;
}
// load_row where the lane has a row, zeros where it has none (nothing is loaded then)
template <int NB>
__device__ __forceinline__ void load_row_or_zero(f32x16 (&x)[NB], const float *p, bool valid, int h)
{
    if (valid) load_row(x, p, h);
    else zero_rows(x);
}

}  // namespace gf
