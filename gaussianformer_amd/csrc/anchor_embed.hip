// The anchor encoder: SparseGaussian3DEncoder.forward (model/encoder/gaussian_encoder/anchor_encoder_module.py:38-53, with
// linear_relu_ln of utils.py:49-59) in one launch, and its training step (the saving forward: the same kernel with SAVE; the
// backward: further down).  The contract: include/gf_hip.h; the design and the measured numbers: DESIGN.md §3.13, §3.13b.
//
// The module is twelve Linear -> ReLU -> LayerNorm stages over 128 features: two per input branch (xyz, scale, rotation,
// opacity, semantics; the first of each has a thin K of 3, 3, 4, 1, S), the branches' sum, then two more.  torch runs it as
// about 40 kernels that each read and write an [A, 128] tensor; here a row's 128 features never leave the registers.
//
// Organisation.  A workgroup of four waves owns 128 anchors, a wave 32 of them.  Every product is Y^T = W X^T on
// v_mfma_f32_32x32x2_f32 (exact fp32 operands and accumulate): the accumulator's columns are the wave's 32 anchors, its rows
// features, and four accumulators hold all 128 features.  A lane therefore holds 64 features of ONE anchor (lane % 32), those
// with feature bit 2 == lane / 32:
//     feature(b, r, h) = 32 b + 8 (r >> 2) + 4 h + (r & 3)         b: accumulator, r: its register, h = lane / 32
// The MFMA sums over k in steps of two, lanes 0-31 supplying one k and lanes 32-63 the other, and WHICH two k a step takes is
// free as long as A and B agree.  Step (b, r) takes k = feature(b, r, 0) and feature(b, r, 1): exactly the two values that
// register r of accumulator b holds in the two halves of the wave.  So a stage's output registers ARE the next stage's B
// operands -- no transpose, no LDS round trip, no cross-lane move between stages.  Bias, ReLU and the LayerNorm sums are
// per-lane loops over the 64 registers; one exchange with lane ^ 32 completes each sum.
//
// The A operand is the weight in torch's own layout, W[out][in]: lane (f = lane % 32, h) needs W[32 fb + f][feature(b, r, h)],
// and r = 4 m .. 4 m + 3 are four consecutive floats of a row.  The workgroup stages W through LDS in chunks of 32 input
// columns (128 rows x 32 floats, row pitch 36 floats: the ds_read_b128 of 16 lanes then covers all 64 banks), double
// buffered: chunk g + 1 is fetched from L2 into registers before chunk g's 64 MFMAs and written to the other buffer after
// them, one barrier per chunk, across stage boundaries.  No weight is re-laid out in memory, so the op has no workspace.
//
// The thin first layers run on the same MFMA with K padded to even: a lane beyond the branch's K supplies 0 for both operands
// and never loads, so an anchor column that no branch reads cannot reach the result (0 x NaN would be NaN).
//
// Rows past n in the last tile compute on row n - 1 and are not stored.  The result leaves through LDS (the weight buffers,
// idle by then) so that a store instruction writes runs of 256 bytes.
#include "gf_rows_bwd.hpp"

namespace gf {

constexpr int kAeE = 128;        // features (embed_dims); every shipped config
constexpr int kAeMaxS = 32;      // semantic columns (gf_refine_*'s limit)
constexpr int kAeTile = kRowTile;   // anchors per workgroup, 32 per wave (gf_rows.hpp: the layout and the helpers on it)
constexpr int kAePitch4 = kRowPitch4;
constexpr int kAeVecs = 36;      // (5 thin + 7 square stages) x (bias, LayerNorm weight, LayerNorm bias), 128 floats each

struct AeThin { const float *w; int col0, k; };   // a branch's Linear(k -> 128): reads anchor columns col0 .. col0 + k
struct AnchorEmbedArgs {
    const float *anchor;
    float *out;
    AeThin thin[5];          // the nb branches present, in the reference's order
    const float *sq[7];      // the weights of their second layers, then of output_fc's two
    // Linear bias, LayerNorm weight, LayerNorm bias of every stage: thin stage q at 3 q, square stage q at 3 (5 + q)
    const float *vec[kAeVecs];
    int nb, n, Da;
};
// the saving forward (gf_anchor_embed_forward_train) adds: compact stage st = q (thin), nb + q (square) of 2 nb + 2
struct AnchorEmbedSaveArgs : AnchorEmbedArgs {
    float *rsave;            // [2 nb + 2][n][128] every stage's post-ReLU row
    float *stat;             // [2 nb + 2][n][2]   its LayerNorm's (mean, rstd)
    float *sumv;             // [n][128]           the branches' sum, output_fc's input
};
template <bool SAVE> struct AeFwdArgs { using type = AnchorEmbedArgs; };
template <> struct AeFwdArgs<true> { using type = AnchorEmbedSaveArgs; };

// acc <- W1 x^T for a thin first layer: step s takes k = 2 s (lanes 0-31) and 2 s + 1 (lanes 32-63)
__device__ __forceinline__ void thin_product(f32x16 (&acc)[4], const float *arow, const AeThin &t, int j, int h)
{
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    const int k = t.k;
    for (int s0 = 0; 2 * s0 < k; s0 += 8) {
        float bv[8], av[4][8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int kk = 2 * (s0 + s) + h;
            const bool live = kk < k;
            bv[s] = live ? arow[t.col0 + kk] : 0.f;
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) av[fb][s] = live ? t.w[(32 * fb + j) * k + kk] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (2 * (s0 + s) < k) {
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[fb][s], bv[s], acc[fb], 0, 0, 0);
            }
        }
    }
}

template <bool SAVE>
__global__ __launch_bounds__(256) void gf_anchor_embed_kernel(typename AeFwdArgs<SAVE>::type a)
{
    __shared__ float4 s_w[2][kAeE * kAePitch4];
    __shared__ float4 s_vec[kAeVecs * 32];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = blockIdx.x * kAeTile + wv * 32;
    const float *arow = a.anchor + (size_t)min(row0 + j, a.n - 1) * a.Da;
    const int nsq = a.nb + 2;
    // SAVE: where the lane's anchor keeps stage st's row and statistics (null past n: nothing is stored)
    const bool valid = row0 + j < a.n;
    auto rrow = [&](int st) -> float * {
        if constexpr (SAVE) return valid ? a.rsave + ((size_t)st * a.n + row0 + j) * kAeE : nullptr;
        else return nullptr;
    };
    auto st2 = [&](int st) -> float * {
        if constexpr (SAVE) return valid ? a.stat + ((size_t)st * a.n + row0 + j) * 2 : nullptr;
        else return nullptr;
    };

    float4 pre[4];
    auto fetch = [&](const float *w, int c) { chunk_fetch(pre, w, kAeE, 32 * c, t); };
    auto stash = [&](int buf) { chunk_stash(s_w[buf], pre, t); };

    f32x16 x[4], acc[4], sum[4];
    fetch(a.sq[0], 0);
    // every stage's bias and LayerNorm vectors into LDS once (18 KB): a wave takes every fourth vector, half a wave moves one.
    // All loads go out before the first is written (an absent stage's slot repeats vector 0 and is never read)
    {
        const int v0 = __builtin_amdgcn_readfirstlane(wv);
        float4 vec[kAeVecs / 4];
#pragma unroll
        for (int i = 0; i < kAeVecs / 4; ++i) {
            const float *src = a.vec[v0 + 4 * i] ? a.vec[v0 + 4 * i] : a.vec[0];
            vec[i] = ld4(src + 4 * j);
        }
#pragma unroll
        for (int i = 0; i < kAeVecs / 4; ++i)
            if (l < 32) s_vec[(v0 + 4 * i) * 32 + l] = vec[i];
        __syncthreads();
    }
    for (int q = 0; q < nsq; ++q) {
        if (q < a.nb) {
            thin_product(x, arow, a.thin[q], j, h);
            relu_ln<SAVE>(x, s_vec + 96 * q, h, rrow(q), st2(q));
        }
        if (q == 0) {
            stash(0);
            __syncthreads();
        }
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool more = c < 3 || q + 1 < nsq;
            if (more) fetch(c < 3 ? a.sq[q] : a.sq[q + 1], (c + 1) & 3);
            chunk_mfma(acc, x[c], s_w[c & 1], j, h);
            if (more) stash((c + 1) & 1);
            __syncthreads();
        }
        relu_ln<SAVE>(acc, s_vec + 96 * (5 + q), h, rrow(a.nb + q), st2(a.nb + q));
        if (q < a.nb) {   // the branches' sum, left to right (:51)
            if (q == 0) {
#pragma unroll
                for (int b = 0; b < 4; ++b) sum[b] = acc[b];
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b) sum[b] += acc[b];
            }
            if (q == a.nb - 1) {
#pragma unroll
                for (int b = 0; b < 4; ++b) x[b] = sum[b];
                if constexpr (SAVE) {
                    if (valid) store_row_regs(a.sumv + (size_t)(row0 + j) * kAeE, x, h);
                }
            }
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b) x[b] = acc[b];
        }
    }

    // x = the result, through the (idle) weight buffers
    store_rows(reinterpret_cast<float *>(&s_w[0][0]) + wv * (32 * kRowOutPitch), x, a.out, row0, a.n, l, j, h);
}

// ---- the backward (gf_anchor_embed_backward) ---------------------------------------------------------------
// Three kernels, no atomics.  (1) The data backward: the forward's tile and register layout, the stages in reverse.  A stage's
// LayerNorm + ReLU backward is per-lane loops and two lane ^ 32 exchanges; dX^T = W^T dZ^T runs on the same MFMA with the dz
// registers as the B operand as they stand (step (b, r) sums over o = feature(b, r, 0 / 1)) and W read along its rows, staged
// through LDS in chunks of 32 output rows.  It writes every stage's dz rows for (2), grad_anchor, and per tile the sums over
// its anchors of dz, dy n^ and dy (Linear bias, LayerNorm weight, LayerNorm bias).  (2) The weight gradients dW = dz^T x, a
// workgroup per (block of kAeWgRows rows, stage), x recomputed from the saved rows.  (3) One fixed-order sum of the partials of
// (1) and (2) into the caller's gradient tensors: stored, not accumulated.
constexpr int kAeMaxStages = 12;
constexpr int kAeWgRows = GF_ANCHOR_EMBED_WGRAD_ROWS;   // rows per workgroup of the weight-gradient kernel
// (1) and (2) run chunk by chunk of this many rows (512 tiles, two per CU), one after the other on the stream, so the dz rows
// -- as large per row as everything the forward saves -- are held for one chunk only; the partials are kept for all of them
constexpr int kAeChunkRows = GF_ANCHOR_EMBED_CHUNK_ROWS;
static_assert(kAeChunkRows % kAeWgRows == 0 && kAeWgRows % kAeTile == 0, "a chunk is whole weight-gradient blocks, a block whole tiles");

struct AeBwdArgs {
    const float *grad_out;
    float *grad_anchor;
    const float *rsave, *stat;
    float *dz;                    // [2 nb + 2][crows][128], the chunk's rows
    float *vpart;                 // [tiles][2 nb + 2][3][128], all chunks'
    const float *w[kAeMaxStages], *gam[kAeMaxStages];   // compact stage st: Linear weight, LayerNorm weight
    int k[5], col0[5];
    int nb, n, Da, used;
    int base, crows;              // the chunk: its first row, the rows a stage of dz holds
};

// g: dL/dy of the stage (the lane's 64 features of its anchor) -> dL/dz, the gradient before bias and ReLU:
//     n^ = (r - mean) rstd,  dn = dy gamma,  dr = rstd (dn - mean(dn) - n^ mean(dn n^)),  dz = r <= 0 ? 0 : dr
// (torch's threshold: a NaN r passes the gradient on).  part: the wave's [3][128] sums over its 32 anchors of dz, dy n^, dy,
// written by lanes 31 and 63 (sum32_last); rows past n add 0.
__device__ __forceinline__ void ln_relu_bwd(f32x16 (&g)[4], const float *rrow, float mean, float rstd, const float *gam, bool valid,
                                            float *part, int j, int h)
{
    f32x16 nh[4];
    uint32_t dead[4];
    float p1[4], p2[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float s1 = 0.f, s2 = 0.f;
        uint32_t dm = 0u;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int f0 = 32 * b + 8 * m + 4 * h;
            const float4 rr = ld4(rrow + f0), gg = ld4(gam + f0);
            const float rv[4] = {rr.x, rr.y, rr.z, rr.w}, gv[4] = {gg.x, gg.y, gg.z, gg.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * m + i;
                const float nhat = (rv[i] - mean) * rstd, dy = g[b][r];
                const float a1 = sum32_last(valid ? dy * nhat : 0.f), a2 = sum32_last(valid ? dy : 0.f);
                if (j == 31) {
                    part[kAeE + f0 + i] = a1;
                    part[2 * kAeE + f0 + i] = a2;
                }
                const float dn = dy * gv[i];
                s1 += dn;
                s2 += dn * nhat;
                g[b][r] = dn;
                nh[b][r] = nhat;
                dm |= (rv[i] <= 0.f ? 1u : 0u) << r;
            }
        }
        p1[b] = s1;
        p2[b] = s2;
        dead[b] = dm;
    }
    const float m1 = wave_xor_reduce_strided((p1[0] + p1[1]) + (p1[2] + p1[3]), 32, Sum()) * (1.f / kAeE);
    const float m2 = wave_xor_reduce_strided((p2[0] + p2[1]) + (p2[2] + p2[3]), 32, Sum()) * (1.f / kAeE);
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float dr = rstd * (g[b][r] - m1 - nh[b][r] * m2);
            const float dz = (dead[b] >> r) & 1u ? 0.f : dr;
            g[b][r] = dz;
            const float a0 = sum32_last(valid ? dz : 0.f);
            if (j == 31) part[32 * b + 8 * (r >> 2) + 4 * h + (r & 3)] = a0;
        }
}

// one stage's LayerNorm + ReLU backward on g, its dz row stored, the tile's three vector partials written
__device__ __forceinline__ void ae_stage_bwd(const AeBwdArgs &a, f32x16 (&g)[4], int st, int row, bool valid, float (*s_part)[3 * kAeE],
                                             int t, int wv, int j, int h)
{
    const size_t at = (size_t)st * a.n + row;
    const float2 ms = *reinterpret_cast<const float2 *>(a.stat + at * 2);
    ln_relu_bwd(g, a.rsave + at * kAeE, ms.x, ms.y, a.gam[st], valid, s_part[wv], j, h);
    if (valid) store_row_regs(a.dz + ((size_t)st * a.crows + (row - a.base)) * kAeE, g, h);
    __syncthreads();
    const int ns = 2 * a.nb + 2;
    for (int e = t; e < 3 * kAeE; e += 256)   // the four waves, in their order
        a.vpart[((size_t)(a.base / kAeTile + blockIdx.x) * ns + st) * (3 * kAeE) + e] = (s_part[0][e] + s_part[1][e]) + (s_part[2][e] + s_part[3][e]);
    __syncthreads();
}

// g <- W^T g for a square stage
__device__ __forceinline__ void ae_product_bwd(f32x16 (&g)[4], const float *w, float (*s_w)[32 * kRowTPitch], int t, int j, int h)
{
    f32x16 acc[4];
    zero_rows(acc);
    product_t<4, false>(acc, g, w, kAeE, 0, s_w[0], s_w[1], t, j, h);
#pragma unroll
    for (int b = 0; b < 4; ++b) g[b] = acc[b];
}

__global__ __launch_bounds__(256) void gf_anchor_embed_bwd_kernel(AeBwdArgs a)
{
    __shared__ float s_w[2][32 * kRowTPitch];
    __shared__ float s_part[4][3 * kAeE];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = a.base + blockIdx.x * kAeTile + wv * 32;
    const bool valid = row0 + j < a.n;
    const int row = min(row0 + j, a.n - 1);   // a row past n walks row n - 1 with a zero gradient and stores nothing
    const int nb = a.nb;

    f32x16 g[4], dsum[4];
    load_row_or_zero(g, a.grad_out + (size_t)row * kAeE, valid, h);
    // i = 0, 1: output_fc's second and first stage; then the branches, last to first: square stage, thin stage
    for (int i = 0; i < nb + 2; ++i) {
        const int q = nb + 1 - i, st = i < 2 ? 2 * nb + 1 - i : nb + q;
        if (i >= 2) {
#pragma unroll
            for (int b = 0; b < 4; ++b) g[b] = dsum[b];
        }
        ae_stage_bwd(a, g, st, row, valid, s_part, t, wv, j, h);
        ae_product_bwd(g, a.w[st], s_w, t, j, h);
        if (i == 1) {
#pragma unroll
            for (int b = 0; b < 4; ++b) dsum[b] = g[b];
        }
        if (i >= 2) {
            ae_stage_bwd(a, g, q, row, valid, s_part, t, wv, j, h);
            // grad_anchor[col0 + k] = sum_o W1[o][k] dz[o]: the lane's 64 features, then its partner's
            const int K = a.k[q];
            const float *w1 = a.w[q];
            for (int k = 0; k < K; ++k) {
                float s[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    s[b] = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[b] += g[b][r] * w1[(32 * b + 8 * (r >> 2) + 4 * h + (r & 3)) * K + k];
                }
                float p = (s[0] + s[1]) + (s[2] + s[3]);
                p += __shfl_xor(p, 32, 64);
                if (valid && h == 0) a.grad_anchor[(size_t)row * a.Da + a.col0[q] + k] = p;
            }
        }
    }
    if (valid && h == 0)
        for (int c = a.used; c < a.Da; ++c) a.grad_anchor[(size_t)row * a.Da + c] = 0.f;
}

struct AeWgArgs {
    const float *anchor, *rsave, *stat, *sumv, *dz;
    float *wsq;      // [blocks][nb + 2][128][128]
    float *wthin;    // [blocks][nb][128][32]
    const float *gam[kAeMaxStages], *bet[kAeMaxStages];
    int k[5], col0[5];
    int nb, n, Da;
    int base, crows;
};

// dW = dz^T x over one block of rows: A = dz[row][o] and B = x[row][k], two rows a step (lanes 0-31 one, lanes 32-63 the other),
// both loaded from the row-major arrays as they lie.  A wave owns 32 output rows o.  A lane beyond the rows or beyond a thin
// stage's K supplies 0 (a select, not a product) and loads what a live lane reads anyway: no unread column is touched.
__global__ __launch_bounds__(256) void gf_anchor_embed_wgrad_kernel(AeWgArgs a)
{
    const int st = blockIdx.y, blk = a.base / kAeWgRows + blockIdx.x;
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int r0 = blk * kAeWgRows, r1 = min(a.n, r0 + kAeWgRows), nb = a.nb;
    const float *dz = a.dz + (size_t)st * a.crows * kAeE + 32 * wv + j;   // + the row's place in the chunk
    if (st < nb) {
        const int K = a.k[st];
        const float *src = a.anchor + a.col0[st] + (j < K ? j : 0);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        // four steps' loads go out together.  A dead lane reads the block's last row, or the stage's first column, and supplies 0
        for (int r = r0; r < r1; r += 8) {
            float av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int row = min(r + 2 * u + h, r1 - 1);
                av[u] = dz[(size_t)(row - a.base) * kAeE];
                bv[u] = src[(size_t)row * a.Da];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool live = r + 2 * u + h < r1;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(live ? av[u] : 0.f, live && j < K ? bv[u] : 0.f, acc, 0, 0, 0);
            }
        }
        float *dst = a.wthin + ((size_t)blk * nb + st) * (kAeE * 32) + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(32 * wv + 8 * (r >> 2) + 4 * h + (r & 3)) * 32] = acc[r];
        return;
    }
    // x = LayerNorm(r of the stage before) recomputed as the forward applies it; output_fc's first stage reads the saved sum
    const int q = st - nb, ps = q < nb ? q : 2 * nb;
    const bool plain = q == nb;
    const float *src = (plain ? a.sumv : a.rsave + (size_t)ps * a.n * kAeE) + j;
    const float *stat = a.stat + (size_t)ps * a.n * 2;
    float gv[4], ev[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        gv[cb] = plain ? 1.f : a.gam[ps][32 * cb + j];
        ev[cb] = plain ? 0.f : a.bet[ps][32 * cb + j];
    }
    f32x16 acc[4];
    zero_rows(acc);
    if (plain) wgrad_rows<kWgAsIs>(acc, dz, kAeE, a.base, src, nullptr, kAeE, 0, nullptr, gv, ev, r0, r1, r1, h);
    else wgrad_rows<kWgNorm>(acc, dz, kAeE, a.base, src, nullptr, kAeE, 0, stat, gv, ev, r0, r1, r1, h);
    wgrad_store(a.wsq + ((size_t)blk * (nb + 2) + q) * (kAeE * kAeE), kAeE, [&](int cb, int r) { return acc[cb][r]; }, wv, j, h);
}

// (3) is rows_sum_kernel<float>; K > 0 there: a thin weight [128][K], whose partials are rows of 32.  Instantiated here and not
// by the launch alone: a template's kernel is otherwise emitted behind the forward kernels, whose local labels are numbered by
// their place in the code object -- with this line their assembly is the earlier one line for line, labels included
template __global__ void rows_sum_kernel<float, GF_ANCHOR_EMBED_PARAMS>(RowsSumArgs<GF_ANCHOR_EMBED_PARAMS>);

// ---- host ---------------------------------------------------------------------------------------------------------------------

// the shape checks and the 48-pointer table -> the kernels' compact form, reported under the entry point's name
static int ae_parse(const char *fn, int n, int Da, int E, int opa, int S, const void *const *params, AnchorEmbedArgs &a)
{
    GF_CHECK_ARG_AS(fn, n >= 0, "negative n");
    GF_CHECK_ARG_AS(fn, E == kAeE, "only embed_dims = 128 is supported");
    GF_CHECK_ARG_AS(fn, S >= 0 && S <= kAeMaxS, "S must be in 0 .. 32");
    GF_CHECK_ARG_AS(fn, Da >= 10 + opa + S, "Da is smaller than 10 + opacity + S");
    GF_CHECK_ARG_AS(fn, params, "null params");
    const int col0[5] = {0, 3, 6, 10, 10 + opa}, k[5] = {3, 3, 4, opa, S};
    for (int s = 0; s < 6; ++s) {
        const float *const *p = reinterpret_cast<const float *const *>(params) + 8 * s;
        const bool present = s == 5 || k[s] > 0;
        for (int i = 0; i < 8; ++i) {
            GF_CHECK_ARG_AS(fn, !present || p[i], "null parameter of a stage that is present");
            GF_CHECK_ARG_AS(fn, !present || i == 0 || !misaligned16(p[i]), "a parameter is not 16-byte aligned");
        }
        if (!present) continue;
        if (s < 5) {
            a.thin[a.nb] = AeThin{p[0], col0[s], k[s]};
            a.sq[a.nb] = p[4];
            for (int i = 0; i < 3; ++i) {
                a.vec[3 * a.nb + i] = p[1 + i];
                a.vec[3 * (5 + a.nb) + i] = p[5 + i];
            }
            ++a.nb;
        } else {
            GF_CHECK_ARG_AS(fn, !misaligned16(p[0]), "a parameter is not 16-byte aligned");
            a.sq[a.nb] = p[0];
            a.sq[a.nb + 1] = p[4];
            for (int i = 0; i < 3; ++i) {
                a.vec[3 * (5 + a.nb) + i] = p[1 + i];
                a.vec[3 * (6 + a.nb) + i] = p[5 + i];
            }
        }
    }
    a.n = n; a.Da = Da;
    return GF_OK;
}

// The training step's two regions, sized and carved by one function each (a null base: sizes only).
struct AeSaved { float *rsave, *stat, *sumv; size_t bytes; };
static AeSaved ae_carve_saved(void *base, int n, int nb)
{
    Carver c(base);
    AeSaved s;
    s.rsave = c.take<float>((size_t)(2 * nb + 2) * n * kAeE);
    s.stat = c.take<float>((size_t)(2 * nb + 2) * n * 2);
    s.sumv = c.take<float>((size_t)n * kAeE);
    s.bytes = c.bytes();
    return s;
}
struct AeWork { float *dz, *vpart, *wsq, *wthin; int tiles, blocks, crows; size_t bytes; };
static AeWork ae_carve_work(void *base, int n, int nb)
{
    Carver c(base);
    AeWork w;
    w.tiles = (n + kAeTile - 1) / kAeTile;
    w.blocks = (n + kAeWgRows - 1) / kAeWgRows;
    w.crows = n < kAeChunkRows ? n : kAeChunkRows;
    w.dz = c.take<float>((size_t)(2 * nb + 2) * w.crows * kAeE);
    w.vpart = c.take<float>((size_t)w.tiles * (2 * nb + 2) * 3 * kAeE);
    w.wsq = c.take<float>((size_t)w.blocks * (nb + 2) * kAeE * kAeE);
    w.wthin = c.take<float>((size_t)w.blocks * nb * kAeE * 32);
    w.bytes = c.bytes();
    return w;
}

}  // namespace gf

extern "C" int gf_anchor_embed_forward(int n, int Da, int E, int include_opa, int S, const float *anchor, const void *const *params,
                                       float *out, void *stream_)
{
    using namespace gf;
    AnchorEmbedArgs a{};
    if (int rc = ae_parse(__func__, n, Da, E, include_opa ? 1 : 0, S, params, a)) return rc;
    if (n == 0) return GF_OK;
    GF_CHECK_ARG(anchor && out, "null pointer");
    GF_CHECK_ARG(!misaligned16(out), "out is not 16-byte aligned");
    a.anchor = anchor; a.out = out;
    hipLaunchKernelGGL(gf_anchor_embed_kernel<false>, dim3((n + kAeTile - 1) / kAeTile), dim3(256), 0, (hipStream_t)stream_, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_anchor_embed_train_sizes(int n, int include_opa, int S, size_t *saved_bytes, size_t *workspace_bytes)
{
    using namespace gf;
    GF_CHECK_ARG(n >= 0, "negative n");
    GF_CHECK_ARG(S >= 0 && S <= kAeMaxS, "S must be in 0 .. 32");
    GF_CHECK_ARG(saved_bytes && workspace_bytes, "null pointer");
    const int nb = 3 + (include_opa ? 1 : 0) + (S > 0 ? 1 : 0);
    *saved_bytes = ae_carve_saved(nullptr, n, nb).bytes;
    *workspace_bytes = ae_carve_work(nullptr, n, nb).bytes;
    return GF_OK;
}

extern "C" int gf_anchor_embed_forward_train(int n, int Da, int E, int include_opa, int S, const float *anchor, const void *const *params,
                                             float *out, void *saved, size_t saved_bytes, void *stream_)
{
    using namespace gf;
    AnchorEmbedSaveArgs a{};
    if (int rc = ae_parse(__func__, n, Da, E, include_opa ? 1 : 0, S, params, a)) return rc;
    if (n == 0) return GF_OK;
    GF_CHECK_ARG(anchor && out && saved, "null pointer");
    GF_CHECK_ARG(!misaligned16(out), "out is not 16-byte aligned");
    GF_CHECK_ARG(!misaligned16(saved), "saved is not 16-byte aligned");
    const AeSaved sv = ae_carve_saved(saved, n, a.nb);
    GF_CHECK_WORKSPACE_AS(__func__, "saved", saved_bytes, sv.bytes);
    a.anchor = anchor; a.out = out;
    a.rsave = sv.rsave; a.stat = sv.stat; a.sumv = sv.sumv;
    hipLaunchKernelGGL(gf_anchor_embed_kernel<true>, dim3((n + kAeTile - 1) / kAeTile), dim3(256), 0, (hipStream_t)stream_, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_anchor_embed_backward(int n, int Da, int E, int include_opa, int S, const float *anchor, const void *const *params,
                                        const void *saved, const float *grad_out, float *grad_anchor, void *const *grad_params,
                                        void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace gf;
    const int opa = include_opa ? 1 : 0;
    AnchorEmbedArgs f{};
    if (int rc = ae_parse(__func__, n, Da, E, opa, S, params, f)) return rc;
    GF_CHECK_ARG(grad_params, "null grad_params");
    const int nb = f.nb, ns = 2 * nb + 2;
    // the gradient tensors in the compact order: weight and (Linear bias, LayerNorm weight, LayerNorm bias) of stage st
    float *gw[kAeMaxStages], *gvec[kAeMaxStages][3];
    {
        const int k[5] = {3, 3, 4, opa, S};
        int q = 0;
        for (int s = 0; s < 6; ++s) {
            if (s < 5 && k[s] == 0) continue;
            float *const *p = reinterpret_cast<float *const *>(grad_params) + 8 * s;
            for (int i = 0; i < 8; ++i) GF_CHECK_ARG(p[i], "null gradient of a stage that is present");
            const int st1 = s < 5 ? q : 2 * nb, st2 = s < 5 ? nb + q : 2 * nb + 1;
            gw[st1] = p[0]; gw[st2] = p[4];
            for (int i = 0; i < 3; ++i) { gvec[st1][i] = p[1 + i]; gvec[st2][i] = p[5 + i]; }
            q += s < 5;
        }
    }
    const AeSaved sv = ae_carve_saved(n > 0 ? const_cast<void *>(saved) : nullptr, n, nb);
    const AeWork ws = ae_carve_work(n > 0 ? workspace : nullptr, n, nb);
    if (n > 0) {
        GF_CHECK_ARG(anchor && saved && grad_out && grad_anchor && workspace, "null pointer");
        GF_CHECK_ARG(!misaligned16(grad_out), "grad_out is not 16-byte aligned");
        GF_CHECK_ARG(!misaligned16(saved), "saved is not 16-byte aligned");
        GF_CHECK_ARG(!misaligned16(workspace), "workspace is not 16-byte aligned");
        GF_CHECK_WORKSPACE(workspace_bytes, ws.bytes);
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (n > 0) {
        AeBwdArgs b{};
        b.grad_out = grad_out; b.grad_anchor = grad_anchor;
        b.rsave = sv.rsave; b.stat = sv.stat; b.dz = ws.dz; b.vpart = ws.vpart;
        AeWgArgs g{};
        g.anchor = anchor; g.rsave = sv.rsave; g.stat = sv.stat; g.sumv = sv.sumv; g.dz = ws.dz; g.wsq = ws.wsq; g.wthin = ws.wthin;
        for (int q = 0; q < nb; ++q) {
            b.w[q] = f.thin[q].w; b.gam[q] = f.vec[3 * q + 1];
            b.k[q] = g.k[q] = f.thin[q].k; b.col0[q] = g.col0[q] = f.thin[q].col0;
            g.gam[q] = f.vec[3 * q + 1]; g.bet[q] = f.vec[3 * q + 2];
        }
        for (int q = 0; q < nb + 2; ++q) {
            b.w[nb + q] = f.sq[q]; b.gam[nb + q] = f.vec[3 * (5 + q) + 1];
            g.gam[nb + q] = f.vec[3 * (5 + q) + 1]; g.bet[nb + q] = f.vec[3 * (5 + q) + 2];
        }
        b.nb = g.nb = nb; b.n = g.n = n; b.Da = g.Da = Da; b.used = 10 + opa + S;
        b.crows = g.crows = ws.crows;
        for (int base = 0; base < n; base += kAeChunkRows) {   // the next chunk's data backward overwrites dz behind this one's wgrad
            const int rows = n - base < kAeChunkRows ? n - base : kAeChunkRows;
            b.base = g.base = base;
            hipLaunchKernelGGL(gf_anchor_embed_bwd_kernel, dim3((rows + kAeTile - 1) / kAeTile), dim3(256), 0, stream, b);
            GF_CHECK_LAUNCH();
            hipLaunchKernelGGL(gf_anchor_embed_wgrad_kernel, dim3((rows + kAeWgRows - 1) / kAeWgRows, ns), dim3(256), 0, stream, g);
            GF_CHECK_LAUNCH();
        }
    }
    // n == 0: no partials, the sums store zeros
    RowsSumArgs<GF_ANCHOR_EMBED_PARAMS> sa{};   // float sums, a thread per element; K > 0: a thin weight, its partials rows of 32
    int nj = 0;
    for (int st = 0; st < ns; ++st) {
        const bool thin = st < nb;
        const int K = thin ? f.thin[st].k : 0;
        const float *wsrc = n == 0 ? nullptr : thin ? ws.wthin + (size_t)st * kAeE * 32 : ws.wsq + (size_t)(st - nb) * kAeE * kAeE;
        sa.job[nj++] = thin ? RowsSumJob{wsrc, gw[st], (size_t)nb * kAeE * 32, n > 0 ? ws.blocks : 0, kAeE * K, K, 1}
                            : RowsSumJob{wsrc, gw[st], (size_t)(nb + 2) * kAeE * kAeE, n > 0 ? ws.blocks : 0, kAeE * kAeE, 0, 1};
        for (int v = 0; v < 3; ++v)
            sa.job[nj++] = RowsSumJob{n == 0 ? nullptr : ws.vpart + ((size_t)st * 3 + v) * kAeE, gvec[st][v], (size_t)ns * 3 * kAeE, n > 0 ? ws.tiles : 0, kAeE, 0, 1};
    }
    hipLaunchKernelGGL((rows_sum_kernel<float, GF_ANCHOR_EMBED_PARAMS>), dim3(kAeE * kAeE / 256, nj), dim3(256), 0, stream, sa);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
