// gf_ffn.hpp -- what the feed-forward block's two translation units share (ffn.hip: the plain forward; ffn_train.hip: the
// training step): the 128-row tile kernel with its TRAIN build, the keep-mask helpers and the argument
// checks of every launching entry point.  The plain forward stays a translation unit of its own so that its kernels are
// compiled exactly as before the training step existed (the same instruction streams).
#pragma once
#include "gf_rows.hpp"

namespace gf {

constexpr int kFfnE = GF_FFN_EMBED_DIMS, kFfnF = GF_FFN_HIDDEN;
static_assert(kFfnE == 128 && kFfnF % 128 == 0, "the output is one block of gf_rows.hpp, the hidden row whole slices of it");
constexpr int kFfnSlices = kFfnF / 128;

struct FfnArgs {
    const float *x, *residual;
    float *out;
    const float *pre_g, *pre_b, *w1, *b1, *w2, *b2, *wid, *bid, *post_g, *post_b;
    int n;
};
// the saving forward (gf_ffn_forward_train) adds the two keep masks with their scales and where the backward's rows go
struct FfnTrainArgs : FfnArgs {
    const unsigned char *keep_hidden, *keep_out;   // u8 [n, 512], [n, 128]; null: no dropout
    float scale_hidden, scale_out;
    float *ysave;                                  // [n][128] the row before the post norm (written when there is one)
    float *stat_pre, *stat_post;                   // [n][2]   the two norms' (mean, rstd)
};
template <bool TRAIN> struct FfnFwdArgs { using type = FfnArgs; };
template <> struct FfnFwdArgs<true> { using type = FfnTrainArgs; };

// The lane's 64 keep bits of a row's block of 128 mask bytes at p (any alignment): bit 16 b + r <- byte feature(b, r, h) != 0
__device__ __forceinline__ uint64_t keep_bits(const unsigned char *p, int h)
{
    uint64_t bits = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            uint32_t w;
            __builtin_memcpy(&w, p + 32 * b + 8 * m + 4 * h, 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) bits |= (uint64_t)(((w >> (8 * i)) & 0xffu) != 0u) << (16 * b + 4 * m + i);
        }
    return bits;
}
// v <- v * (kept ? scale : 0): a product, as nn.Dropout's, so that a NaN stays a NaN under a dropped entry too
__device__ __forceinline__ void drop_rows(f32x16 (&v)[4], uint64_t bits, float scale)
{
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) v[b][r] *= (bits >> (16 * b + r)) & 1u ? scale : 0.f;
}

// TRAIN: the same instruction chain per output element (out is bitwise the plain kernel's without masks, and with all-ones
// masks at scale 1), plus the dropouts and the stores of what gf_ffn_bwd_kernel reads
template <int CIN, bool TRAIN>
__global__ __launch_bounds__(256) void gf_ffn_kernel(typename FfnFwdArgs<TRAIN>::type a)
{
    constexpr int NB = CIN / 32;            // register blocks of u = chunks of a product over u
    constexpr int PER = NB + 4;             // chunks per hidden slice: W1's, then W2's
    static_assert(NB % 2 == 0, "a slice's chunks start on LDS buffer 0");
    // LDS vectors, in float4: LN_pre weight, bias | b1 | b2 | bid | LN_post weight, bias
    constexpr int vPre = 0, vB1 = 2 * CIN / 4, vB2 = vB1 + kFfnF / 4, vBid = vB2 + 32, vPost = vBid + 32, vEnd = vPost + 64;
    __shared__ float4 s_w[2][128 * kRowPitch4];
    __shared__ float4 s_vec[vEnd];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = blockIdx.x * kRowTile + wv * 32;
    const size_t row = (size_t)min(row0 + j, a.n - 1);
    const int G = kFfnSlices * PER + (a.wid ? NB : 0);
    [[maybe_unused]] const bool valid = row0 + j < a.n;   // TRAIN: rows past n save nothing

    float4 pre[4];
    auto fetch = [&](int g) {     // chunk g of the walk (g is uniform)
        const int s = g / PER, c = g - s * PER;
        if (s == kFfnSlices) chunk_fetch(pre, a.wid, CIN, 32 * c, t);
        else if (c < NB) chunk_fetch(pre, a.w1 + (size_t)(128 * s) * CIN, CIN, 32 * c, t);
        else chunk_fetch(pre, a.w2, kFfnF, 128 * s + 32 * (c - NB), t);
    };
    // one chunk: the next one is fetched before this one's 64 MFMAs and written to the other buffer after them
    auto step = [&](f32x16 (&acc)[4], const f32x16 &xb, int g, int buf) {
        const bool more = g + 1 < G;
        if (more) fetch(g + 1);
        chunk_mfma(acc, xb, s_w[buf], j, h);
        if (more) chunk_stash(s_w[buf ^ 1], pre, t);
        __syncthreads();
    };

    fetch(0);
    {
        auto put = [&](int at, const float *src, int count4) {
            if (src)
                for (int e = t; e < count4; e += 256) s_vec[at + e] = ld4(src + 4 * e);
        };
        put(vPre, a.pre_g, CIN / 4);
        put(vPre + CIN / 4, a.pre_b, CIN / 4);
        put(vB1, a.b1, kFfnF / 4);
        put(vB2, a.b2, 32);
        put(vBid, a.bid, 32);
        put(vPost, a.post_g, 32);
        put(vPost + 32, a.post_b, 32);
    }
    f32x16 u[NB];
    {   // (not load_row: with it the plain kernel comes out with another instruction order)
        const float *xrow = a.x + row * CIN;
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float4 v = ld4(xrow + 32 * b + 8 * m + 4 * h);
                u[b][4 * m] = v.x; u[b][4 * m + 1] = v.y; u[b][4 * m + 2] = v.z; u[b][4 * m + 3] = v.w;
            }
    }
    chunk_stash(s_w[0], pre, t);
    __syncthreads();
    if (a.pre_g) {
        float part[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) s += u[b][r];
            part[b] = s;
        }
        float *st2 = nullptr;
        if constexpr (TRAIN) st2 = valid ? a.stat_pre + 2 * row : nullptr;
        ln_rows<true, NB>(u, tree_sum<NB>(part), s_vec + vPre, s_vec + vPre + CIN / 4, h, st2);
    }

    f32x16 hid[4], y[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) y[b][r] = 0.f;
    int g = 0;
#pragma unroll 1
    for (int s = 0; s < kFfnSlices; ++s) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) hid[b][r] = 0.f;
        [[maybe_unused]] uint64_t kh = 0;
        if constexpr (TRAIN) {
            if (a.keep_hidden) kh = keep_bits(a.keep_hidden + row * kFfnF + 128 * s, h);
        }
#pragma unroll
        for (int c = 0; c < NB; ++c) step(hid, u[c], g++, c & 1);
        const float4 *b1 = s_vec + vB1 + 32 * s;
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float4 bb = b1[8 * b + 2 * m + h];
                const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = hid[b][4 * m + i] + bv[i];
                    hid[b][4 * m + i] = v < 0.f ? 0.f : v;     // (not fmaxf: a NaN stays a NaN, as torch's relu keeps it)
                }
            }
        if constexpr (TRAIN) {
            if (a.keep_hidden) drop_rows(hid, kh, a.scale_hidden);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) step(y, hid[c], g++, c & 1);
    }
    // TRAIN, the output dropout: W2 h' is masked and scaled here, before the identity product adds into the same accumulators,
    // and b2 gets the same factor below -- (W2 h' + b2) dropped as a whole, in the plain kernel's order of additions
    [[maybe_unused]] uint64_t ko = 0;
    if constexpr (TRAIN) {
        if (a.keep_out) {
            ko = keep_bits(a.keep_out + row * kFfnE, h);
            drop_rows(y, ko, a.scale_out);
        }
    }
    if (a.wid) {
#pragma unroll
        for (int c = 0; c < NB; ++c) step(y, u[c], g++, c & 1);
    }

    // y + b2 (+ bid) (+ residual), the lane's sum of it for LN_post
    const float *rrow = a.residual ? a.residual + row * kFfnE : nullptr;
    float part[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 bb = s_vec[vB2 + 8 * b + 2 * m + h];
            float add[4] = {bb.x, bb.y, bb.z, bb.w};
            if constexpr (TRAIN) {
                if (a.keep_out) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) add[i] *= (ko >> (16 * b + 4 * m + i)) & 1u ? a.scale_out : 0.f;
                }
            }
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = y[b][4 * m + i] + add[i];
            if (a.wid) {
                const float4 ii = s_vec[vBid + 8 * b + 2 * m + h];
                v[0] += ii.x; v[1] += ii.y; v[2] += ii.z; v[3] += ii.w;
            }
            if (a.residual) {   // last, so that a residual of zeros changes nothing
                const float4 rr = ld4(rrow + 32 * b + 8 * m + 4 * h);
                v[0] += rr.x; v[1] += rr.y; v[2] += rr.z; v[3] += rr.w;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                y[b][4 * m + i] = v[i];
                s += v[i];
            }
        }
        part[b] = s;
    }
    if (a.post_g) {
        float *st2 = nullptr;
        if constexpr (TRAIN) {
            if (valid) {
                st2 = a.stat_post + 2 * row;
                store_row_regs(a.ysave + row * kFfnE, y, h);
            }
        }
        ln_rows<true, 4>(y, tree_sum<4>(part), s_vec + vPost, s_vec + vPost + 32, h, st2);
    }
    // through the (idle) weight buffers: the last chunk's barrier is behind every wave's reads of them
    store_rows(reinterpret_cast<float *>(&s_w[0][0]) + wv * (32 * kRowOutPitch), y, a.out, row0, a.n, l, j, h);
}


inline constexpr const char *kFfnName[GF_FFN_PARAMS] = {"pre_norm.weight", "pre_norm.bias", "layers.0.0.weight", "layers.0.0.bias", "layers.1.weight",
                                                    "layers.1.bias", "identity_fc.weight", "identity_fc.bias", "norm.weight", "norm.bias"};

// what all three launching entry points refuse, in gf_ffn_forward's order and words, under the name of the one that was called
inline int ffn_check(const char *fn, int n, int Cin, int F, int E, const float *x, const void *const *params, const float *residual,
                     const float *out)
{
    GF_REFUSE_AS(fn, E == kFfnE, "E = %d: only embed_dims = 128 is supported", E);
    GF_REFUSE_AS(fn, F == kFfnF, "F = %d: only feedforward_channels = 512 is supported", F);
    GF_REFUSE_AS(fn, Cin == 128 || Cin == 256, "Cin = %d: only in_channels = 128 or 256 is supported", Cin);
    GF_REFUSE_AS(fn, n >= 0, "n = %d is negative", n);
    GF_REFUSE_AS(fn, params, "null params");
    const float *const *p = reinterpret_cast<const float *const *>(params);
    for (int i = 0; i < GF_FFN_PARAMS; i += 2) {
        if (i == 2 || i == 4) {
            GF_REFUSE_AS(fn, p[i], "%s is missing", kFfnName[i]);
            GF_REFUSE_AS(fn, p[i + 1], "%s is missing", kFfnName[i + 1]);
        }
        GF_REFUSE_AS(fn, !p[i] == !p[i + 1], "a half-present pair: %s is null and %s is not", kFfnName[p[i] ? i + 1 : i], kFfnName[p[i] ? i : i + 1]);
        for (int k = i; k < i + 2; ++k) GF_REFUSE_AS(fn, !misaligned16(p[k]), "%s is not 16-byte aligned", kFfnName[k]);
    }
    GF_REFUSE_AS(fn, !misaligned16(x), "x is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(residual), "residual is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(out), "out is not 16-byte aligned");
    return GF_OK;
}
}  // namespace gf
