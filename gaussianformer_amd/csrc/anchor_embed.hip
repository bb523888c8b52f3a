// The anchor encoder: SparseGaussian3DEncoder.forward (model/encoder/gaussian_encoder/anchor_encoder_module.py:38-53, with
// linear_relu_ln of utils.py:49-59) in one launch.  The contract: include/gf_hip.h; the design and the measured numbers:
// DESIGN.md §3.13.
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
#include "gf_common.hpp"

namespace gf {

constexpr int kAeE = 128;        // features (embed_dims); every shipped config
constexpr int kAeMaxS = 32;      // semantic columns (gf_refine_*'s limit)
constexpr int kAeTile = 128;     // anchors per workgroup, 32 per wave
constexpr int kAePitch4 = 9;     // float4 per staged weight row: 32 floats + 4 of padding
constexpr int kAeOutPitch = 68;  // floats per row of the output staging tile: 64 features + 4 of padding
constexpr float kAeLnEps = 1e-5f;
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

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

// v <- LayerNorm(relu(v + bias)) over the 128 features of the lane's anchor (biased variance, two passes); p: the stage's
// three vectors in LDS (32 float4 each: bias, LayerNorm weight, LayerNorm bias)
__device__ __forceinline__ void relu_ln(f32x16 (&v)[4], const float4 *p, int h)
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
        }
        part[b] = s;
    }
    const float mean = wave_xor_reduce_strided((part[0] + part[1]) + (part[2] + part[3]), 32, Sum()) * (1.f / kAeE);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float d = v[b][r] - mean;
            v[b][r] = d;
            s += d * d;
        }
        part[b] = s;
    }
    const float var = wave_xor_reduce_strided((part[0] + part[1]) + (part[2] + part[3]), 32, Sum()) * (1.f / kAeE);
    const float rstd = 1.f / sqrtf(var + kAeLnEps);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 gg = p[32 + 8 * b + 2 * m + h], ee = p[64 + 8 * b + 2 * m + h];
            const float gv[4] = {gg.x, gg.y, gg.z, gg.w}, ev[4] = {ee.x, ee.y, ee.z, ee.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) v[b][4 * m + i] = v[b][4 * m + i] * rstd * gv[i] + ev[i];
        }
    }
}

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

__global__ __launch_bounds__(256) void gf_anchor_embed_kernel(AnchorEmbedArgs a)
{
    __shared__ float4 s_w[2][kAeE * kAePitch4];
    __shared__ float4 s_vec[kAeVecs * 32];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = blockIdx.x * kAeTile + wv * 32;
    const float *arow = a.anchor + (size_t)min(row0 + j, a.n - 1) * a.Da;
    const int nsq = a.nb + 2;

    // staging of a weight chunk: thread -> rows ff + 32 i, float4 fq of the chunk's 8
    const int ff = t >> 3, fq = t & 7;
    float4 pre[4];
    auto fetch = [&](const float *w, int c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[i] = ld4(w + (size_t)(ff + 32 * i) * kAeE + 32 * c + 4 * fq);
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s_w[buf][(ff + 32 * i) * kAePitch4 + fq] = pre[i];
    };

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
            relu_ln(x, s_vec + 96 * q, h);
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
#pragma unroll
            for (int m = 0; m < 4; ++m) {
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const float4 w4 = s_w[c & 1][(32 * fb + j) * kAePitch4 + 2 * m + h];
                    acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w4.x, x[c][4 * m + 0], acc[fb], 0, 0, 0);
                    acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w4.y, x[c][4 * m + 1], acc[fb], 0, 0, 0);
                    acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w4.z, x[c][4 * m + 2], acc[fb], 0, 0, 0);
                    acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w4.w, x[c][4 * m + 3], acc[fb], 0, 0, 0);
                }
            }
            if (more) stash((c + 1) & 1);
            __syncthreads();
        }
        relu_ln(acc, s_vec + 96 * (5 + q), h);
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
            }
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b) x[b] = acc[b];
        }
    }

    // x = the result.  Through the (idle) weight buffers, 64 features at a time: the lane writes its anchor's float4s, the wave
    // reads four rows per instruction back and stores them
    float *so = reinterpret_cast<float *>(&s_w[0][0]) + wv * (32 * kAeOutPitch);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const f32x16 &v = x[2 * half + bb];
                *reinterpret_cast<float4 *>(so + j * kAeOutPitch + 32 * bb + 8 * m + 4 * h) =
                    make_float4(v[4 * m], v[4 * m + 1], v[4 * m + 2], v[4 * m + 3]);
            }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = 4 * i + (l >> 4), col = 4 * (l & 15);
            const float4 v = *reinterpret_cast<const float4 *>(so + r * kAeOutPitch + col);
            if (row0 + r < a.n) *reinterpret_cast<float4 *>(a.out + (size_t)(row0 + r) * kAeE + 64 * half + col) = v;
        }
        __syncthreads();
    }
}
static_assert(4 * 32 * kAeOutPitch <= 2 * kAeE * kAePitch4 * 4, "the output staging tiles fit the weight buffers");

}  // namespace gf

extern "C" int gf_anchor_embed_forward(int n, int Da, int E, int include_opa, int S, const float *anchor, const void *const *params,
                                       float *out, void *stream_)
{
    using namespace gf;
    const int opa = include_opa ? 1 : 0;
    GF_CHECK_ARG(n >= 0, "negative n");
    GF_CHECK_ARG(E == kAeE, "only embed_dims = 128 is supported");
    GF_CHECK_ARG(S >= 0 && S <= kAeMaxS, "S must be in 0 .. 32");
    GF_CHECK_ARG(Da >= 10 + opa + S, "Da is smaller than 10 + opacity + S");
    GF_CHECK_ARG(params, "null params");
    AnchorEmbedArgs a{};
    const int col0[5] = {0, 3, 6, 10, 10 + opa}, k[5] = {3, 3, 4, opa, S};
    for (int s = 0; s < 6; ++s) {
        const float *const *p = reinterpret_cast<const float *const *>(params) + 8 * s;
        const bool present = s == 5 || k[s] > 0;
        for (int i = 0; i < 8; ++i) {
            GF_CHECK_ARG(!present || p[i], "null parameter of a stage that is present");
            GF_CHECK_ARG(!present || i == 0 || (reinterpret_cast<uintptr_t>(p[i]) & 15) == 0, "a parameter is not 16-byte aligned");
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
            GF_CHECK_ARG((reinterpret_cast<uintptr_t>(p[0]) & 15) == 0, "a parameter is not 16-byte aligned");
            a.sq[a.nb] = p[0];
            a.sq[a.nb + 1] = p[4];
            for (int i = 0; i < 3; ++i) {
                a.vec[3 * (5 + a.nb) + i] = p[1 + i];
                a.vec[3 * (6 + a.nb) + i] = p[5 + i];
            }
        }
    }
    if (n == 0) return GF_OK;
    GF_CHECK_ARG(anchor && out, "null pointer");
    GF_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 15) == 0, "out is not 16-byte aligned");
    a.anchor = anchor; a.out = out; a.n = n; a.Da = Da;
    hipLaunchKernelGGL(gf_anchor_embed_kernel, dim3((n + kAeTile - 1) / kAeTile), dim3(256), 0, (hipStream_t)stream_, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
