// The encoder's feed-forward block: AsymmetricFFN.forward (model/encoder/gaussian_encoder/ffn_module.py:66-75) and the
// "add" / "norm" that follow it in the encoder's operation_order, in one launch.  The contract: include/gf_hip.h; the design
// and the measured numbers: DESIGN.md §3.13c.
//
//     u   = LN_pre(x)                       (optional)            x [n, Cin], Cin = 128 or 256
//     y   = W2 relu(W1 u + b1) + b2                               W1 [512, Cin], W2 [128, 512]
//     y  += Wid u + bid                     (optional)            Wid [128, Cin]
//     y  += residual                        (optional)            residual [n, 128]
//     out = LN_post(y)                      (optional)            out [n, 128]
//
// torch runs this as two LayerNorms, three GEMMs, a ReLU and an add, writing and re-reading an [n, 512] hidden tensor; here a
// row's 512 hidden values never exist at once, let alone in memory.
//
// Organisation: gf_rows.hpp's (the anchor encoder's).  A wave owns 32 rows; u is Cin / 32 register blocks per lane (128
// registers for Cin = 256) and stays for the whole kernel.  The hidden row is walked in four slices of 128: slice s of
// relu(W1 u + b1) is produced into four accumulators (Cin / 32 weight chunks of W1's rows 128 s ..), gets its bias and ReLU
// in place, and is at once the B operand of W2[:, 128 s ..]'s four chunks, which add into the four output accumulators.  The
// identity product Wid u adds into the same accumulators last.  Every weight chunk (128 rows x 32 columns of a matrix where
// the module keeps it) goes through the double-buffered LDS staging, one barrier per chunk, across all stage boundaries:
// 4 (Cin / 32 + 4) + Cin / 32 chunks, 56 for the base family.  Biases and LayerNorm vectors are put into LDS once.
//
// ReLU is x < 0 ? 0 : x (a NaN stays).  Rows past n compute on row n - 1 and are not stored.  No workspace, no atomics: a
// row's result depends on nothing but the row and the parameters.
//
// Few rows (gf_ffn_rows32_kernel).  A tile is one wave's serial walk of all chunks, about 130 us, whether 1 or 256 tiles are
// resident; below one tile per CU most of the chip idles.  While n <= 32 x the CU count a workgroup therefore owns 32 rows
// and its four waves split the OUTPUT features of every product: wave w computes accumulator w alone (a quarter of the
// MFMAs), reading its 32 weight rows from L2 straight into the A operand's registers, one chunk ahead.  A slice's hidden
// block goes through LDS to the other three waves (it is everybody's B operand), the post norm's two sums likewise.  Every
// output element is the same chain of MFMAs over the same k in the same order as in the tile kernel, and the LayerNorms are
// written with their fusions spelled out (ln_rows<true>) in both, so the two kernels give the same bits: which one runs is
// a matter of speed only, and a row's result does not depend on n.
//
// The tile kernel itself (gf_ffn_kernel) and the argument checks are in gf_ffn.hpp, which the training step (ffn_train.hip,
// DESIGN.md §3.13d) shares; this file instantiates the plain build only and stays a translation unit of its own, so that its
// four kernels are compiled as they were before the training step existed.
#include "gf_ffn.hpp"

namespace gf {

// n <= 32 CUs' worth of rows: 32 rows per workgroup, wave w owns feature block w of every product (see the top)
template <int CIN>
__global__ __launch_bounds__(256) void gf_ffn_rows32_kernel(FfnArgs a)
{
    constexpr int NB = CIN / 32, PER = NB + 4;
    constexpr int vPre = 0, vB1 = 2 * CIN / 4, vB2 = vB1 + kFfnF / 4, vBid = vB2 + 32, vPost = vBid + 32, vEnd = vPost + 64;
    __shared__ float4 s_vec[vEnd];
    __shared__ float s_hid[2][4][16][64];    // [slice parity][block][register][lane]
    __shared__ float s_sum[2][4][64];        // the post norm's two sums: [which][block][lane]
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = blockIdx.x * 32;
    const size_t row = (size_t)min(row0 + j, a.n - 1);
    const int G = kFfnSlices * PER + (a.wid ? NB : 0);

    // the lane's A operands of chunk g: its weight row's 4 float4 at columns 8 m + 4 h of the chunk
    float4 cur[4], nxt[4];
    auto fetch = [&](float4 (&w4)[4], int g) {
        const int s = g / PER, c = g - s * PER;
        const float *p;
        if (s == kFfnSlices) p = a.wid + (size_t)(32 * wv + j) * CIN + 32 * c;
        else if (c < NB) p = a.w1 + (size_t)(128 * s + 32 * wv + j) * CIN + 32 * c;
        else p = a.w2 + (size_t)(32 * wv + j) * kFfnF + 128 * s + 32 * (c - NB);
#pragma unroll
        for (int m = 0; m < 4; ++m) w4[m] = ld4(p + 8 * m + 4 * h);
    };
    auto step = [&](f32x16 &acc, const f32x16 &xb, int g) {
        const bool more = g + 1 < G;
        if (more) fetch(nxt, g + 1);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[m].x, xb[4 * m + 0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[m].y, xb[4 * m + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[m].z, xb[4 * m + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[m].w, xb[4 * m + 3], acc, 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int m = 0; m < 4; ++m) cur[m] = nxt[m];
        }
    };

    fetch(cur, 0);
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
    f32x16 u[NB];   // every wave holds the whole row: it is the B operand of all of them
    load_row(u, a.x + row * CIN, h);
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
        ln_rows<true, NB>(u, tree_sum<NB>(part), s_vec + vPre, s_vec + vPre + CIN / 4, h);
    }

    f32x16 hw, y, hid[4];
#pragma unroll
    for (int r = 0; r < 16; ++r) y[r] = 0.f;
    int g = 0;
#pragma unroll 1
    for (int s = 0; s < kFfnSlices; ++s) {
#pragma unroll
        for (int r = 0; r < 16; ++r) hw[r] = 0.f;
#pragma unroll
        for (int c = 0; c < NB; ++c) step(hw, u[c], g++);
        const float4 *b1 = s_vec + vB1 + 32 * s + 8 * wv;
        float (*hs)[16][64] = s_hid[s & 1];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 bb = b1[2 * m + h];
            const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = hw[4 * m + i] + bv[i];
                hs[wv][4 * m + i][l] = v < 0.f ? 0.f : v;
            }
        }
        // (one barrier per slice: the other parity's buffer is rewritten only behind the next slice's barrier)
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) hid[b][r] = hs[b][r][l];
#pragma unroll
        for (int c = 0; c < 4; ++c) step(y, hid[c], g++);
    }
    if (a.wid) {
#pragma unroll
        for (int c = 0; c < NB; ++c) step(y, u[c], g++);
    }

    // the wave's 32 features of y + b2 (+ bid) (+ residual); the block's sums in the tile kernel's order
    const float *rrow = a.residual ? a.residual + row * kFfnE : nullptr;
    float sum = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float4 bb = s_vec[vB2 + 8 * wv + 2 * m + h];
        float add[4] = {bb.x, bb.y, bb.z, bb.w};
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = y[4 * m + i] + add[i];
        if (a.wid) {
            const float4 ii = s_vec[vBid + 8 * wv + 2 * m + h];
            v[0] += ii.x; v[1] += ii.y; v[2] += ii.z; v[3] += ii.w;
        }
        if (a.residual) {
            const float4 rr = ld4(rrow + 32 * wv + 8 * m + 4 * h);
            v[0] += rr.x; v[1] += rr.y; v[2] += rr.z; v[3] += rr.w;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            y[4 * m + i] = v[i];
            sum += v[i];
        }
    }
    if (a.post_g)   // ln_rows<true, 4> with the four blocks' sums met in LDS
        ln_rows_split(y, sum, s_sum, wv, l, [&](int which, int m) { return s_vec[vPost + 32 * which + 8 * wv + 2 * m + h]; });
    if (row0 + j < a.n) {
        float *orow = a.out + (size_t)(row0 + j) * kFfnE + 32 * wv + 4 * h;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            *reinterpret_cast<float4 *>(orow + 8 * m) = make_float4(y[4 * m], y[4 * m + 1], y[4 * m + 2], y[4 * m + 3]);
    }
}

}  // namespace gf

extern "C" int gf_ffn_forward(int n, int Cin, int F, int E, const float *x, const void *const *params, const float *residual,
                              float *out, void *stream_)
{
    using namespace gf;
    const char *fn = __func__;
    if (int rc = ffn_check(fn, n, Cin, F, E, x, params, residual, out)) return rc;
    if (n == 0) return GF_OK;
    GF_REFUSE_AS(fn, x && out, "null pointer");
    const float *const *p = reinterpret_cast<const float *const *>(params);
    FfnArgs a{x, residual, out, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], n};
    hipStream_t stream = (hipStream_t)stream_;
    if ((n + 31) / 32 <= cu_count()) {   // at most one 32-row workgroup per CU: the same bits, sooner
        const dim3 grid((n + 31) / 32);
        if (Cin == 256) hipLaunchKernelGGL(gf_ffn_rows32_kernel<256>, grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(gf_ffn_rows32_kernel<128>, grid, dim3(256), 0, stream, a);
    } else {
        const dim3 grid((n + kRowTile - 1) / kRowTile);
        if (Cin == 256) hipLaunchKernelGGL((gf_ffn_kernel<256, false>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((gf_ffn_kernel<128, false>), grid, dim3(256), 0, stream, a);
    }
    GF_CHECK_LAUNCH();
    return GF_OK;
}
