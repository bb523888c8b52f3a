// The dense ends of the deformable block, DeformableFeatureAggregation.forward (model/encoder/gaussian_encoder/
// deformable_module.py:146-262), around the native middle (key_points.hip, daf_fused.hip).  The contract: include/gf_hip.h;
// the design and the measured numbers: DESIGN.md §3.13e.
//
// Front, gf_deform_logits_forward, one launch:
//     learned = Wl f + bl              Wl = kps_generator.learnable_fc.weight [3K, 128]   (:59-63; f, NOT f + e)
//     raw     = Ww (f + e) + bw        Ww = weights_fc.weight [Nw, 128]                   (:250-262)
// Back, gf_deform_output_forward, one launch:
//     y   = Wo feats + bo              Wo = output_proj.weight [128, 128]                 (:243)
//     out = y | y + f | [y | f]        residual_mode "none" | "add" | "cat"               (:244-247)
//     out = LN(out + residual)         the encoder's "add", "norm" behind the block, where given (not with "cat")
//
// Organisation: gf_rows.hpp's.  A wave owns 32 rows; f, and f + e formed in registers, are B operands as loaded.  The 128-row
// kernels stage every weight chunk (128 output columns x 32 inputs) through the double-buffered LDS staging, one barrier per
// chunk; a product over the 128 inputs is four chunks.  The front walks the learned columns first (one accumulator), then raw's
// columns in groups of 128 with as many accumulators as the group has blocks of 32 columns: a weight row past the width is
// staged as zeros, its column is never stored.  Finished columns leave through an LDS tile of their own (the weight buffers
// are busy with the next group), learned as the wave's contiguous run of 32 x 3K floats.
//
// Few rows (the *_rows32_kernel): as in ffn.hip, while n <= 32 x the CU count a workgroup owns 32 rows and its four waves
// split the OUTPUT columns in blocks of 32, each wave reading its weight rows from L2 straight into the A operand's registers;
// no LDS but the post norm's two sums.  Every output element is the same chain of MFMAs over the same k in the same order, the
// same additions behind it and the LayerNorm with its fusions spelled out (ln_rows<true>) in both, so the two kernels of an
// op give the same bits: a row's result does not depend on n.
//
// Rows past n compute on row n - 1 and are not stored.  No workspace, no atomics.
//
// The back's 128-row kernel, its arguments and its checks are in gf_deform.hpp, which the back's training step
// (deform_dense_train.hip) shares: a translation unit of its own, so that this one's kernels stay the
// instruction streams they are.
#include <type_traits>

#include "gf_deform.hpp"

namespace gf {

struct DeformLogitsArgs {
    const float *f, *e, *wl, *bl, *ww, *bw;
    float *learned, *raw;
    int n, K3, Nw;
};
// f and s = f + e (f itself without e) of the lane's row
__device__ __forceinline__ void load_operands(f32x16 (&f)[4], f32x16 (&s)[4], const DeformLogitsArgs &a, size_t row, int h)
{
    load_row(f, a.f + row * kDeformE, h);
    if (a.e) {
        load_row(s, a.e + row * kDeformE, h);
#pragma unroll
        for (int b = 0; b < 4; ++b) s[b] += f[b];
    } else {
#pragma unroll
        for (int b = 0; b < 4; ++b) s[b] = f[b];
    }
}
// the 16 MFMAs of one chunk on the A operands a lane holds in registers (the rows32 kernels)
__device__ __forceinline__ void lane_mfma(f32x16 &acc, const f32x16 &xb, const float4 (&w4)[4])
{
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w4[m].x, xb[4 * m + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w4[m].y, xb[4 * m + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w4[m].z, xb[4 * m + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w4[m].w, xb[4 * m + 3], acc, 0, 0, 0);
    }
}

// ---- front ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void gf_deform_logits_kernel(DeformLogitsArgs a)
{
    __shared__ float4 s_w[2][128 * kRowPitch4];
    __shared__ float s_out[4][32 * kRowOutPitch];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = blockIdx.x * kRowTile + wv * 32;
    const size_t row = (size_t)min(row0 + j, a.n - 1);
    const int nl = a.K3 > 0, groups = (a.Nw + 127) / 128, G = 4 * (nl + groups);
    float *so = s_out[wv];

    float4 pre[4];
    auto fetch = [&](int g) {     // chunk g of the walk (uniform): the learned columns' four, then four per group of raw's
        const int q = (g >> 2) - nl, c = g & 3;
        if (q < 0) chunk_fetch_rows(pre, a.wl, kDeformE, 32 * c, t, a.K3);
        else chunk_fetch_rows(pre, a.ww + (size_t)(128 * q) * kDeformE, kDeformE, 32 * c, t, a.Nw - 128 * q);
    };
    int g = 0;
    // acc <- the next four chunks against x; the chunk behind is fetched before a chunk's MFMAs and stashed after them
    auto product = [&](auto &acc, const f32x16 (&x)[4]) {
        constexpr int NFB = std::extent_v<std::remove_reference_t<decltype(acc)>>;
#pragma unroll
        for (int b = 0; b < NFB; ++b) zero_block(acc[b]);
#pragma unroll
        for (int c = 0; c < 4; ++c, ++g) {
            const bool more = g + 1 < G;
            if (more) fetch(g + 1);
            chunk_mfma<NFB>(acc, x[c], s_w[c & 1], j, h);
            if (more) chunk_stash(s_w[(c & 1) ^ 1], pre, t);
            __syncthreads();
        }
    };

    fetch(0);
    f32x16 f[4], s[4];     // s: e until the learned columns are done with f, then f + e (f dies there)
    load_row(f, a.f + row * kDeformE, h);
    if (a.e) load_row(s, a.e + row * kDeformE, h);
    chunk_stash(s_w[0], pre, t);
    __syncthreads();

    if (nl) {
        f32x16 acc[1];
        product(acc, f);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = 8 * m + 4 * h + i;
                if (col < a.K3) so[j * a.K3 + col] = acc[0][4 * m + i] + a.bl[col];
            }
        __syncthreads();
        // the wave's rows of learned are one run of memory
        const int count = min(32, a.n - row0) * a.K3;
        for (int k = l; k < count; k += 64) a.learned[(size_t)row0 * a.K3 + k] = so[k];
        __syncthreads();
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) s[b] = a.e ? s[b] + f[b] : f[b];
#pragma unroll 1
    for (int q = 0; q < groups; ++q) {
        const int col0 = 128 * q, ncols = min(128, a.Nw - col0);
        auto group = [&](auto nfb) {
            constexpr int NFB = decltype(nfb)::value;
            f32x16 acc[NFB];
            product(acc, s);
#pragma unroll
            for (int b = 0; b < NFB; ++b)
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int col = col0 + 32 * b + 8 * m + 4 * h;
                    const float4 bb = col < a.Nw ? ld4(a.bw + col) : make_float4(0.f, 0.f, 0.f, 0.f);
                    acc[b][4 * m] += bb.x; acc[b][4 * m + 1] += bb.y; acc[b][4 * m + 2] += bb.z; acc[b][4 * m + 3] += bb.w;
                }
            store_cols<NFB>(so, acc, a.raw, (size_t)a.Nw, col0, ncols, row0, a.n, l, j, h);
        };
        switch ((ncols + 31) / 32) {
        case 1: group(std::integral_constant<int, 1>()); break;
        case 2: group(std::integral_constant<int, 2>()); break;
        case 3: group(std::integral_constant<int, 3>()); break;
        default: group(std::integral_constant<int, 4>()); break;
        }
    }
}

// n <= 32 CUs' worth of rows: 32 rows per workgroup; the blocks of 32 output columns -- the learned columns' one, then raw's --
// are dealt to the four waves in turn (see the top)
__global__ __launch_bounds__(256) void gf_deform_logits_rows32_kernel(DeformLogitsArgs a)
{
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = blockIdx.x * 32;
    const size_t row = (size_t)min(row0 + j, a.n - 1);
    const bool valid = row0 + j < a.n;
    const int nl = a.K3 > 0, nblk = nl + (a.Nw + 31) / 32;
    const int mine = nblk > wv ? (nblk - wv + 3) / 4 : 0;      // the wave's blocks: wv, wv + 4, ..

    // the lane's A operands of chunk g of the wave's walk: its weight row's 4 float4 at columns 8 m + 4 h of the chunk
    float4 cur[4], nxt[4];
    auto fetch = [&](float4 (&w4)[4], int g) {
        const int q = wv + 4 * (g >> 2) - nl, c = g & 3;
        const float *w = q < 0 ? a.wl : a.ww + (size_t)(32 * q) * kDeformE;
        const int rows = q < 0 ? a.K3 : a.Nw - 32 * q;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            w4[m] = j < rows ? ld4(w + (size_t)j * kDeformE + 32 * c + 8 * m + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto product = [&](f32x16 &acc, const f32x16 (&x)[4], int i) {    // the wave's i-th block
        zero_block(acc);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool more = 4 * i + c + 1 < 4 * mine;
            if (more) fetch(nxt, 4 * i + c + 1);
            lane_mfma(acc, x[c], cur);
            if (more) {
#pragma unroll
                for (int m = 0; m < 4; ++m) cur[m] = nxt[m];
            }
        }
    };

    if (mine > 0) fetch(cur, 0);
    f32x16 f[4], s[4], acc;
    load_operands(f, s, a, row, h);
#pragma unroll 1
    for (int i = 0; i < mine; ++i) {
        const int q = wv + 4 * i - nl;
        if (q < 0) {
            product(acc, f, i);
            if (valid) {
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int col = 8 * m + 4 * h + k;
                        if (col < a.K3) a.learned[row * a.K3 + col] = acc[4 * m + k] + a.bl[col];
                    }
            }
        } else {
            product(acc, s, i);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int col = 32 * q + 8 * m + 4 * h;
                if (valid && col < a.Nw) {
                    const float4 bb = ld4(a.bw + col);
                    *reinterpret_cast<float4 *>(a.raw + row * a.Nw + col) =
                        make_float4(acc[4 * m] + bb.x, acc[4 * m + 1] + bb.y, acc[4 * m + 2] + bb.z, acc[4 * m + 3] + bb.w);
                }
            }
        }
    }
}

// ---- back -------------------------------------------------------------------------------------------------------------------

// n <= 32 CUs' worth of rows: 32 rows per workgroup, wave w owns output features 32 w .. 32 w + 31 (see the top)
__global__ __launch_bounds__(256) void gf_deform_output_rows32_kernel(DeformOutputArgs a)
{
    __shared__ float s_sum[2][4][64];        // the norm's two sums: [which][block][lane]
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = blockIdx.x * 32;
    const size_t row = (size_t)min(row0 + j, a.n - 1);
    const bool valid = row0 + j < a.n;

    float4 w4[4][4];     // the lane's A operands of the four chunks: its weight row 32 wv + j
    {
        const float *wrow = a.w + (size_t)(32 * wv + j) * kDeformE + 4 * h;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int m = 0; m < 4; ++m) w4[c][m] = ld4(wrow + 32 * c + 8 * m);
    }
    f32x16 x[4], y;
    load_row(x, a.x + row * kDeformE, h);
    zero_block(y);
#pragma unroll
    for (int c = 0; c < 4; ++c) lane_mfma(y, x[c], w4[c]);

    // the wave's 32 features of y + bias (+ f) (+ residual); the block's sums in the tile kernel's order
    const int at = 32 * wv + 4 * h;
    const float *frow = a.mode != GF_DEFORM_NONE ? a.f + row * kDeformE + at : nullptr;
    const float *rrow = a.residual ? a.residual + row * kDeformE + at : nullptr;
    float sum = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float4 bb = ld4(a.b + at + 8 * m);
        float v[4] = {y[4 * m] + bb.x, y[4 * m + 1] + bb.y, y[4 * m + 2] + bb.z, y[4 * m + 3] + bb.w};
        if (frow) {
            const float4 ff = ld4(frow + 8 * m);
            if (a.mode == GF_DEFORM_ADD) {
                v[0] += ff.x; v[1] += ff.y; v[2] += ff.z; v[3] += ff.w;
            } else if (valid) {   // "cat": the right half
                *reinterpret_cast<float4 *>(a.out + row * (2 * kDeformE) + kDeformE + at + 8 * m) = ff;
            }
        }
        if (rrow) {
            const float4 rr = ld4(rrow + 8 * m);
            v[0] += rr.x; v[1] += rr.y; v[2] += rr.z; v[3] += rr.w;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            y[4 * m + i] = v[i];
            sum += v[i];
        }
    }
    if (a.gam)   // ln_rows<true, 4> with the four blocks' sums met in LDS
        ln_rows_split(y, sum, s_sum, wv, l, [&](int which, int m) { return ld4((which ? a.bet : a.gam) + at + 8 * m); });
    if (valid) {
        float *orow = a.out + row * (a.mode == GF_DEFORM_CAT ? 2 * kDeformE : kDeformE) + at;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            *reinterpret_cast<float4 *>(orow + 8 * m) = make_float4(y[4 * m], y[4 * m + 1], y[4 * m + 2], y[4 * m + 3]);
    }
}

}  // namespace gf

extern "C" int gf_deform_logits_forward(int n, int E, int K3, int Nw, const float *feature, const float *embed,
                                        const void *const *params, float *learned, float *raw, void *stream_)
{
    using namespace gf;
    static const char *const name[GF_DEFORM_LOGITS_PARAMS] = {"kps_generator.learnable_fc.weight", "kps_generator.learnable_fc.bias",
                                                              "weights_fc.weight", "weights_fc.bias"};
    GF_REFUSE_AS(__func__, E == kDeformE, "E = %d: only embed_dims = 128 is supported", E);
    GF_REFUSE_AS(__func__, K3 >= 0 && K3 <= GF_DEFORM_MAX_LEARNED, "K3 = %d: the learned columns 3 K must be 0 .. %d", K3, GF_DEFORM_MAX_LEARNED);
    GF_REFUSE_AS(__func__, Nw >= 4 && Nw % 4 == 0, "Nw = %d: the logits' width must be a positive multiple of 4", Nw);
    GF_REFUSE_AS(__func__, n >= 0, "n = %d is negative", n);
    GF_REFUSE_AS(__func__, params, "null params");
    const float *const *p = reinterpret_cast<const float *const *>(params);
    for (int i = K3 > 0 ? 0 : 2; i < GF_DEFORM_LOGITS_PARAMS; ++i) {
        GF_REFUSE_AS(__func__, p[i], "%s is missing", name[i]);
        GF_REFUSE_AS(__func__, !misaligned16(p[i]), "%s is not 16-byte aligned", name[i]);
    }
    GF_REFUSE_AS(__func__, !misaligned16(feature), "instance_feature is not 16-byte aligned");
    GF_REFUSE_AS(__func__, !misaligned16(embed), "anchor_embed is not 16-byte aligned");
    GF_REFUSE_AS(__func__, !misaligned16(learned), "learned is not 16-byte aligned");
    GF_REFUSE_AS(__func__, !misaligned16(raw), "raw is not 16-byte aligned");
    if (n == 0) return GF_OK;
    GF_REFUSE_AS(__func__, feature && raw && (K3 == 0 || learned), "null pointer");
    const size_t in_bytes = (size_t)n * kDeformE * 4, raw_bytes = (size_t)n * Nw * 4, learned_bytes = (size_t)n * K3 * 4;
    GF_REFUSE_AS(__func__, !overlap(raw, raw_bytes, feature, in_bytes) && !overlap(raw, raw_bytes, embed, in_bytes), "raw aliases an input");
    GF_REFUSE_AS(__func__, !overlap(learned, learned_bytes, feature, in_bytes) && !overlap(learned, learned_bytes, embed, in_bytes),
                     "learned aliases an input");
    GF_REFUSE_AS(__func__, !overlap(learned, learned_bytes, raw, raw_bytes), "learned aliases raw");
    DeformLogitsArgs a{feature, embed, K3 > 0 ? p[0] : nullptr, K3 > 0 ? p[1] : nullptr, p[2], p[3], learned, raw, n, K3, Nw};
    hipStream_t stream = (hipStream_t)stream_;
    if ((n + 31) / 32 <= cu_count())   // at most one 32-row workgroup per CU: the same bits, sooner
        hipLaunchKernelGGL(gf_deform_logits_rows32_kernel, dim3((n + 31) / 32), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(gf_deform_logits_kernel, dim3((n + kRowTile - 1) / kRowTile), dim3(256), 0, stream, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_deform_output_forward(int n, int E, int mode, const float *features, const float *instance_feature,
                                        const void *const *params, const float *residual, float *out, void *stream_)
{
    using namespace gf;
    if (int rc = deform_output_check(__func__, n, E, mode, params, residual != nullptr)) return rc;
    if (int rc = deform_output_check_rows(__func__, n, mode, features, instance_feature, residual, out)) return rc;
    if (n == 0) return GF_OK;
    const float *const *p = reinterpret_cast<const float *const *>(params);
    DeformOutputArgs a{features, mode == GF_DEFORM_NONE ? nullptr : instance_feature, residual, p[0], p[1], p[2], p[3], out, n, mode};
    hipStream_t stream = (hipStream_t)stream_;
    if ((n + 31) / 32 <= cu_count())   // at most one 32-row workgroup per CU: the same bits, sooner
        hipLaunchKernelGGL(gf_deform_output_rows32_kernel, dim3((n + 31) / 32), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(gf_deform_output_kernel<DeformOutputArgs>, dim3((n + kRowTile - 1) / kRowTile), dim3(256), 0, stream, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
