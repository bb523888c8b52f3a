// The refinement modules' MLP and tail in one launch, forward only: what SparseGaussian3DRefinementModule.forward
// (model/encoder/gaussian_encoder/refine_module.py:70-123) and SparseGaussian3DRefinementModuleV2.forward
// (refine_module_v2.py:62-107) compute from (instance_feature, anchor, anchor_embed).  The contract: include/gf_hip.h; the
// design and the measured numbers: DESIGN.md §3.12b.
//
// The MLP (`layers`) is Linear, ReLU, Linear, ReLU, LayerNorm twice over 128 features, then Linear(128 -> D) and Scale.  torch
// runs it as a dozen kernels that each read and write an [n, 128] tensor; here a row's features stay in registers, in
// gf_rows.hpp's layout: a workgroup of four waves owns 128 rows, a wave 32, every product is Y^T = W X^T on
// v_mfma_f32_32x32x2_f32 (exact fp32), and a product's accumulators are the next product's B operands as they stand.  The
// weights are read in torch's layout, in chunks of 32 input columns double-buffered through LDS: 20 chunks in one walk, four
// for each square Linear and four of 64 rows for the last one, whose rows from D on are supplied as zero -- the row index is
// clamped and the value masked, nothing beyond the tensor is loaded -- and whose product takes two accumulators.
//
// The tail is gf_refine.hpp's, the code gf_refine_forward runs.  After bias and Scale a wave writes its 32 x D result into an
// LDS tile of odd pitch in the weight buffers (idle by then), loads its 32 anchor rows next to it, and lanes 0-31 take one row
// each; the outputs leave as contiguous runs out of the tiles.  Four waves of 32 rows keep all four SIMDs busy and need no
// hand-over between waves.  The tiles of the four waves fit the weight buffers when po + pa + pn <= 72 floats per row (every
// shipped config: 67); wider rows (D = 43: 95) go in two passes of two waves.
//
// Rows past n in the last tile compute on row n - 1 and are not stored.
//
// The training step's forward (gf_refine_mlp_forward_train) is the same kernel's SAVE instantiation; the
// backward is refine_mlp_train.hip.
#include <type_traits>

#include "gf_refine.hpp"
#include "gf_rows.hpp"

namespace gf {

constexpr int kRmVecs = 8;                    // b0 | b2, LN4 weight, bias | b5 | b7, LN9 weight, bias: 32 float4 each
constexpr int kRmTail4 = kRmVecs * 32;         // then layers.10.bias and layers.11.scale, 64 floats each, zero from D on
constexpr int kRmWeightFloats = 2 * kRmE * kRowPitch4 * 4;
constexpr int kRmFitAll = kRmWeightFloats / kRowTile;        // floats per row that four waves' tiles may take: 72
static_assert(10 + 1 + kRefMaxS <= 64, "the last product's two accumulators hold D features");
static_assert((((10 + 1 + kRefMaxS) | 1) * 2 + ((kNSem + kRefMaxS) | 1)) * 64 <= kRmWeightFloats, "two waves' widest tiles fit the weight buffers");

struct RefineMlpArgs {
    RefineArgs r;
    const float *feat, *embed;
    const float *w[5];            // layers.0, .2, .5, .7 [128, 128], layers.10 [D, 128]
    const float *vec[kRmVecs];
    const float *b10, *scale;     // [D]
    float *mlp_out;               // [n, D] or null
    int wpp;                      // waves per pass of the tail: 4, or 2 where four waves' tiles do not fit
};
// the saving forward's (gf_refine_mlp_forward_train): the plain kernel's arguments as they are, then where the saved rows go
struct RefineMlpTrainArgs : RefineMlpArgs {
    float *sv_rows, *sv_stat, *sv_y, *sv_o;   // gf_refine.hpp's RefineMlpSaved
};

// v <- relu(v + bias); p: the bias in LDS, 32 float4
__device__ __forceinline__ void bias_relu(f32x16 (&v)[4], const float4 *p, int h)
{
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 bb = p[8 * b + 2 * m + h];
            const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float x = v[b][4 * m + i] + bv[i];
                v[b][4 * m + i] = x < 0.f ? 0.f : x;     // (not fmaxf: a NaN stays a NaN, as torch's relu keeps it)
            }
        }
}

// SAVE: the training step's forward.  The same stages on the same expressions (relu_ln<true> spells out the plain build's
// fusions, gf_rows.hpp), and each lane also stores what the backward needs of its row: the four post-ReLU rows, the two
// LayerNorms' (mean, rstd), the last Linear's result before Scale and o.  tests/test_refine_mlp_train_gpu.py holds the two
// instantiations together bit for bit
template <int VERSION, bool SAVE = false>
__global__ __launch_bounds__(256, 2) void gf_refine_mlp_kernel(std::conditional_t<SAVE, RefineMlpTrainArgs, RefineMlpArgs> a)
{
    __shared__ float4 s_w[2][kRmE * kRowPitch4];
    __shared__ float4 s_vec[kRmTail4 + 32];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int n = a.r.n, D = a.r.D;
    const int row0 = blockIdx.x * kRowTile + wv * 32;
    const size_t row = (size_t)min(row0 + j, n - 1);

    float4 pre[4];
    auto fetch = [&](int g) {     // chunk g of the walk (g is uniform)
        const int s = g >> 2, c = g & 3;
        if (s < 4) {
            chunk_fetch(pre, a.w[s], kRmE, 32 * c, t);
        } else {                  // layers.10: rows 0 .. 63, those from D on as zero
            const int ff = t >> 3, fq = t & 7;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = ff + 32 * i;
                const float4 v = ld4(a.w[4] + (size_t)min(r, D - 1) * kRmE + 32 * c + 4 * fq);
                pre[i] = r < D ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            pre[2] = pre[3] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    f32x16 x[4], acc[4];
    fetch(0);
    // the biases and LayerNorm vectors into LDS once: a wave takes every fourth vector, half a wave moves one
    {
        const int v0 = __builtin_amdgcn_readfirstlane(wv);
        float4 vec[kRmVecs / 4];
#pragma unroll
        for (int i = 0; i < kRmVecs / 4; ++i) vec[i] = ld4(a.vec[v0 + 4 * i] + 4 * j);
        float tail = 0.f;
        if (v0 < 2) {
            const float *src = v0 == 0 ? a.b10 : a.scale;
            const float v = src[min(l, D - 1)];
            tail = l < D ? v : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kRmVecs / 4; ++i)
            if (l < 32) s_vec[(v0 + 4 * i) * 32 + l] = vec[i];
        if (v0 < 2) reinterpret_cast<float *>(s_vec + kRmTail4)[64 * v0 + l] = tail;
    }
    // x = instance_feature + anchor_embed, in the B-operand layout from the two global rows
    {
        const float *fr = a.feat + row * kRmE, *er = a.embed + row * kRmE;
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float4 u = ld4(fr + 32 * b + 8 * m + 4 * h), v = ld4(er + 32 * b + 8 * m + 4 * h);
                x[b][4 * m] = u.x + v.x; x[b][4 * m + 1] = u.y + v.y; x[b][4 * m + 2] = u.z + v.z; x[b][4 * m + 3] = u.w + v.w;
            }
    }
    chunk_stash(s_w[0], pre, t);
    __syncthreads();

    // the four square stages: chunk g + 1 is fetched before chunk g's 64 MFMAs and written to the other buffer after them
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            fetch(4 * q + c + 1);
            chunk_mfma(acc, x[c], s_w[c & 1], j, h);
            chunk_stash(s_w[(c + 1) & 1], pre, t);
            __syncthreads();
        }
        const float4 *p = s_vec + 32 * (4 * (q >> 1) + (q & 1));
        if constexpr (SAVE) {
            // the stage's post-ReLU row [q][row][128]; a row past n stores nothing
            float *rrow = row0 + j < n ? a.sv_rows + ((size_t)q * n + row) * kRmE : nullptr;
            if (q & 1) {
                relu_ln<true>(acc, p, h, rrow, a.sv_stat + ((size_t)(q >> 1) * n + row) * 2);
            } else {
                bias_relu(acc, p, h);
                if (rrow) store_row_regs(rrow, acc, h);
            }
        } else {
            if (q & 1) relu_ln<false>(acc, p, h);      // layers.2 -> .3 -> .4, layers.7 -> .8 -> .9
            else bias_relu(acc, p, h);                 // layers.0 -> .1,       layers.5 -> .6
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) x[b] = acc[b];
    }

    // layers.10 and .11: 64 output features, of which the first D are the row's result
    f32x16 y[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) y[b][r] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c < 3) fetch(17 + c);
        chunk_mfma(y, x[c], s_w[c & 1], j, h);
        if (c < 3) chunk_stash(s_w[(c + 1) & 1], pre, t);
        __syncthreads();
    }
    {
        const float4 *pb = s_vec + kRmTail4, *ps = pb + 16;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float4 bb = pb[8 * b + 2 * m + h], ss = ps[8 * b + 2 * m + h];
                const float bv[4] = {bb.x, bb.y, bb.z, bb.w}, sv[4] = {ss.x, ss.y, ss.z, ss.w};
                if constexpr (SAVE) {     // the value before Scale, to its row (features from D on: 0, as the weight and bias are)
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[b][4 * m + i] = y[b][4 * m + i] + bv[i];
                    if (row0 + j < n)
                        *reinterpret_cast<float4 *>(a.sv_y + row * kRmYPitch + 32 * b + 8 * m + 4 * h) =
                            make_float4(y[b][4 * m], y[b][4 * m + 1], y[b][4 * m + 2], y[b][4 * m + 3]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[b][4 * m + i] = y[b][4 * m + i] * sv[i];
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[b][4 * m + i] = (y[b][4 * m + i] + bv[i]) * sv[i];
                }
            }
    }

    // the tail, through the (idle) weight buffers: the last chunk's barrier is behind every wave's reads of them
    float *tiles = reinterpret_cast<float *>(&s_w[0][0]);
    const int po = a.r.po, pa = a.r.pa, pn = a.r.pn;
    const int rows = min(32, n - row0);      // <= 0: the wave has nothing to store
    const size_t first = (size_t)row0;
    for (int p0 = 0; p0 < 4; p0 += a.wpp) {
        const bool mine = wv >= p0 && wv < p0 + a.wpp;
        float *t_o = tiles + (mine ? wv - p0 : 0) * (32 * (po + pa + pn)), *t_a = t_o + 32 * po, *t_n = t_a + 32 * pa;
        if (mine) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = 32 * b + 8 * (r >> 2) + 4 * h + (r & 3);
                    if (f < D) t_o[j * po + f] = y[b][r];
                }
            tile_load(a.r.anchor, first, a.r.Da, t_a, pa, 0, a.r.C, rows);
        }
        __syncthreads();
        if (mine) {
            if (a.mlp_out) tile_store(a.mlp_out, first, t_o, po, 0, D, D, rows);
            if constexpr (SAVE) tile_store(a.sv_o, first, t_o, po, 0, D, D, rows);
            if (l < rows) refine_row_forward<VERSION>(a.r, t_o + l * po, t_a + l * pa, t_n + l * pn);
        }
        __syncthreads();
        if (mine) refine_store_forward<VERSION>(a.r, first, t_o, t_n, rows);
        if (p0 + a.wpp < 4) __syncthreads();      // the next pass writes the same tiles
    }
}

// Both forwards: the checks in one order under the name of the entry point that was called, then the plain kernel (saved
// null) or the saving one
static int refine_mlp_run(const char *fn, int n, int E, int D, int Da, int version, int flags, int R, int S, const double *consts,
                          const float *instance_feature, const float *anchor_embed, const float *anchor, const void *const *params,
                          float *mlp_out, float *anchor_out, float *means, float *scales, float *rotations, float *opacities,
                          float *semantics, float *original_means, float *delta_means, bool train, void *saved, size_t saved_bytes,
                          hipStream_t stream)
{
    RefineMlpTrainArgs a{};
    if (int rc = refine_fill_args(a.r, fn, n, D, Da, version, flags, R, S, consts)) return rc;
    GF_REFUSE_AS(fn, E == kRmE, "E = %d: only embed_dims = 128 is supported", E);
    if (n == 0) return GF_OK;
    if (int rc = refine_mlp_check_inputs(fn, params, instance_feature, anchor_embed, anchor)) return rc;
    GF_CHECK_ARG_AS(fn, refine_forward_outputs_present(version, flags, S, anchor_out, means, scales, rotations, opacities, semantics, original_means, delta_means),
                    "null pointer");
    if (train) {
        GF_REFUSE_AS(fn, saved, "saved is null");
        GF_REFUSE_AS(fn, !misaligned16(saved), "saved = %p is not 16-byte aligned", saved);
        const RefineMlpSaved sv = refine_mlp_carve_saved(saved, n, D);
        GF_CHECK_WORKSPACE_AS(fn, "saved", saved_bytes, sv.bytes);
        a.sv_rows = sv.rows; a.sv_stat = sv.stat; a.sv_y = sv.y; a.sv_o = sv.o;
    }
    const float *const *p = reinterpret_cast<const float *const *>(params);
    a.feat = instance_feature; a.embed = anchor_embed; a.mlp_out = mlp_out;
    a.r.anchor = anchor; a.r.anchor_out = anchor_out; a.r.means = means; a.r.scales = scales; a.r.rotations = rotations;
    a.r.opacities = opacities; a.r.semantics = semantics; a.r.original_means = original_means; a.r.delta_means = delta_means;
    const int wi[5] = {0, 2, 6, 8, 12}, vi[kRmVecs] = {1, 3, 4, 5, 7, 9, 10, 11};
    for (int i = 0; i < 5; ++i) a.w[i] = p[wi[i]];
    for (int i = 0; i < kRmVecs; ++i) a.vec[i] = p[vi[i]];
    a.b10 = p[13]; a.scale = p[14];
    a.wpp = a.r.po + a.r.pa + a.r.pn <= kRmFitAll ? 4 : 2;
    const dim3 grid((n + kRowTile - 1) / kRowTile), block(256);
    const RefineMlpArgs &plain = a;
    if (train) {
        if (version == 1) hipLaunchKernelGGL((gf_refine_mlp_kernel<1, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((gf_refine_mlp_kernel<2, true>), grid, block, 0, stream, a);
    } else {
        if (version == 1) hipLaunchKernelGGL((gf_refine_mlp_kernel<1, false>), grid, block, 0, stream, plain);
        else hipLaunchKernelGGL((gf_refine_mlp_kernel<2, false>), grid, block, 0, stream, plain);
    }
    GF_CHECK_LAUNCH_AS(fn);
    return GF_OK;
}

}  // namespace gf

extern "C" int gf_refine_mlp_forward(int n, int E, int D, int Da, int version, int flags, int R, int S, const double *consts,
                                     const float *instance_feature, const float *anchor_embed, const float *anchor,
                                     const void *const *params, float *mlp_out, float *anchor_out, float *means, float *scales,
                                     float *rotations, float *opacities, float *semantics, float *original_means, float *delta_means,
                                     void *stream_)
{
    return gf::refine_mlp_run(__func__, n, E, D, Da, version, flags, R, S, consts, instance_feature, anchor_embed, anchor, params, mlp_out,
                              anchor_out, means, scales, rotations, opacities, semantics, original_means, delta_means, false, nullptr, 0,
                              (hipStream_t)stream_);
}

extern "C" int gf_refine_mlp_forward_train(int n, int E, int D, int Da, int version, int flags, int R, int S, const double *consts,
                                           const float *instance_feature, const float *anchor_embed, const float *anchor,
                                           const void *const *params, float *mlp_out, float *anchor_out, float *means, float *scales,
                                           float *rotations, float *opacities, float *semantics, float *original_means,
                                           float *delta_means, void *saved, size_t saved_bytes, void *stream_)
{
    return gf::refine_mlp_run(__func__, n, E, D, Da, version, flags, R, S, consts, instance_feature, anchor_embed, anchor, params, mlp_out,
                              anchor_out, means, scales, rotations, opacities, semantics, original_means, delta_means, true, saved,
                              saved_bytes, (hipStream_t)stream_);
}
