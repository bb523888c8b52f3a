// gf_deform.hpp -- what the dense back of the deformable block (deform_dense.hip) and its training step (deform_dense_train.hip)
// share: the output launch's arguments, the 128-row output kernel with its saving form, and the entry points' argument checks.
// The design: DESIGN.md §3.13e, §3.13f.
#pragma once
#include <type_traits>

#include "gf_rows.hpp"

namespace gf {

constexpr int kDeformE = GF_DEFORM_EMBED_DIMS;
static_assert(kDeformE == 128, "a row is the four register blocks of gf_rows.hpp");

struct DeformOutputArgs {
    const float *x, *f, *residual, *w, *b, *gam, *bet;
    float *out;
    int n, mode;
};
struct DeformOutputTrainArgs : DeformOutputArgs {
    float *ysave, *stat;     // the row the post norm reads [n, 128] and its (mean, rstd) [n, 2]
};

__device__ __forceinline__ void zero_block(f32x16 &v)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = 0.f;
}

// y = Wo x + bo, the add or the cat, the residual and the post norm on a tile of 128 rows (deform_dense.hip's top).
// SAVE (the training step, with a post norm): the lane also stores its 64 values of the row the norm reads, as float4s from
// the registers, and the norm's (mean, rstd); out's bits are the plain kernel's
template <class Args>
__global__ __launch_bounds__(256) void gf_deform_output_kernel(Args a)
{
    constexpr bool SAVE = std::is_same_v<Args, DeformOutputTrainArgs>;
    constexpr int vB = 0, vG = 32, vBeta = 64;     // LDS vectors, in float4: output_proj.bias | the norm's weight | bias
    __shared__ float4 s_w[2][128 * kRowPitch4];
    __shared__ float4 s_vec[96];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = blockIdx.x * kRowTile + wv * 32;
    const size_t row = (size_t)min(row0 + j, a.n - 1);

    float4 pre[4];
    chunk_fetch(pre, a.w, kDeformE, 0, t);
    if (t < 32) s_vec[vB + t] = ld4(a.b + 4 * t);
    if (a.gam && t >= 64 && t < 96) s_vec[vG + (t - 64)] = ld4(a.gam + 4 * (t - 64));
    if (a.gam && t >= 96 && t < 128) s_vec[vBeta + (t - 96)] = ld4(a.bet + 4 * (t - 96));
    f32x16 x[4], y[4];
    load_row(x, a.x + row * kDeformE, h);
    chunk_stash(s_w[0], pre, t);
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 4; ++b) zero_block(y[b]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c < 3) chunk_fetch(pre, a.w, kDeformE, 32 * (c + 1), t);
        chunk_mfma<4>(y, x[c], s_w[c & 1], j, h);
        if (c < 3) chunk_stash(s_w[(c & 1) ^ 1], pre, t);
        __syncthreads();
    }

    // y + bias (+ f) (+ residual), the lane's sum of it for the norm
    const float *frow = a.mode == GF_DEFORM_ADD ? a.f + row * kDeformE : nullptr;
    const float *rrow = a.residual ? a.residual + row * kDeformE : nullptr;
    float part[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float sum = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 bb = s_vec[vB + 8 * b + 2 * m + h];
            float v[4] = {y[b][4 * m] + bb.x, y[b][4 * m + 1] + bb.y, y[b][4 * m + 2] + bb.z, y[b][4 * m + 3] + bb.w};
            if (frow) {
                const float4 ff = ld4(frow + 32 * b + 8 * m + 4 * h);
                v[0] += ff.x; v[1] += ff.y; v[2] += ff.z; v[3] += ff.w;
            }
            if (rrow) {   // last, so that a residual of zeros changes nothing
                const float4 rr = ld4(rrow + 32 * b + 8 * m + 4 * h);
                v[0] += rr.x; v[1] += rr.y; v[2] += rr.z; v[3] += rr.w;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                y[b][4 * m + i] = v[i];
                sum += v[i];
            }
        }
        part[b] = sum;
    }
    if constexpr (SAVE) {
        const bool valid = row0 + j < a.n;
        if (valid) store_row_regs(a.ysave + row * kDeformE, y, h);
        ln_rows<true, 4>(y, tree_sum<4>(part), s_vec + vG, s_vec + vBeta, h, valid ? a.stat + 2 * row : nullptr);
    } else if (a.gam) {
        ln_rows<true, 4>(y, tree_sum<4>(part), s_vec + vG, s_vec + vBeta, h);
    }
    // through the (idle) weight buffers: the last chunk's barrier is behind every wave's reads of them
    float *so = reinterpret_cast<float *>(&s_w[0][0]) + wv * (32 * kRowOutPitch);
    if (a.mode == GF_DEFORM_CAT) {
        store_cols<4>(so, y, a.out, 2 * kDeformE, 0, kDeformE, row0, a.n, l, j, h);
        // the right half: instance_feature as it is, 32 float4 per row of the tile
        const int tile0 = blockIdx.x * kRowTile, rows = min(kRowTile, a.n - tile0);
        for (int k = t; k < 32 * rows; k += 256) {
            const size_t r = (size_t)(tile0 + (k >> 5));
            *reinterpret_cast<float4 *>(a.out + r * (2 * kDeformE) + kDeformE + 4 * (k & 31)) = ld4(a.f + r * kDeformE + 4 * (k & 31));
        }
    } else {
        store_rows(so, y, a.out, row0, a.n, l, j, h);
    }
}

// the byte ranges [a, a + na) and [b, b + nb) meet (a null or empty one meets nothing)
static bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

static const char *const kDeformOutputName[GF_DEFORM_OUTPUT_PARAMS] = {"output_proj.weight", "output_proj.bias", "norm.weight", "norm.bias"};

// what every entry point of the back checks of the sizes and the parameter table, under the name `fn` of the one called
static int deform_output_check(const char *fn, int n, int E, int mode, const void *const *params, bool residual)
{
    const char *const *name = kDeformOutputName;
    GF_REFUSE_AS(fn, E == kDeformE, "E = %d: only embed_dims = 128 is supported", E);
    GF_REFUSE_AS(fn, mode == GF_DEFORM_NONE || mode == GF_DEFORM_ADD || mode == GF_DEFORM_CAT, "mode = %d is not GF_DEFORM_NONE / ADD / CAT", mode);
    GF_REFUSE_AS(fn, n >= 0, "n = %d is negative", n);
    GF_REFUSE_AS(fn, params, "null params");
    const float *const *p = reinterpret_cast<const float *const *>(params);
    GF_REFUSE_AS(fn, p[0], "%s is missing", name[0]);
    GF_REFUSE_AS(fn, p[1], "%s is missing", name[1]);
    GF_REFUSE_AS(fn, !p[2] == !p[3], "a half-present pair: %s is null and %s is not", name[p[2] ? 3 : 2], name[p[2] ? 2 : 3]);
    GF_REFUSE_AS(fn, !(p[2] && mode == GF_DEFORM_CAT), "a post norm with mode = %d (GF_DEFORM_CAT): the norm is 128 wide, the row 256", mode);
    GF_REFUSE_AS(fn, !(residual && mode == GF_DEFORM_CAT), "a residual with mode = %d (GF_DEFORM_CAT)", mode);
    for (int i = 0; i < GF_DEFORM_OUTPUT_PARAMS; ++i) GF_REFUSE_AS(fn, !misaligned16(p[i]), "%s is not 16-byte aligned", name[i]);
    return GF_OK;
}
// ... and of the forward's row pointers (gf_deform_output_forward, gf_deform_output_forward_train)
static int deform_output_check_rows(const char *fn, int n, int mode, const float *features, const float *instance_feature,
                                    const float *residual, const float *out)
{
    GF_REFUSE_AS(fn, !misaligned16(features), "features is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(instance_feature), "instance_feature is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(residual), "residual is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(out), "out is not 16-byte aligned");
    if (n == 0) return GF_OK;
    GF_REFUSE_AS(fn, features && out && (mode == GF_DEFORM_NONE || instance_feature), "null pointer");
    const size_t in_bytes = (size_t)n * kDeformE * 4, out_bytes = in_bytes * (mode == GF_DEFORM_CAT ? 2 : 1);
    GF_REFUSE_AS(fn, !overlap(out, out_bytes, features, in_bytes) && !overlap(out, out_bytes, residual, in_bytes) &&
                         !(mode != GF_DEFORM_NONE && overlap(out, out_bytes, instance_feature, in_bytes)),
                     "out aliases an input");
    return GF_OK;
}

}  // namespace gf
