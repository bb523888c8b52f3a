// The training step of the deformable block's dense back: the saving forward (gf_deform.hpp's 128-row output kernel with the
// training arguments) and the backward.  The contract: include/gf_hip.h; the design and the measured numbers: DESIGN.md
// §3.13f.  A translation unit of its own: deform_dense.hip's kernels stay the instruction streams they are.
#include "gf_deform.hpp"
#include "gf_rows_bwd.hpp"

namespace gf {

// ---- the back's backward (gf_deform_output_backward) --------------------------------------------------------
// Three kernels, no atomics, §3.13b's organisation.  (1) The data backward, on the forward's tile and register layout: the post
// norm's backward gives g_s (x^ formed again from the saved row and statistics), grad_features = Wo^T g_y through product_t;
// it writes the per-row outputs, g_s for (2) where it is not grad_out itself, and per tile the sums over its rows of the
// vector gradients.  (2) dWo = g_y^T x per block of kDeformWgRows rows.  (3) One fixed-order sum of the partials into the
// caller's gradient tensors: stored, not accumulated.
constexpr int kDeformWgRows = GF_DEFORM_OUTPUT_WGRAD_ROWS;
static_assert(kDeformWgRows % kRowTile == 0, "a weight-gradient block is whole tiles");
// a tile's vector partials, in floats: dbo | d(norm weight) | d(norm bias)
constexpr int kDoVpBo = 0, kDoVpG = 128, kDoVpBeta = 256, kDoVpLen = 384;
constexpr size_t kDoWpLen = (size_t)kDeformE * kDeformE;

struct DeformOutputBwdArgs {
    const float *grad_out, *w, *gam, *ysave, *stat;
    float *grad_x, *grad_inst, *grad_res, *gs, *vpart;
    int n, mode;
};

__global__ __launch_bounds__(256) void gf_deform_output_bwd_kernel(DeformOutputBwdArgs a)
{
    __shared__ float s_t[2][32 * kRowTPitch];
    __shared__ float s_part[4][128];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = blockIdx.x * kRowTile + wv * 32;
    const bool valid = row0 + j < a.n;
    const size_t row = (size_t)min(row0 + j, a.n - 1);   // a row past n walks row n - 1 with a zero gradient and stores nothing
    const size_t gpitch = a.mode == GF_DEFORM_CAT ? 2 * kDeformE : kDeformE;
    float *vp = a.vpart + (size_t)blockIdx.x * kDoVpLen;

    // g = grad_out (its left half with "cat"), then g_s: the post norm's backward
    f32x16 g[4];
    load_row_or_zero(g, a.grad_out + row * gpitch, valid, h);
    if (a.gam) {
        const float2 ms = *reinterpret_cast<const float2 *>(a.stat + 2 * row);
        f32x16 nh[4];
        load_row(nh, a.ysave + row * kDeformE, h);
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) nh[b][r] = (nh[b][r] - ms.x) * ms.y;
        tile_sum<4>([&](int b, int r) { return g[b][r] * nh[b][r]; }, valid, s_part, vp + kDoVpG, t, wv, j, h);
        tile_sum<4>([&](int b, int r) { return g[b][r]; }, valid, s_part, vp + kDoVpBeta, t, wv, j, h);
        ln_bwd_rows(g, nh, a.gam, ms.y, h);
        if (valid) store_row_regs(a.gs + row * kDeformE, g, h);
    }
    if (valid) {
        if (a.grad_res) store_row_regs(a.grad_res + row * kDeformE, g, h);
        if (a.grad_inst && a.mode == GF_DEFORM_ADD) store_row_regs(a.grad_inst + row * kDeformE, g, h);
    }
    if (a.grad_inst && a.mode == GF_DEFORM_CAT) {   // the right half of grad_out as it is, 32 float4 per row of the tile
        const int tile0 = blockIdx.x * kRowTile, rows = min(kRowTile, a.n - tile0);
        for (int k = t; k < 32 * rows; k += 256) {
            const size_t r = (size_t)(tile0 + (k >> 5));
            *reinterpret_cast<float4 *>(a.grad_inst + r * kDeformE + 4 * (k & 31)) = ld4(a.grad_out + r * (2 * kDeformE) + kDeformE + 4 * (k & 31));
        }
    }
    tile_sum<4>([&](int b, int r) { return g[b][r]; }, valid, s_part, vp + kDoVpBo, t, wv, j, h);

    f32x16 acc[4];
    zero_rows(acc);
    product_t<4, false>(acc, g, a.w, kDeformE, 0, s_t[0], s_t[1], t, j, h);
    if (valid) store_row_regs(a.grad_x + row * kDeformE, acc, h);
}

struct DeformOutputWgArgs {
    const float *left;     // g_y [n][ldl]
    const float *x;        // features [n][128]
    float *wpart;          // [blocks][128 x 128]
    size_t ldl;
    int n;
};

// A row block's dWo = g_y^T x, A = g_y[row][o] and B = x[row][k], two rows a step; a wave owns 32 rows o (wgrad_rows)
__global__ __launch_bounds__(256) void gf_deform_output_wgrad_kernel(DeformOutputWgArgs a)
{
    const int blk = blockIdx.x;
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int r0 = blk * kDeformWgRows, r1 = min(a.n, r0 + kDeformWgRows);
    const float gv[4] = {1.f, 1.f, 1.f, 1.f}, ev[4] = {0.f, 0.f, 0.f, 0.f};
    f32x16 acc[4];
    zero_rows(acc);
    wgrad_rows<kWgAsIs>(acc, a.left + 32 * wv + j, a.ldl, 0, a.x + j, nullptr, kDeformE, 0, nullptr, gv, ev, r0, r1, r1, h);
    wgrad_store(a.wpart + (size_t)blk * kDoWpLen, kDeformE, [&](int cb, int r) { return acc[cb][r]; }, wv, j, h);
}

static const size_t kDeformOutputBytes[GF_DEFORM_OUTPUT_PARAMS] = {kDoWpLen * 4, kDeformE * 4, kDeformE * 4, kDeformE * 4};

// The training step's two regions, sized and carved by one function each (a null base: sizes only).
struct DeformOutputSaved { float *ysave, *stat; size_t bytes; };
static DeformOutputSaved deform_output_carve_saved(void *base, int n, bool with_norm)
{
    Carver c(base);
    DeformOutputSaved s;
    s.ysave = c.take<float>(with_norm ? (size_t)n * kDeformE : 0);
    s.stat = c.take<float>(with_norm ? (size_t)n * 2 : 0);
    s.bytes = c.bytes();
    return s;
}
struct DeformOutputWork { float *gs, *vpart, *wpart; int tiles, blocks; size_t bytes; };
static DeformOutputWork deform_output_carve_work(void *base, int n, bool with_norm)
{
    Carver c(base);
    DeformOutputWork w;
    w.tiles = (n + kRowTile - 1) / kRowTile;
    w.blocks = (n + kDeformWgRows - 1) / kDeformWgRows;
    w.gs = c.take<float>(with_norm ? (size_t)n * kDeformE : 0);     // without a norm g_s is grad_out itself
    w.vpart = c.take<float>((size_t)w.tiles * kDoVpLen);
    w.wpart = c.take<float>((size_t)w.blocks * kDoWpLen);
    w.bytes = c.bytes();
    return w;
}

}  // namespace gf

extern "C" int gf_deform_output_train_sizes(int n, int E, int mode, int with_norm, size_t *saved_bytes, size_t *workspace_bytes)
{
    using namespace gf;
    const char *fn = __func__;
    GF_REFUSE_AS(fn, E == kDeformE, "E = %d: only embed_dims = 128 is supported", E);
    GF_REFUSE_AS(fn, mode == GF_DEFORM_NONE || mode == GF_DEFORM_ADD || mode == GF_DEFORM_CAT, "mode = %d is not GF_DEFORM_NONE / ADD / CAT", mode);
    GF_REFUSE_AS(fn, !(with_norm && mode == GF_DEFORM_CAT), "a post norm with mode = %d (GF_DEFORM_CAT): the norm is 128 wide, the row 256", mode);
    GF_REFUSE_AS(fn, n >= 0, "n = %d is negative", n);
    GF_REFUSE_AS(fn, saved_bytes && workspace_bytes, "null pointer");
    *saved_bytes = deform_output_carve_saved(nullptr, n, with_norm != 0).bytes;
    *workspace_bytes = deform_output_carve_work(nullptr, n, with_norm != 0).bytes;
    return GF_OK;
}

extern "C" int gf_deform_output_forward_train(int n, int E, int mode, const float *features, const float *instance_feature,
                                              const void *const *params, const float *residual, float *out, void *saved,
                                              size_t saved_bytes, void *stream_)
{
    using namespace gf;
    const char *fn = __func__;
    if (int rc = deform_output_check(fn, n, E, mode, params, residual != nullptr)) return rc;
    if (int rc = deform_output_check_rows(fn, n, mode, features, instance_feature, residual, out)) return rc;
    GF_REFUSE_AS(fn, !misaligned16(saved), "saved is not 16-byte aligned");
    if (n == 0) return GF_OK;
    const float *const *p = reinterpret_cast<const float *const *>(params);
    // without a post norm nothing is saved: the forward's own call
    if (!p[2]) return gf_deform_output_forward(n, E, mode, features, instance_feature, params, residual, out, stream_);
    GF_REFUSE_AS(fn, saved, "saved is null");
    const DeformOutputSaved sv = deform_output_carve_saved(saved, n, true);
    GF_CHECK_WORKSPACE_AS(fn, "saved", saved_bytes, sv.bytes);
    const size_t in_bytes = (size_t)n * kDeformE * 4;
    GF_REFUSE_AS(fn, !overlap(saved, sv.bytes, out, in_bytes), "saved aliases out");
    GF_REFUSE_AS(fn, !overlap(saved, sv.bytes, features, in_bytes) && !overlap(saved, sv.bytes, residual, in_bytes) &&
                         !(mode != GF_DEFORM_NONE && overlap(saved, sv.bytes, instance_feature, in_bytes)),
                     "saved aliases an input");
    DeformOutputTrainArgs a{};
    static_cast<DeformOutputArgs &>(a) = DeformOutputArgs{features, mode == GF_DEFORM_NONE ? nullptr : instance_feature, residual, p[0], p[1], p[2], p[3], out, n, mode};
    a.ysave = sv.ysave; a.stat = sv.stat;
    // the tile kernel at every n: the 32-row kernel's bits (§3.13e), one saving build
    hipLaunchKernelGGL(gf_deform_output_kernel<DeformOutputTrainArgs>, dim3((n + kRowTile - 1) / kRowTile), dim3(256), 0, (hipStream_t)stream_, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_deform_output_backward(int n, int E, int mode, const float *features, const void *const *params, const void *saved,
                                         const float *grad_out, float *grad_features, float *grad_instance, float *grad_residual,
                                         void *const *grad_params, void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace gf;
    const char *fn = __func__;
    if (int rc = deform_output_check(fn, n, E, mode, params, false)) return rc;
    const float *const *p = reinterpret_cast<const float *const *>(params);
    const bool with_norm = p[2] != nullptr;
    GF_REFUSE_AS(fn, !(grad_instance && mode == GF_DEFORM_NONE), "grad_instance with mode = %d (GF_DEFORM_NONE): instance_feature is not part of the op", mode);
    GF_REFUSE_AS(fn, !(grad_residual && mode == GF_DEFORM_CAT), "grad_residual with mode = %d (GF_DEFORM_CAT)", mode);
    GF_REFUSE_AS(fn, grad_params, "null grad_params");
    float *const *gp = reinterpret_cast<float *const *>(grad_params);
    for (int i = 0; i < GF_DEFORM_OUTPUT_PARAMS; ++i) {
        GF_REFUSE_AS(fn, !gp[i] || p[i], "a gradient for %s, which is absent", kDeformOutputName[i]);
        GF_REFUSE_AS(fn, !misaligned16(gp[i]), "the gradient of %s is not 16-byte aligned", kDeformOutputName[i]);
    }
    GF_REFUSE_AS(fn, !misaligned16(features), "features is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(grad_out), "grad_out is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(grad_features), "grad_features is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(grad_instance), "grad_instance is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(grad_residual), "grad_residual is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(saved), "saved is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(workspace), "workspace is not 16-byte aligned");
    const DeformOutputSaved sv = deform_output_carve_saved(n > 0 && with_norm ? const_cast<void *>(saved) : nullptr, n, with_norm);
    const DeformOutputWork ws = deform_output_carve_work(n > 0 ? workspace : nullptr, n, with_norm);
    const size_t in_bytes = (size_t)n * kDeformE * 4, go_bytes = in_bytes * (mode == GF_DEFORM_CAT ? 2 : 1);
    if (n > 0) {
        GF_REFUSE_AS(fn, features && grad_out && grad_features, "null pointer");
        GF_REFUSE_AS(fn, !with_norm || saved, "saved is null");
        GF_REFUSE_AS(fn, workspace, "workspace is null");
        GF_CHECK_WORKSPACE_AS(fn, "workspace", workspace_bytes, ws.bytes);
    }
    // every output against every input, the two regions and the outputs before it
    struct Range { const void *p; size_t bytes; const char *what; };
    const Range ins[] = {{features, in_bytes, "an input"}, {grad_out, go_bytes, "an input"}, {p[0], kDeformOutputBytes[0], "an input"},
                         {p[1], kDeformOutputBytes[1], "an input"}, {p[2], kDeformOutputBytes[2], "an input"}, {p[3], kDeformOutputBytes[3], "an input"},
                         {saved, sv.bytes, "the saved region"}, {workspace, n > 0 ? ws.bytes : 0, "the workspace"}};
    const Range outs[] = {{grad_features, in_bytes, "grad_features"}, {grad_instance, in_bytes, "grad_instance"},
                          {grad_residual, in_bytes, "grad_residual"}, {gp[0], kDeformOutputBytes[0], "the gradient of output_proj.weight"},
                          {gp[1], kDeformOutputBytes[1], "the gradient of output_proj.bias"}, {gp[2], kDeformOutputBytes[2], "the gradient of norm.weight"},
                          {gp[3], kDeformOutputBytes[3], "the gradient of norm.bias"}};
    for (size_t o = 0; o < sizeof(outs) / sizeof(outs[0]); ++o) {
        for (const Range &in : ins) GF_REFUSE_AS(fn, !overlap(outs[o].p, outs[o].bytes, in.p, in.bytes), "%s aliases %s", outs[o].what, in.what);
        for (size_t q = 0; q < o; ++q)
            GF_REFUSE_AS(fn, !overlap(outs[o].p, outs[o].bytes, outs[q].p, outs[q].bytes), "%s aliases %s", outs[o].what, outs[q].what);
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (n > 0) {
        DeformOutputBwdArgs b{grad_out, p[0], p[2], sv.ysave, sv.stat, grad_features, grad_instance, grad_residual, ws.gs, ws.vpart, n, mode};
        hipLaunchKernelGGL(gf_deform_output_bwd_kernel, dim3(ws.tiles), dim3(256), 0, stream, b);
        GF_CHECK_LAUNCH();
        if (gp[0]) {
            DeformOutputWgArgs g{with_norm ? ws.gs : grad_out, features, ws.wpart, with_norm ? (size_t)kDeformE : go_bytes / 4 / (size_t)n, n};
            hipLaunchKernelGGL(gf_deform_output_wgrad_kernel, dim3(ws.blocks), dim3(256), 0, stream, g);
            GF_CHECK_LAUNCH();
        }
    }
    // n == 0: no partials, the sums store zeros
    RowsSumArgs<GF_DEFORM_OUTPUT_PARAMS> sa{};   // float sums, a thread per element
    int nj = 0;
    if (gp[0]) sa.job[nj++] = RowsSumJob{n > 0 ? ws.wpart : nullptr, gp[0], kDoWpLen, n > 0 ? ws.blocks : 0, (int)kDoWpLen, 0, 1};
    auto vec = [&](int i, int at) {
        if (gp[i]) sa.job[nj++] = RowsSumJob{n > 0 ? ws.vpart + at : nullptr, gp[i], (size_t)kDoVpLen, n > 0 ? ws.tiles : 0, kDeformE, 0, 1};
    };
    vec(1, kDoVpBo);
    vec(2, kDoVpG);
    vec(3, kDoVpBeta);
    if (nj > 0) {
        hipLaunchKernelGGL((rows_sum_kernel<float, GF_DEFORM_OUTPUT_PARAMS>), dim3(gp[0] ? (int)kDoWpLen / 256 : 1, nj), dim3(256), 0, stream, sa);
        GF_CHECK_LAUNCH();
    }
    return GF_OK;
}

