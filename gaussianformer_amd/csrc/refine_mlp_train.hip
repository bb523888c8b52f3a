// The refinement modules' training step, backward (gf_refine_mlp_backward) and the size query.  The saving forward is
// refine_mlp.hip's kernel with SAVE.  The contract: include/gf_hip.h; the design and the measured numbers: DESIGN.md §3.12c.
//
// Four kinds of launch, no atomics, §3.13b's organisation.  (0) The tail's backward on (saved o, anchor, the output gradients):
// refine.hip's kernel through refine_launch_backward; it gives grad_anchor and go, the gradient of o.  (1) The MLP's data backward
// in the forward's tile and register layout, stages in reverse: Scale and the [D, 128] Linear (the reduction over D padded with
// zeros to 64), then twice LayerNorm backward, ReLU mask, dX^T = W^T dZ^T, ReLU mask, dX^T = W^T dZ^T.  The ReLU masks come
// off the saved post-ReLU rows (r > 0, or a NaN: torch's threshold passes that gradient on).  It writes grad_x, each stage's dz
// rows for (2), and per tile the sums over its rows of the vector gradients.  (2) The weight gradients dW_s = dz_s^T x_s per
// block of kRmWgRows rows, x_s formed again from what was saved as the forward applies it.  (3) One fixed-order sum of the
// partials into the caller's 15 gradient tensors: stored, not accumulated.
#include "gf_refine.hpp"
#include "gf_rows_bwd.hpp"

namespace gf {

constexpr int kRmWgRows = GF_REFINE_MLP_WGRAD_ROWS;
constexpr int kRmChunkRows = GF_REFINE_MLP_CHUNK_ROWS;
constexpr int kRmWgFlush = 64;     // rows of one fp32 accumulation chain of the weight-gradient kernel
static_assert(kRmChunkRows % kRmWgRows == 0 && kRmWgRows % kRowTile == 0, "a chunk is whole weight-gradient blocks, a block whole tiles");

// a tile's vector partials, in floats: db0 | db2 | db5 | db7 | d(LN4 weight) | d(LN4 bias) | d(LN9 weight) | d(LN9 bias) |
// db10 (64) | dscale (64)
constexpr int kRmVBias = 0, kRmVLn = 4 * kRmE, kRmVB10 = 8 * kRmE, kRmVScale = kRmVB10 + kRmYPitch, kRmVLen = kRmVScale + kRmYPitch;
// a row block's matrix partials: the four square dW [128, 128], then dW10 [64, 128] (rows from D on: zero)
constexpr size_t kRmWLen = (size_t)4 * kRmE * kRmE + (size_t)kRmYPitch * kRmE;

struct RmBwdArgs {
    const float *go;                 // [n, D] the gradient of o (the tail's backward wrote it)
    const float *w[5];               // layers.0, .2, .5, .7 [128, 128], layers.10 [D, 128]
    const float *ln_g[2];            // layers.4.weight, layers.9.weight
    const float *scale;              // [D]
    const float *rows, *stat, *y;    // the saved forward (RefineMlpSaved)
    float *dz;                       // [4][crows][128] the chunk's dz rows of the square stages
    float *dz4;                      // [crows][64] and of the last Linear (zero from D on)
    float *grad_x;                   // [n, 128]
    float *vpart;                    // [tiles][kRmVLen], all chunks'
    int n, D, base, crows;           // base: the chunk's first row
};

__global__ __launch_bounds__(256) void gf_refine_mlp_bwd_kernel(RmBwdArgs a)
{
    __shared__ float4 s_w[2][32 * kRowTPitch / 4];
    __shared__ float s_part[4][kRmE];
    float *buf0 = reinterpret_cast<float *>(s_w[0]), *buf1 = reinterpret_cast<float *>(s_w[1]);
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int n = a.n, D = a.D;
    const int row0 = a.base + blockIdx.x * kRowTile + wv * 32;
    const bool valid = row0 + j < n;
    const size_t row = (size_t)min(row0 + j, n - 1);     // a row past n walks row n - 1 with a zero gradient and stores nothing
    const size_t lrow = row - a.base;                    // its place in the chunk
    float *vp = a.vpart + (size_t)(a.base / kRowTile + blockIdx.x) * kRmVLen;

    f32x16 g[4], acc[4];
    // Scale and layers.10: with y the value before Scale, do = go; dscale = sum go y; dz4 = go scale; db10 = sum dz4.  Features
    // from D on carry zeros
    {
        f32x16 gy[2], yv[2];
        load_row(yv, a.y + row * kRmYPitch, h);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * b + 8 * (r >> 2) + 4 * h + (r & 3), fc = min(f, D - 1);
                const float gv = a.go[row * D + fc], sc = a.scale[fc];
                const bool in = valid && f < D;
                yv[b][r] = in ? gv * yv[b][r] : 0.f;
                gy[b][r] = in ? gv * sc : 0.f;
            }
        tile_sum<2>([&](int b, int r) { return yv[b][r]; }, valid, s_part, vp + kRmVScale, t, wv, j, h);
        tile_sum<2>([&](int b, int r) { return gy[b][r]; }, valid, s_part, vp + kRmVB10, t, wv, j, h);
        if (valid) store_row_regs(a.dz4 + lrow * kRmYPitch, gy, h);
        zero_rows(acc);
        product_t<2, true>(acc, gy, a.w[4], kRmE, D, buf0, buf1, t, j, h);
    }

    // the four square stages, last first: acc holds the gradient of the stage's output (behind the LayerNorm where it has one)
#pragma unroll 1
    for (int q = 3; q >= 0; --q) {
        // the stage's saved post-ReLU row, and where it passes a gradient
        load_row(g, a.rows + ((size_t)q * n + row) * kRmE, h);
        uint64_t live = 0;       // bit 16 b + r
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) live |= (uint64_t)(!(g[b][r] <= 0.f)) << (16 * b + r);
        if (q & 1) {
            // the LayerNorm's backward: r^ = (r - mean) rstd, dn = acc gamma, dr = rstd (dn - mean(dn) - r^ mean(dn r^))
            const float2 ms = *reinterpret_cast<const float2 *>(a.stat + ((size_t)(q >> 1) * n + row) * 2);
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) g[b][r] = (g[b][r] - ms.x) * ms.y;
            float *vln = vp + kRmVLn + 2 * kRmE * (q >> 1);
            tile_sum<4>([&](int b, int r) { return acc[b][r] * g[b][r]; }, valid, s_part, vln, t, wv, j, h);
            tile_sum<4>([&](int b, int r) { return acc[b][r]; }, valid, s_part, vln + kRmE, t, wv, j, h);
            ln_bwd_rows(acc, g, a.ln_g[q >> 1], ms.y, h);
        }
        // dz = the ReLU's backward; a row past n carries zeros
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) g[b][r] = valid && ((live >> (16 * b + r)) & 1u) ? acc[b][r] : 0.f;
        if (valid) store_row_regs(a.dz + ((size_t)q * a.crows + lrow) * kRmE, g, h);
        tile_sum<4>([&](int b, int r) { return g[b][r]; }, valid, s_part, vp + kRmVBias + kRmE * q, t, wv, j, h);
        zero_rows(acc);
        product_t<4, false>(acc, g, a.w[q], kRmE, 0, buf0, buf1, t, j, h);
    }
    if (valid) store_row_regs(a.grad_x + row * kRmE, acc, h);
}

struct RmWgArgs {
    const float *feat, *embed;       // x_0 = instance_feature + anchor_embed, formed again
    const float *rows, *stat;        // the saved forward
    const float *ln_g[2], *ln_b[2];
    const float *dz, *dz4;           // the chunk's rows
    float *wpart;                    // [blocks][kRmWLen]
    int n, base, crows;
};

// One job of a row block: dW_s = dz_s^T x_s over the block's rows, A = dz_s[row][o] and B = x_s[row][k], two rows a step (lanes
// 0-31 one, lanes 32-63 the other), loaded from the row-major arrays as they lie; a wave owns 32 rows o.  x_s: s = 0 the sum of
// the two inputs, s = 1, 3 the saved post-ReLU rows 0, 2, s = 2, 4 the LayerNorm of the saved rows 1, 3 from its saved
// (mean, rstd), in the saving forward's expression.  Job 4 (layers.10) has 64 rows o: waves 2 and 3 have nothing to do.  A lane
// beyond the block's rows supplies 0 (a select) and loads the block's last row.  (KIND: wgrad_rows' -- kWgSum the sum of the two
// inputs, kWgAsIs saved rows as they are, kWgNorm their LayerNorm)
template <int KIND>
__device__ __forceinline__ void rm_wgrad_job(const RmWgArgs &a, int s)
{
    const int blk = a.base / kRmWgRows + blockIdx.x;
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    if (s == 4 && wv >= 2) return;
    const int n = a.n, r0 = blk * kRmWgRows, r1 = min(n, r0 + kRmWgRows);
    const float *left = s < 4 ? a.dz + (size_t)s * a.crows * kRmE : a.dz4;
    const size_t ldl = s < 4 ? kRmE : kRmYPitch;
    left += 32 * wv + j;
    const float *right = (KIND == kWgSum ? a.feat : a.rows + (size_t)(s - 1) * n * kRmE) + j, *right2 = a.embed + j;
    const float *stat = a.stat + (size_t)(s == 4 ? 1 : 0) * n * 2;
    float gv[4], ev[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        gv[cb] = KIND == kWgNorm ? a.ln_g[s == 4][32 * cb + j] : 1.f;
        ev[cb] = KIND == kWgNorm ? a.ln_b[s == 4][32 * cb + j] : 0.f;
    }
    // Two levels: an fp32 MFMA chain over kRmWgFlush rows, then the chains of the block join in double and the block's partial is
    // rounded once.  One chain over all 512 rows left the last Linear's gradients at n = 33 350 at 2.5 times the error of
    // torch's product (the cotangent of the tests' scalar nearly cancels over the rows, so the sum's own rounding shows)
    f32x16 acc[4];
    double outer[4][16];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) outer[cb][r] = 0.0;
#pragma unroll 1
    for (int rb = r0; rb < r1; rb += kRmWgFlush) {
        zero_rows(acc);
        wgrad_rows<KIND>(acc, left, ldl, a.base, right, right2, kRmE, 0, stat, gv, ev, rb, min(r1, rb + kRmWgFlush), r1, h);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) outer[cb][r] += (double)acc[cb][r];
    }
    wgrad_store(a.wpart + (size_t)blk * kRmWLen + (size_t)s * kRmE * kRmE, kRmE, [&](int cb, int r) { return (float)outer[cb][r]; }, wv, j, h);
}

__global__ __launch_bounds__(256, 2) void gf_refine_mlp_wgrad_kernel(RmWgArgs a)
{
    const int s = blockIdx.y;
    if (s == 0) rm_wgrad_job<kWgSum>(a, s);
    else if (s & 1) rm_wgrad_job<kWgAsIs>(a, s);
    else rm_wgrad_job<kWgNorm>(a, s);
}

// The backward's scratch, sized and carved by one function (a null base: the size only)
struct RmWork { float *go, *dz, *dz4, *vpart, *wpart; int tiles, blocks, crows; size_t bytes; };
static RmWork rm_carve_work(void *base, int n, int D)
{
    Carver c(base);
    RmWork w;
    w.tiles = (n + kRowTile - 1) / kRowTile;
    w.blocks = (n + kRmWgRows - 1) / kRmWgRows;
    w.crows = n < kRmChunkRows ? n : kRmChunkRows;
    w.go = c.take<float>((size_t)n * D);     // the gradient of o, where the caller does not ask for it
    w.dz = c.take<float>((size_t)4 * w.crows * kRmE);
    w.dz4 = c.take<float>((size_t)w.crows * kRmYPitch);
    w.vpart = c.take<float>((size_t)w.tiles * kRmVLen);
    w.wpart = c.take<float>((size_t)w.blocks * kRmWLen);
    w.bytes = c.bytes();
    return w;
}

}  // namespace gf

extern "C" int gf_refine_mlp_train_sizes(int n, int D, int Da, size_t *saved_bytes, size_t *workspace_bytes)
{
    using namespace gf;
    const char *fn = __func__;
    GF_REFUSE_AS(fn, n >= 0, "n = %d is negative", n);
    GF_REFUSE_AS(fn, D >= 10 && D <= 10 + 1 + kRefMaxS, "D = %d is not in 10 .. %d", D, 10 + 1 + kRefMaxS);
    GF_REFUSE_AS(fn, Da >= 0, "Da = %d is negative", Da);
    GF_REFUSE_AS(fn, saved_bytes && workspace_bytes, "null pointer");
    *saved_bytes = refine_mlp_carve_saved(nullptr, n, D).bytes;
    *workspace_bytes = rm_carve_work(nullptr, n, D).bytes;
    return GF_OK;
}

extern "C" int gf_refine_mlp_backward(int n, int E, int D, int Da, int version, int flags, int R, int S, const double *consts,
                                      const float *instance_feature, const float *anchor_embed, const float *anchor,
                                      const void *const *params, const void *saved, const float *grad_anchor_out, const float *grad_means,
                                      const float *grad_scales, const float *grad_rotations, const float *grad_opacities,
                                      const float *grad_semantics, const float *grad_original_means, const float *grad_delta_means,
                                      float *grad_x, float *grad_anchor, float *grad_mlp_out, void *const *grad_params, void *workspace,
                                      size_t workspace_bytes, void *stream_)
{
    using namespace gf;
    const char *fn = __func__;
    RefineArgs r{};
    if (int rc = refine_fill_args(r, fn, n, D, Da, version, flags, R, S, consts)) return rc;
    GF_REFUSE_AS(fn, E == kRmE, "E = %d: only embed_dims = 128 is supported", E);
    GF_REFUSE_AS(fn, grad_params, "null grad_params");
    float *const *gp = reinterpret_cast<float *const *>(grad_params);
    for (int i = 0; i < GF_REFINE_MLP_PARAMS; ++i) GF_REFUSE_AS(fn, gp[i], "grad_params[%d] (the gradient of %s) is null", i, kRmName[i]);
    hipStream_t stream = (hipStream_t)stream_;
    const RefineMlpSaved sv = refine_mlp_carve_saved(n > 0 ? const_cast<void *>(saved) : nullptr, n, D);
    const RmWork ws = rm_carve_work(n > 0 ? workspace : nullptr, n, D);
    if (n > 0) {
        if (int rc = refine_mlp_check_inputs(fn, params, instance_feature, anchor_embed, anchor)) return rc;
        GF_REFUSE_AS(fn, saved, "saved is null");
        GF_REFUSE_AS(fn, !misaligned16(saved), "saved = %p is not 16-byte aligned", saved);
        GF_REFUSE_AS(fn, workspace, "workspace is null");
        GF_REFUSE_AS(fn, !misaligned16(workspace), "workspace = %p is not 16-byte aligned", workspace);
        GF_REFUSE_AS(fn, grad_x, "grad_x is null");
        GF_REFUSE_AS(fn, !misaligned16(grad_x), "grad_x = %p is not 16-byte aligned", (const void *)grad_x);
        GF_REFUSE_AS(fn, grad_anchor, "grad_anchor is null");
        GF_CHECK_WORKSPACE_AS(fn, "workspace", workspace_bytes, ws.bytes);
        const float *const *p = reinterpret_cast<const float *const *>(params);

        // (0) the tail
        float *go = grad_mlp_out ? grad_mlp_out : ws.go;
        r.output = sv.o; r.anchor = anchor;
        r.g_anchor_out = grad_anchor_out; r.g_means = grad_means; r.g_scales = grad_scales; r.g_rotations = grad_rotations;
        r.g_opacities = grad_opacities; r.g_semantics = grad_semantics; r.g_original = grad_original_means; r.g_delta = grad_delta_means;
        r.grad_output = go; r.grad_anchor = grad_anchor;
        if (int rc = refine_launch_backward(fn, r, version, stream)) return rc;

        RmBwdArgs b{};
        b.go = go;
        const int wi[5] = {0, 2, 6, 8, 12};
        for (int i = 0; i < 5; ++i) b.w[i] = p[wi[i]];
        b.ln_g[0] = p[4]; b.ln_g[1] = p[10]; b.scale = p[14];
        b.rows = sv.rows; b.stat = sv.stat; b.y = sv.y;
        b.dz = ws.dz; b.dz4 = ws.dz4; b.grad_x = grad_x; b.vpart = ws.vpart;
        b.n = n; b.D = D; b.crows = ws.crows;
        RmWgArgs g{};
        g.feat = instance_feature; g.embed = anchor_embed; g.rows = sv.rows; g.stat = sv.stat;
        g.ln_g[0] = p[4]; g.ln_g[1] = p[10]; g.ln_b[0] = p[5]; g.ln_b[1] = p[11];
        g.dz = ws.dz; g.dz4 = ws.dz4; g.wpart = ws.wpart;
        g.n = n; g.crows = ws.crows;
        for (int base = 0; base < n; base += kRmChunkRows) {   // the next chunk's data backward overwrites the rows behind this one's wgrad
            const int rows = n - base < kRmChunkRows ? n - base : kRmChunkRows;
            b.base = g.base = base;
            hipLaunchKernelGGL(gf_refine_mlp_bwd_kernel, dim3((rows + kRowTile - 1) / kRowTile), dim3(256), 0, stream, b);
            GF_CHECK_LAUNCH();
            hipLaunchKernelGGL(gf_refine_mlp_wgrad_kernel, dim3((rows + kRmWgRows - 1) / kRmWgRows, 5), dim3(256), 0, stream, g);
            GF_CHECK_LAUNCH();
        }
    }
    // (3) sums in double, rounded once (the partials are fp32 sums over 128 or 512 rows; at 144 000 rows there are 1 125 or 282
    // of them): the matrices -- many elements, few partials -- a thread per element, the vectors -- few elements, a partial per
    // tile -- kRowsSumSlots threads per element, the two-level sum §3.13b asked for.  n == 0: no partials, the sums store zeros
    RowsSumArgs<GF_REFINE_MLP_PARAMS> sa{};
    auto vec = [&](int i, int at, int len) {
        sa.job[i] = RowsSumJob{n > 0 ? ws.vpart + at : nullptr, gp[i], (size_t)kRmVLen, n > 0 ? ws.tiles : 0, len, 0, kRowsSumSlots};
    };
    auto mat = [&](int i, int s, int len) {
        sa.job[i] = RowsSumJob{n > 0 ? ws.wpart + (size_t)s * kRmE * kRmE : nullptr, gp[i], kRmWLen, n > 0 ? ws.blocks : 0, len, 0, 1};
    };
    mat(0, 0, kRmE * kRmE);   vec(1, kRmVBias, kRmE);
    mat(2, 1, kRmE * kRmE);   vec(3, kRmVBias + kRmE, kRmE);
    vec(4, kRmVLn, kRmE);     vec(5, kRmVLn + kRmE, kRmE);
    mat(6, 2, kRmE * kRmE);   vec(7, kRmVBias + 2 * kRmE, kRmE);
    mat(8, 3, kRmE * kRmE);   vec(9, kRmVBias + 3 * kRmE, kRmE);
    vec(10, kRmVLn + 2 * kRmE, kRmE); vec(11, kRmVLn + 3 * kRmE, kRmE);
    mat(12, 4, D * kRmE);     vec(13, kRmVB10, D);
    vec(14, kRmVScale, D);
    hipLaunchKernelGGL((rows_sum_kernel<double, GF_REFINE_MLP_PARAMS>), dim3(kRmE * kRmE / 256, GF_REFINE_MLP_PARAMS), dim3(256), 0, stream, sa);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
