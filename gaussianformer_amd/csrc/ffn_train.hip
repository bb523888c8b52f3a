// The feed-forward block's training step: the saving forward (gf_ffn.hpp's tile kernel with TRAIN) and the backward.  The
// contract: include/gf_hip.h; the design and the measured numbers: DESIGN.md §3.13d.
#include <cmath>

#include "gf_ffn.hpp"
#include "gf_rows_bwd.hpp"

namespace gf {

// ---- the backward (gf_ffn_backward) ------------------------------------------------------------------------
// Three kernels, no atomics, §3.13b's organisation.  (1) The data backward: the forward's tile and register layout.  The post
// norm's backward gives dy and da.  Pass 1 walks the four hidden slices: h_s is formed again from u by the forward's own chunk
// chain (so h <= 0 is the forward's decision bit for bit), dh_s = W2[:, s]^T da, dz_s = dropout and ReLU backward of it.
// Pass 2: du = Wid^T dy + sum_s W1_s^T dz_s, then the pre norm's backward.  The transposed products read the weight along its
// rows from LDS (product_t).  It writes grad_x, grad_residual, the chunk's h', dz, da and dy rows for (2), and per tile
// the sums over its rows of the vector gradients.  (2) The weight gradients dW1 = dz^T u, dW2 = da^T h', dWid = dy^T u per block of
// kFfnWgRows rows, u recomputed from x and the saved statistics.  (3) One fixed-order sum of the partials into the caller's
// gradient tensors: stored, not accumulated.
constexpr int kFfnWgRows = GF_FFN_WGRAD_ROWS;
constexpr int kFfnChunkRows = GF_FFN_CHUNK_ROWS;
static_assert(kFfnChunkRows % kFfnWgRows == 0 && kFfnWgRows % kRowTile == 0, "a chunk is whole weight-gradient blocks, a block whole tiles");

// a tile's vector partials, in floats: db1 | db2 | dbid | d(post weight) | d(post bias) | d(pre weight) | d(pre bias)
constexpr int kVpB1 = 0, kVpB2 = kFfnF, kVpBid = kVpB2 + 128, kVpPostG = kVpBid + 128, kVpPostB = kVpPostG + 128, kVpPre = kVpPostB + 128;
constexpr int ffn_vpart_len(int cin) { return kVpPre + 2 * cin; }
// a row block's matrix partials: dW1 [512, Cin] | dW2 [128, 512] | dWid [128, Cin]
constexpr size_t ffn_wpart_len(int cin) { return (size_t)kFfnF * cin + (size_t)kFfnE * kFfnF + (size_t)kFfnE * cin; }

struct FfnBwdArgs {
    const float *x, *grad_out;
    float *grad_x, *grad_res;
    const float *pre_g, *pre_b, *w1, *b1, *w2, *wid, *post_g;
    const unsigned char *keep_hidden, *keep_out;
    float scale_hidden, scale_out;
    const float *ysave, *stat_pre, *stat_post;
    float *hrows, *dz;           // [crows][512] the chunk's h' and dz rows
    float *da, *dy;              // [crows][128]
    float *vpart;                // [tiles][ffn_vpart_len(Cin)], all chunks'
    int n, base;                 // base: the chunk's first row
};

template <int CIN>
__global__ __launch_bounds__(256) void gf_ffn_bwd_kernel(FfnBwdArgs a)
{
    constexpr int NB = CIN / 32;
    constexpr int kFwdBuf = 128 * kRowPitch4 * 4, kTBuf = 32 * kRowTPitch;    // floats: a forward chunk, a transposed chunk
    constexpr int kBuf = kFwdBuf > kTBuf ? kFwdBuf : kTBuf;
    __shared__ float4 s_w[2][kBuf / 4];
    __shared__ float s_part[4][128];
    float *buf0 = reinterpret_cast<float *>(s_w[0]), *buf1 = reinterpret_cast<float *>(s_w[1]);
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = a.base + blockIdx.x * kRowTile + wv * 32;
    const bool valid = row0 + j < a.n;
    const size_t row = (size_t)min(row0 + j, a.n - 1);   // a row past n walks row n - 1 with a zero gradient and stores nothing
    const size_t lrow = row - a.base;                    // its place in the chunk
    float *vp = a.vpart + (size_t)(a.base / kRowTile + blockIdx.x) * ffn_vpart_len(CIN);

    // g = grad_out, then dy: the post norm's backward
    //     y^ = (y - mean) rstd,  dn = g gamma,  dy = rstd (dn - mean(dn) - y^ mean(dn y^))
    f32x16 g[4];
    load_row_or_zero(g, a.grad_out + row * kFfnE, valid, h);
    if (a.post_g) {
        const float2 ms = *reinterpret_cast<const float2 *>(a.stat_post + 2 * row);
        f32x16 nh[4];
        load_row(nh, a.ysave + row * kFfnE, h);
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) nh[b][r] = (nh[b][r] - ms.x) * ms.y;
        tile_sum<4>([&](int b, int r) { return g[b][r] * nh[b][r]; }, valid, s_part, vp + kVpPostG, t, wv, j, h);
        tile_sum<4>([&](int b, int r) { return g[b][r]; }, valid, s_part, vp + kVpPostB, t, wv, j, h);
        ln_bwd_rows(g, nh, a.post_g, ms.y, h);
    }
    if (valid) {
        store_row_regs(a.dy + lrow * kFfnE, g, h);
        if (a.grad_res) store_row_regs(a.grad_res + row * kFfnE, g, h);
    }

    // g = da = dy * (kept ? scale_out : 0)
    if (a.wid) tile_sum<4>([&](int b, int r) { return g[b][r]; }, valid, s_part, vp + kVpBid, t, wv, j, h);
    if (a.keep_out) drop_rows(g, keep_bits(a.keep_out + row * kFfnE, h), a.scale_out);
    if (valid) store_row_regs(a.da + lrow * kFfnE, g, h);
    tile_sum<4>([&](int b, int r) { return g[b][r]; }, valid, s_part, vp + kVpB2, t, wv, j, h);

    // Pass 1, the hidden slices: h' and dz of every slice, to the chunk's rows.  u, as the forward forms it
    f32x16 u[NB];
    load_row(u, a.x + row * CIN, h);
    if (a.pre_g) {
        float part[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) s += u[b][r];
            part[b] = s;
        }
        ln_rows<true, NB>(u, tree_sum<NB>(part), reinterpret_cast<const float4 *>(a.pre_g), reinterpret_cast<const float4 *>(a.pre_b), h);
    }

    f32x16 hid[4];
    float4 pre[4];
#pragma unroll 1
    for (int s = 0; s < kFfnSlices; ++s) {
        // h_s = relu(W1_s u + b1_s) by the forward's chain: chunk c of W1's rows 128 s .. against u's block c
        const float *w1s = a.w1 + (size_t)(128 * s) * CIN;
        zero_rows(hid);
        chunk_fetch(pre, w1s, CIN, 0, t);
        chunk_stash(s_w[0], pre, t);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            if (c + 1 < NB) chunk_fetch(pre, w1s, CIN, 32 * (c + 1), t);
            chunk_mfma(hid, u[c], s_w[c & 1], j, h);
            if (c + 1 < NB) chunk_stash(s_w[(c + 1) & 1], pre, t);
            __syncthreads();
        }
        uint64_t live = 0;     // bit 16 b + r: h > 0 or NaN (torch's threshold passes the gradient of a NaN on)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float4 bb = ld4(a.b1 + 128 * s + 32 * b + 8 * m + 4 * h);
                const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = hid[b][4 * m + i] + bv[i];
                    hid[b][4 * m + i] = v < 0.f ? 0.f : v;
                    live |= (uint64_t)(!(v <= 0.f)) << (16 * b + 4 * m + i);
                }
            }
        uint64_t kh = ~0ull;
        if (a.keep_hidden) {
            kh = keep_bits(a.keep_hidden + row * kFfnF + 128 * s, h);
            drop_rows(hid, kh, a.scale_hidden);
        }
        if (valid) store_row_regs(a.hrows + lrow * kFfnF + 128 * s, hid, h);

        // dh_s = W2[:, 128 s ..]^T da, then dz_s
        zero_rows(hid);
        product_t<4, false>(hid, g, a.w2 + 128 * s, kFfnF, 0, buf0, buf1, t, j, h);
        if (a.keep_hidden) drop_rows(hid, kh, a.scale_hidden);
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) hid[b][r] = (live >> (16 * b + r)) & 1u ? hid[b][r] : 0.f;
        if (valid) store_row_regs(a.dz + lrow * kFfnF + 128 * s, hid, h);
        tile_sum<4>([&](int b, int r) { return hid[b][r]; }, valid, s_part, vp + kVpB1 + 128 * s, t, wv, j, h);
    }

    // Pass 2: du = Wid^T dy + sum over the slices of W1_s^T dz_s, from the rows the lane itself stored (u's registers are free
    // by now: u, du, da and a slice at once do not fit a wave's 512 registers at Cin = 256).  A row past n supplies zeros.
    // Each of the five products is a chain of its own from 0 and joins du by one addition: 128 terms a chain, not 640 in one
    // accumulator, whose rounding showed in the pre norm's bias gradient (a plain sum of du over the rows) at small n
    f32x16 du[NB];
    zero_rows(du);
    auto add_product = [&](const float *w) {      // du += W^T hid, W's 128 rows at w
#pragma unroll
        for (int q = 0; q < NB / 4; ++q) {
            f32x16 acc[4];
            zero_rows(acc);
            product_t<4, false>(acc, hid, w + 128 * q, CIN, 0, buf0, buf1, t, j, h);
#pragma unroll
            for (int b = 0; b < 4; ++b) du[4 * q + b] += acc[b];
        }
    };
    auto reload = [&](const float *p) { load_row_or_zero(hid, p, valid, h); };
    if (a.wid) {
        reload(a.dy + lrow * kFfnE);
        add_product(a.wid);
    }
#pragma unroll 1
    for (int s = 0; s < kFfnSlices; ++s) {
        reload(a.dz + lrow * kFfnF + 128 * s);
        add_product(a.w1 + (size_t)(128 * s) * CIN);
    }

    // the pre norm's backward on du, x^ formed again in u's registers
    if (a.pre_g) {
        const float2 ms = *reinterpret_cast<const float2 *>(a.stat_pre + 2 * row);
        load_row(u, a.x + row * CIN, h);
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) u[b][r] = (u[b][r] - ms.x) * ms.y;
#pragma unroll
        for (int q = 0; q < NB / 4; ++q) {
            tile_sum<4>([&](int b, int r) { return du[4 * q + b][r] * u[4 * q + b][r]; }, valid, s_part, vp + kVpPre + 128 * q, t, wv, j, h);
            tile_sum<4>([&](int b, int r) { return du[4 * q + b][r]; }, valid, s_part, vp + kVpPre + CIN + 128 * q, t, wv, j, h);
        }
        ln_bwd_rows(du, u, a.pre_g, ms.y, h);
    }
    if (valid) store_row_regs(a.grad_x + row * CIN, du, h);
}

struct FfnWgArgs {
    const float *x, *stat_pre, *pre_g, *pre_b;   // u = LN_pre(x) formed again (pre_g null: u = x)
    const float *hrows, *dz, *da, *dy;           // the chunk's rows
    float *wpart;                                // [blocks][ffn_wpart_len(Cin)]
    int n, base, cin;
};

// One job of a row block: a 128 x 128 piece of dW = left^T right over the block's rows, A = left[row][o] and B = right[row][k],
// two rows a step (lanes 0-31 one, lanes 32-63 the other), loaded from the row-major arrays as they lie; a wave owns 32 rows
// o.  Jobs, with KG = Cin / 128: 4 KG of dW1 (left dz, right u), 4 of dW2 (left da, right h'), KG of dWid (left dy, right u).
// A lane beyond the block's rows supplies 0 (a select) and loads the block's last row.
__global__ __launch_bounds__(256) void gf_ffn_wgrad_kernel(FfnWgArgs a)
{
    const int job = blockIdx.y, blk = a.base / kFfnWgRows + blockIdx.x, cin = a.cin, KG = cin / 128;
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int r0 = blk * kFfnWgRows, r1 = min(a.n, r0 + kFfnWgRows);
    const float *left, *right;     // the left array's column group, the right one's; chunk arrays start at row a.base
    size_t ldl, ldr;
    float *dst;
    size_t ldd;
    bool right_is_u;
    int kcol = 0;                  // right_is_u: the first column of x in the job
    float *part = a.wpart + (size_t)blk * ffn_wpart_len(cin);
    if (job < 4 * KG) {
        const int og = job / KG, kg = job - og * KG;
        left = a.dz + 128 * og; ldl = kFfnF;
        right = a.x + 128 * kg; ldr = cin; right_is_u = true; kcol = 128 * kg;
        dst = part + (size_t)(128 * og) * cin + 128 * kg; ldd = cin;
    } else if (job < 4 * KG + 4) {
        const int kg = job - 4 * KG;
        left = a.da; ldl = kFfnE;
        right = a.hrows + 128 * kg; ldr = kFfnF; right_is_u = false;
        dst = part + (size_t)kFfnF * cin + 128 * kg; ldd = kFfnF;
    } else {
        const int kg = job - 4 * KG - 4;
        left = a.dy; ldl = kFfnE;
        right = a.x + 128 * kg; ldr = cin; right_is_u = true; kcol = 128 * kg;
        dst = part + (size_t)kFfnF * cin + (size_t)kFfnE * kFfnF + 128 * kg; ldd = cin;
    }
    left += 32 * wv + j;
    right += j;
    const bool norm = right_is_u && a.pre_g;
    const int rsub = right_is_u ? 0 : a.base;
    float gv[4], ev[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        gv[cb] = norm ? a.pre_g[kcol + 32 * cb + j] : 1.f;
        ev[cb] = norm ? a.pre_b[kcol + 32 * cb + j] : 0.f;
    }
    f32x16 acc[4];
    zero_rows(acc);
    if (norm) wgrad_rows<kWgNorm>(acc, left, ldl, a.base, right, nullptr, ldr, rsub, a.stat_pre, gv, ev, r0, r1, r1, h);
    else wgrad_rows<kWgAsIs>(acc, left, ldl, a.base, right, nullptr, ldr, rsub, nullptr, gv, ev, r0, r1, r1, h);
    wgrad_store(dst, ldd, [&](int cb, int r) { return acc[cb][r]; }, wv, j, h);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

// a dropout's scale where its mask is given
static int ffn_check_scale(const char *fn, const char *what, const unsigned char *keep, float scale)
{
    GF_REFUSE_AS(fn, !keep || (std::isfinite(scale) && scale > 0.f), "%s = %g is not a positive finite number", what, (double)scale);
    return GF_OK;
}

// The training step's two regions, sized and carved by one function each (a null base: sizes only).
struct FfnSaved { float *ysave, *stat_pre, *stat_post; size_t bytes; };
static FfnSaved ffn_carve_saved(void *base, int n)
{
    Carver c(base);
    FfnSaved s;
    s.ysave = c.take<float>((size_t)n * kFfnE);
    s.stat_pre = c.take<float>((size_t)n * 2);
    s.stat_post = c.take<float>((size_t)n * 2);
    s.bytes = c.bytes();
    return s;
}
struct FfnWork { float *hrows, *dz, *da, *dy, *vpart, *wpart; int tiles, blocks, crows; size_t bytes; };
static FfnWork ffn_carve_work(void *base, int n, int Cin)
{
    Carver c(base);
    FfnWork w;
    w.tiles = (n + kRowTile - 1) / kRowTile;
    w.blocks = (n + kFfnWgRows - 1) / kFfnWgRows;
    w.crows = n < kFfnChunkRows ? n : kFfnChunkRows;
    w.hrows = c.take<float>((size_t)w.crows * kFfnF);
    w.dz = c.take<float>((size_t)w.crows * kFfnF);
    w.da = c.take<float>((size_t)w.crows * kFfnE);
    w.dy = c.take<float>((size_t)w.crows * kFfnE);
    w.vpart = c.take<float>((size_t)w.tiles * ffn_vpart_len(Cin));
    w.wpart = c.take<float>((size_t)w.blocks * ffn_wpart_len(Cin));
    w.bytes = c.bytes();
    return w;
}

}  // namespace gf

extern "C" int gf_ffn_train_sizes(int n, int Cin, size_t *saved_bytes, size_t *workspace_bytes)
{
    using namespace gf;
    const char *fn = __func__;
    GF_REFUSE_AS(fn, Cin == 128 || Cin == 256, "Cin = %d: only in_channels = 128 or 256 is supported", Cin);
    GF_REFUSE_AS(fn, n >= 0, "n = %d is negative", n);
    GF_REFUSE_AS(fn, saved_bytes && workspace_bytes, "null pointer");
    *saved_bytes = ffn_carve_saved(nullptr, n).bytes;
    *workspace_bytes = ffn_carve_work(nullptr, n, Cin).bytes;
    return GF_OK;
}

extern "C" int gf_ffn_forward_train(int n, int Cin, int F, int E, const float *x, const void *const *params, const float *residual,
                                    const unsigned char *keep_hidden, float scale_hidden, const unsigned char *keep_out, float scale_out,
                                    float *out, void *saved, size_t saved_bytes, void *stream_)
{
    using namespace gf;
    const char *fn = __func__;
    if (int rc = ffn_check(fn, n, Cin, F, E, x, params, residual, out)) return rc;
    if (int rc = ffn_check_scale(fn, "scale_hidden", keep_hidden, scale_hidden)) return rc;
    if (int rc = ffn_check_scale(fn, "scale_out", keep_out, scale_out)) return rc;
    GF_REFUSE_AS(fn, !misaligned16(saved), "saved is not 16-byte aligned");
    if (n == 0) return GF_OK;
    GF_REFUSE_AS(fn, x && out, "null pointer");
    GF_REFUSE_AS(fn, saved, "saved is null");
    const FfnSaved sv = ffn_carve_saved(saved, n);
    GF_CHECK_WORKSPACE_AS(fn, "saved", saved_bytes, sv.bytes);
    const float *const *p = reinterpret_cast<const float *const *>(params);
    FfnTrainArgs a{};
    static_cast<FfnArgs &>(a) = FfnArgs{x, residual, out, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], n};
    a.keep_hidden = keep_hidden; a.keep_out = keep_out;
    a.scale_hidden = scale_hidden; a.scale_out = scale_out;
    a.ysave = sv.ysave; a.stat_pre = sv.stat_pre; a.stat_post = sv.stat_post;
    // the tile kernel at every n: the 32-row kernel's bits (§3.13c), one saving build
    const dim3 grid((n + kRowTile - 1) / kRowTile);
    if (Cin == 256) hipLaunchKernelGGL((gf_ffn_kernel<256, true>), grid, dim3(256), 0, (hipStream_t)stream_, a);
    else hipLaunchKernelGGL((gf_ffn_kernel<128, true>), grid, dim3(256), 0, (hipStream_t)stream_, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_ffn_backward(int n, int Cin, int F, int E, const float *x, const void *const *params, const unsigned char *keep_hidden,
                               float scale_hidden, const unsigned char *keep_out, float scale_out, const void *saved, const float *grad_out,
                               float *grad_x, float *grad_residual, void *const *grad_params, void *workspace, size_t workspace_bytes,
                               void *stream_)
{
    using namespace gf;
    const char *fn = __func__;
    if (int rc = ffn_check(fn, n, Cin, F, E, x, params, nullptr, nullptr)) return rc;
    GF_REFUSE_AS(fn, !misaligned16(grad_x), "grad_x is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(grad_residual), "grad_residual is not 16-byte aligned");
    if (int rc = ffn_check_scale(fn, "scale_hidden", keep_hidden, scale_hidden)) return rc;
    if (int rc = ffn_check_scale(fn, "scale_out", keep_out, scale_out)) return rc;
    GF_REFUSE_AS(fn, grad_params, "null grad_params");
    const float *const *p = reinterpret_cast<const float *const *>(params);
    float *const *gp = reinterpret_cast<float *const *>(grad_params);
    for (int i = 0; i < GF_FFN_PARAMS; ++i) {
        GF_REFUSE_AS(fn, !p[i] || gp[i], "the gradient of %s is null", kFfnName[i]);
        GF_REFUSE_AS(fn, !p[i] || !misaligned16(gp[i]), "the gradient of %s is not 16-byte aligned", kFfnName[i]);
    }
    GF_REFUSE_AS(fn, !misaligned16(grad_out), "grad_out is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(saved), "saved is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(workspace), "workspace is not 16-byte aligned");
    const FfnSaved sv = ffn_carve_saved(n > 0 ? const_cast<void *>(saved) : nullptr, n);
    const FfnWork ws = ffn_carve_work(n > 0 ? workspace : nullptr, n, Cin);
    if (n > 0) {
        GF_REFUSE_AS(fn, x && grad_out && grad_x, "null pointer");
        GF_REFUSE_AS(fn, saved, "saved is null");
        GF_REFUSE_AS(fn, workspace, "workspace is null");
        GF_CHECK_WORKSPACE_AS(fn, "workspace", workspace_bytes, ws.bytes);
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (n > 0) {
        FfnBwdArgs b{};
        b.x = x; b.grad_out = grad_out; b.grad_x = grad_x; b.grad_res = grad_residual;
        b.pre_g = p[0]; b.pre_b = p[1]; b.w1 = p[2]; b.b1 = p[3]; b.w2 = p[4]; b.wid = p[6]; b.post_g = p[8];
        b.keep_hidden = keep_hidden; b.keep_out = keep_out; b.scale_hidden = scale_hidden; b.scale_out = scale_out;
        b.ysave = sv.ysave; b.stat_pre = sv.stat_pre; b.stat_post = sv.stat_post;
        b.hrows = ws.hrows; b.dz = ws.dz; b.da = ws.da; b.dy = ws.dy; b.vpart = ws.vpart;
        b.n = n;
        FfnWgArgs g{};
        g.x = x; g.stat_pre = sv.stat_pre; g.pre_g = p[0]; g.pre_b = p[1];
        g.hrows = ws.hrows; g.dz = ws.dz; g.da = ws.da; g.dy = ws.dy; g.wpart = ws.wpart;
        g.n = n; g.cin = Cin;
        const int jobs = 4 * (Cin / 128) + 4 + (p[6] ? Cin / 128 : 0);
        for (int base = 0; base < n; base += kFfnChunkRows) {   // the next chunk's data backward overwrites the rows behind this one's wgrad
            const int rows = n - base < kFfnChunkRows ? n - base : kFfnChunkRows;
            b.base = g.base = base;
            const dim3 grid((rows + kRowTile - 1) / kRowTile);
            if (Cin == 256) hipLaunchKernelGGL(gf_ffn_bwd_kernel<256>, grid, dim3(256), 0, stream, b);
            else hipLaunchKernelGGL(gf_ffn_bwd_kernel<128>, grid, dim3(256), 0, stream, b);
            GF_CHECK_LAUNCH();
            hipLaunchKernelGGL(gf_ffn_wgrad_kernel, dim3((rows + kFfnWgRows - 1) / kFfnWgRows, jobs), dim3(256), 0, stream, g);
            GF_CHECK_LAUNCH();
        }
    }
    // n == 0: no partials, the sums store zeros
    RowsSumArgs<GF_FFN_PARAMS> sa{};   // float sums, a thread per element
    int nj = 0;
    const int vlen = ffn_vpart_len(Cin);
    auto vec = [&](int i, int at, int len) {
        if (p[i]) sa.job[nj++] = RowsSumJob{n > 0 ? ws.vpart + at : nullptr, gp[i], (size_t)vlen, n > 0 ? ws.tiles : 0, len, 0, 1};
    };
    auto mat = [&](int i, size_t at, int len) {
        if (p[i]) sa.job[nj++] = RowsSumJob{n > 0 ? ws.wpart + at : nullptr, gp[i], ffn_wpart_len(Cin), n > 0 ? ws.blocks : 0, len, 0, 1};
    };
    vec(0, kVpPre, Cin);
    vec(1, kVpPre + Cin, Cin);
    mat(2, 0, kFfnF * Cin);
    vec(3, kVpB1, kFfnF);
    mat(4, (size_t)kFfnF * Cin, kFfnE * kFfnF);
    vec(5, kVpB2, kFfnE);
    mat(6, (size_t)kFfnF * Cin + (size_t)kFfnE * kFfnF, kFfnE * Cin);
    vec(7, kVpBid, kFfnE);
    vec(8, kVpPostG, kFfnE);
    vec(9, kVpPostB, kFfnE);
    hipLaunchKernelGGL((rows_sum_kernel<float, GF_FFN_PARAMS>), dim3(kFfnF * Cin / 256, nj), dim3(256), 0, stream, sa);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
