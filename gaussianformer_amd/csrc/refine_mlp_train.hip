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
#include "gf_rows.hpp"

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

// dst[0 .. 32 NB) = the sum over the tile's rows of f(b, r), the lane's value at feature(b, r, h) of its row (rows past n add
// 0): sum32_last over a wave's 32 rows, then the four waves in their order.  Every wave calls it together (two barriers)
template <int NB, class F>
__device__ __forceinline__ void rm_tile_sum(F f, bool valid, float (*s_part)[kRmE], float *dst, int t, int wv, int j, int h)
{
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float s = sum32_last(valid ? f(b, r) : 0.f);
            if (j == 31) s_part[wv][32 * b + 8 * (r >> 2) + 4 * h + (r & 3)] = s;
        }
    __syncthreads();
    if (t < 32 * NB) dst[t] = (s_part[0][t] + s_part[1][t]) + (s_part[2][t] + s_part[3][t]);
    __syncthreads();
}

// the lane's values of NB blocks of its row, to / from memory as float4s
template <int NB>
__device__ __forceinline__ void rm_store_row(float *p, const f32x16 (&v)[NB], int h)
{
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int m = 0; m < 4; ++m)
            *reinterpret_cast<float4 *>(p + 32 * b + 8 * m + 4 * h) = make_float4(v[b][4 * m], v[b][4 * m + 1], v[b][4 * m + 2], v[b][4 * m + 3]);
}
template <int NB>
__device__ __forceinline__ void rm_load_row(f32x16 (&v)[NB], const float *p, int h)
{
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 q = ld4(p + 32 * b + 8 * m + 4 * h);
            v[b][4 * m] = q.x; v[b][4 * m + 1] = q.y; v[b][4 * m + 2] = q.z; v[b][4 * m + 3] = q.w;
        }
}

// acc[fb] += (W^T g)'s features 32 fb ..: W [nrows, 128] row-major, g holds the features 0 .. 32 NC of the wave's rows, acc the
// 128 input features.  A local copy of ffn_train.hip's ffn_product_t (that one stays where it is: its translation unit's
// assembly is not touched) with two differences: NC chunks of 32 rows o instead of four, and W's rows from nrows on supplied as
// zero -- the row index is clamped and the value masked, nothing beyond the tensor is loaded.  W goes through LDS in chunks of
// 32 rows x 128 floats, double buffered; step (c, r) sums over o = feature(c, r, 0 / 1) with g's register as the B operand as
// it stands and W[o][32 fb + j] read along the row (pitch 136: rows 4 apart lie 32 banks apart).  Every wave of the workgroup
// calls it together; it ends behind a barrier
constexpr int kRmTPitch = 136;
template <int NC>
__device__ __forceinline__ void rm_product_t(f32x16 (&acc)[4], const f32x16 (&g)[NC], const float *w, int nrows, float *buf0, float *buf1,
                                             int t, int j, int h)
{
    constexpr int P = kRmTPitch;
    const int rr = t >> 3, fq = t & 7;
    float4 pre[4];
    auto fetch = [&](int c) {
        const int o = 32 * c + rr;
        const float *src = w + (size_t)min(o, nrows - 1) * kRmE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 v = ld4(src + 4 * (fq + 8 * i));
            pre[i] = o < nrows ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    fetch(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4 *>(buf0 + rr * P + 4 * (fq + 8 * i)) = pre[i];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float *cur = c & 1 ? buf1 : buf0;
        float *nxt = c & 1 ? buf0 : buf1;
        if (c + 1 < NC) fetch(c + 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float *wrow = cur + (8 * (r >> 2) + 4 * h + (r & 3)) * P + j;
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[32 * fb], g[c][r], acc[fb], 0, 0, 0);
        }
        if (c + 1 < NC) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<float4 *>(nxt + rr * P + 4 * (fq + 8 * i)) = pre[i];
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void rm_zero(f32x16 (&v)[4])
{
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) v[b][r] = 0.f;
}

__global__ __launch_bounds__(256) void gf_refine_mlp_bwd_kernel(RmBwdArgs a)
{
    __shared__ float4 s_w[2][32 * kRmTPitch / 4];
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
        rm_load_row<2>(yv, a.y + row * kRmYPitch, h);
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
        rm_tile_sum<2>([&](int b, int r) { return yv[b][r]; }, valid, s_part, vp + kRmVScale, t, wv, j, h);
        rm_tile_sum<2>([&](int b, int r) { return gy[b][r]; }, valid, s_part, vp + kRmVB10, t, wv, j, h);
        if (valid) rm_store_row<2>(a.dz4 + lrow * kRmYPitch, gy, h);
        rm_zero(acc);
        rm_product_t<2>(acc, gy, a.w[4], D, buf0, buf1, t, j, h);
    }

    // the four square stages, last first: acc holds the gradient of the stage's output (behind the LayerNorm where it has one)
#pragma unroll 1
    for (int q = 3; q >= 0; --q) {
        // the stage's saved post-ReLU row, and where it passes a gradient
        rm_load_row<4>(g, a.rows + ((size_t)q * n + row) * kRmE, h);
        uint64_t live = 0;       // bit 16 b + r
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) live |= (uint64_t)(!(g[b][r] <= 0.f)) << (16 * b + r);
        if (q & 1) {
            // the LayerNorm's backward: r^ = (r - mean) rstd, dn = acc gamma, dr = rstd (dn - mean(dn) - r^ mean(dn r^))
            const float2 ms = *reinterpret_cast<const float2 *>(a.stat + ((size_t)(q >> 1) * n + row) * 2);
            const float *gam = a.ln_g[q >> 1];
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) g[b][r] = (g[b][r] - ms.x) * ms.y;
            float *vln = vp + kRmVLn + 2 * kRmE * (q >> 1);
            rm_tile_sum<4>([&](int b, int r) { return acc[b][r] * g[b][r]; }, valid, s_part, vln, t, wv, j, h);
            rm_tile_sum<4>([&](int b, int r) { return acc[b][r]; }, valid, s_part, vln + kRmE, t, wv, j, h);
            float p1[4], p2[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float4 gg = ld4(gam + 32 * b + 8 * m + 4 * h);
                    const float gv[4] = {gg.x, gg.y, gg.z, gg.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float dn = acc[b][4 * m + i] * gv[i];
                        s1 += dn;
                        s2 += dn * g[b][4 * m + i];
                        acc[b][4 * m + i] = dn;
                    }
                }
                p1[b] = s1;
                p2[b] = s2;
            }
            const float m1 = wave_xor_reduce_strided(tree_sum<4>(p1), 32, Sum()) * (1.f / kRmE);
            const float m2 = wave_xor_reduce_strided(tree_sum<4>(p2), 32, Sum()) * (1.f / kRmE);
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[b][r] = ms.y * (acc[b][r] - m1 - g[b][r] * m2);
        }
        // dz = the ReLU's backward; a row past n carries zeros
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) g[b][r] = valid && ((live >> (16 * b + r)) & 1u) ? acc[b][r] : 0.f;
        if (valid) rm_store_row<4>(a.dz + ((size_t)q * a.crows + lrow) * kRmE, g, h);
        rm_tile_sum<4>([&](int b, int r) { return g[b][r]; }, valid, s_part, vp + kRmVBias + kRmE * q, t, wv, j, h);
        rm_zero(acc);
        rm_product_t<4>(acc, g, a.w[q], kRmE, buf0, buf1, t, j, h);
    }
    if (valid) rm_store_row<4>(a.grad_x + row * kRmE, acc, h);
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
// beyond the block's rows supplies 0 (a select) and loads the block's last row.  (gf_ffn_wgrad_kernel's scheme.)
// (KIND: 0 the sum of the two inputs, 1 saved rows as they are, 2 their LayerNorm -- a template, so the row loop has no branch
// in it and its loads go out together)
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
    const float *right = (KIND == 0 ? a.feat : a.rows + (size_t)(s - 1) * n * kRmE) + j, *right2 = a.embed + j;
    const float *stat = a.stat + (size_t)(s == 4 ? 1 : 0) * n * 2;
    float gv[4], ev[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        gv[cb] = KIND == 2 ? a.ln_g[s == 4][32 * cb + j] : 1.f;
        ev[cb] = KIND == 2 ? a.ln_b[s == 4][32 * cb + j] : 0.f;
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
        const int re = min(r1, rb + kRmWgFlush);
        rm_zero(acc);
        for (int r = rb; r < re; r += 8) {
            float av[4], xv[4][4];
            float2 ms[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = min(r + 2 * q + h, r1 - 1);
                av[q] = left[(size_t)(row - a.base) * ldl];
                if constexpr (KIND == 2) ms[q] = *reinterpret_cast<const float2 *>(stat + (size_t)row * 2);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    xv[q][cb] = right[(size_t)row * kRmE + 32 * cb];
                    if constexpr (KIND == 0) xv[q][cb] = xv[q][cb] + right2[(size_t)row * kRmE + 32 * cb];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool live = r + 2 * q + h < r1;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    float bv = xv[q][cb];
                    if constexpr (KIND == 2) bv = __builtin_fmaf((bv - ms[q].x) * ms[q].y, gv[cb], ev[cb]);
                    acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(live ? av[q] : 0.f, live ? bv : 0.f, acc[cb], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) outer[cb][r] += (double)acc[cb][r];
    }
    float *dst = a.wpart + (size_t)blk * kRmWLen + (size_t)s * kRmE * kRmE + j;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(size_t)(32 * wv + 8 * (r >> 2) + 4 * h + (r & 3)) * kRmE + 32 * cb] = (float)outer[cb][r];
}

__global__ __launch_bounds__(256, 2) void gf_refine_mlp_wgrad_kernel(RmWgArgs a)
{
    const int s = blockIdx.y;
    if (s == 0) rm_wgrad_job<0>(a, s);
    else if (s & 1) rm_wgrad_job<1>(a, s);
    else rm_wgrad_job<2>(a, s);
}

// dst[e] = the sum over `count` partials, `stride` floats apart, in a fixed order, accumulated in double and rounded once (the
// partials are fp32 sums over 128 or 512 rows; at 144 000 rows there are 1 125 or 282 of them).  slots == 1 (the matrices:
// many elements, few partials): a thread per element, four interleaved running sums, then their tree, as gf_ffn_sum_kernel's.
// slots == kRmSumSlots (the vectors: few elements, a partial per tile): 16 threads per element, thread k takes the partials
// k, k + 16, .. the same way, and the 16 results meet in a tree -- the two-level sum §3.13b asked for.  count == 0 stores zeros.
constexpr int kRmSumSlots = 16;
struct RmSumJob { const float *src; float *dst; size_t stride; int count, len, slots; };
struct RmSumArgs { RmSumJob job[GF_REFINE_MLP_PARAMS]; };
__global__ __launch_bounds__(256) void gf_refine_mlp_sum_kernel(RmSumArgs a)
{
    __shared__ double s_sum[256];
    const RmSumJob &jb = a.job[blockIdx.y];
    const int slots = jb.slots, per = 256 / slots;          // elements of a workgroup
    if ((int)blockIdx.x * per >= jb.len) return;            // (the whole workgroup)
    const int el = threadIdx.x % per, slot = threadIdx.x / per, e = blockIdx.x * per + el;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (e < jb.len) {
        const float *src = jb.src + e;
        int i = slot;
        for (; i + 3 * slots < jb.count; i += 4 * slots) {
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += (double)src[(size_t)(i + q * slots) * jb.stride];
        }
        for (; i < jb.count; i += slots) s[0] += (double)src[(size_t)i * jb.stride];
    }
    const double v = (s[0] + s[1]) + (s[2] + s[3]);
    if (slots == 1) {
        if (e < jb.len) jb.dst[e] = (float)v;
        return;
    }
    s_sum[threadIdx.x] = v;
    __syncthreads();
    if (slot == 0 && e < jb.len) {
        double p[kRmSumSlots];
#pragma unroll
        for (int k = 0; k < kRmSumSlots; ++k) p[k] = s_sum[k * per + el];
#pragma unroll
        for (int w = kRmSumSlots / 2; w > 0; w >>= 1)
#pragma unroll
            for (int k = 0; k < w; ++k) p[k] = p[2 * k] + p[2 * k + 1];
        jb.dst[e] = (float)p[0];
    }
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
    GF_RM_REFUSE(n >= 0, "n = %d is negative", n);
    GF_RM_REFUSE(D >= 10 && D <= 10 + 1 + kRefMaxS, "D = %d is not in 10 .. %d", D, 10 + 1 + kRefMaxS);
    GF_RM_REFUSE(Da >= 0, "Da = %d is negative", Da);
    GF_RM_REFUSE(saved_bytes && workspace_bytes, "null pointer");
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
    GF_RM_REFUSE(E == kRmE, "E = %d: only embed_dims = 128 is supported", E);
    GF_RM_REFUSE(grad_params, "null grad_params");
    float *const *gp = reinterpret_cast<float *const *>(grad_params);
    for (int i = 0; i < GF_REFINE_MLP_PARAMS; ++i) GF_RM_REFUSE(gp[i], "grad_params[%d] (the gradient of %s) is null", i, kRmName[i]);
    hipStream_t stream = (hipStream_t)stream_;
    const RefineMlpSaved sv = refine_mlp_carve_saved(n > 0 ? const_cast<void *>(saved) : nullptr, n, D);
    const RmWork ws = rm_carve_work(n > 0 ? workspace : nullptr, n, D);
    if (n > 0) {
        if (int rc = refine_mlp_check_inputs(fn, params, instance_feature, anchor_embed, anchor)) return rc;
        GF_RM_REFUSE(saved, "saved is null");
        GF_RM_REFUSE(!rm_misaligned(saved), "saved = %p is not 16-byte aligned", saved);
        GF_RM_REFUSE(workspace, "workspace is null");
        GF_RM_REFUSE(!rm_misaligned(workspace), "workspace = %p is not 16-byte aligned", workspace);
        GF_RM_REFUSE(grad_x, "grad_x is null");
        GF_RM_REFUSE(!rm_misaligned(grad_x), "grad_x = %p is not 16-byte aligned", (const void *)grad_x);
        GF_RM_REFUSE(grad_anchor, "grad_anchor is null");
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
    // (3) n == 0: no partials, the sums store zeros
    RmSumArgs sa{};
    auto vec = [&](int i, int at, int len) {
        sa.job[i] = RmSumJob{n > 0 ? ws.vpart + at : nullptr, gp[i], (size_t)kRmVLen, n > 0 ? ws.tiles : 0, len, kRmSumSlots};
    };
    auto mat = [&](int i, int s, int len) {
        sa.job[i] = RmSumJob{n > 0 ? ws.wpart + (size_t)s * kRmE * kRmE : nullptr, gp[i], kRmWLen, n > 0 ? ws.blocks : 0, len, 1};
    };
    mat(0, 0, kRmE * kRmE);   vec(1, kRmVBias, kRmE);
    mat(2, 1, kRmE * kRmE);   vec(3, kRmVBias + kRmE, kRmE);
    vec(4, kRmVLn, kRmE);     vec(5, kRmVLn + kRmE, kRmE);
    mat(6, 2, kRmE * kRmE);   vec(7, kRmVBias + 2 * kRmE, kRmE);
    mat(8, 3, kRmE * kRmE);   vec(9, kRmVBias + 3 * kRmE, kRmE);
    vec(10, kRmVLn + 2 * kRmE, kRmE); vec(11, kRmVLn + 3 * kRmE, kRmE);
    mat(12, 4, D * kRmE);     vec(13, kRmVB10, D);
    vec(14, kRmVScale, D);
    hipLaunchKernelGGL(gf_refine_mlp_sum_kernel, dim3(kRmE * kRmE / 256, GF_REFINE_MLP_PARAMS), dim3(256), 0, stream, sa);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
