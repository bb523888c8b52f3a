// Modulated deformable convolution (mmcv's DCNv2, ModulatedDeformConv2dPack) for the image backbone's layer3 / layer4.
// The contract: include/gf_hip.h and gaussianformer_amd/deform_conv.py; the design and the measured numbers: DESIGN.md §3.11.
//
// Every product runs on v_mfma_f32_32x32x2_f32 (exact fp32 operands, fp32 accumulate).  No column matrix is written to memory:
//   relayout   input [N][C][H W] -> channels-last [N][H W][C] in the workspace (each bilinear corner is one contiguous row), and
//              the weight [Co][C][kh kw] -> [tap][C][Co] (forward) or [tap][Co][C] (backward)
//   forward    a workgroup owns 128 output pixels x 64 output channels.  Per (tap, deform group) the 128 pixels' corner rows,
//              bilinear weights and mask are computed once (LDS); per 32-channel chunk the column tile [32 c][128 p] is built
//              in LDS from the four corner rows, and each wave multiplies a 32 x 32 weight slice into two 32 x 32 pixel tiles.
//              NCHW output, bias in the epilogue
//   bwd data   a workgroup owns 128 output pixels and every (tap, group, chunk): grad_col [32 c][32 p] = W^T grad_out per wave
//              (K = Co), through LDS to one (pixel, channel) per lane, channels on the lanes; grad_input by fp32 atomics into
//              a channels-last scratch (then transposed), grad_offset / grad_mask as fixed-order sums over the group's channels
//   bwd weight grad_weight [Co][c, tap] = grad_out . cols^T with the columns rebuilt per 64-pixel block; the pixels are split over
//              `slices` workgroups whose partials are summed in slice order by a second kernel (fixed order)
//   bwd bias   one workgroup per output channel, fixed-order tree
// Only grad_input uses atomics; everything else is bitwise reproducible.
#include "gf_common.hpp"

namespace gf {
namespace dcn {   // a named namespace: every kernel has external linkage and a stable name

constexpr int kThreads = 256;
constexpr int kGran = 32;          // channel granule: Cin / dg and Co are multiples of it
constexpr int kFwdBM = 128;        // forward: output pixels per workgroup
constexpr int kFwdBN = 64;         // forward: output channels per workgroup
constexpr int kColS = kFwdBM + 2;  // LDS row pitch of the forward column tile (8 c4-groups x 8 pixels hit distinct banks)
constexpr int kBdBM = 128;         // backward data: output pixels per workgroup (one 32-pixel tile per wave)
constexpr int kWgBP = 64;          // backward weight: pixels per block
constexpr int kWgBN = 128;         // backward weight: output channels per workgroup (one 32-row tile per wave)
constexpr int kWgTarget = 1024;    // backward weight: workgroups aimed at (tiles x slices)
constexpr int kWgMaxSlices = 16;

struct Geom {
    int N, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg;
    int Ho, Wo, HoWo, NP, Cg, kk;
};

inline int wg_tiles(const Geom &g) { return ((g.Co + kWgBN - 1) / kWgBN) * g.kk * (g.C / kGran); }
inline int wg_slices(const Geom &g)
{
    int s = (kWgTarget + wg_tiles(g) - 1) / wg_tiles(g);
    s = s < 1 ? 1 : (s > kWgMaxSlices ? kWgMaxSlices : s);
    const int blocks = (g.NP + kWgBP - 1) / kWgBP;
    return s > blocks ? (blocks > 0 ? blocks : 1) : s;
}

struct Ws {
    float *xn;     // [N][H W][C]
    float *wr;     // forward [kk][C][Co]; backward [kk][Co][C]
    float *gin;    // backward: [N][H W][C] grad_input accumulator
    float *part;   // backward: [slices][kk][Co][C] grad_weight partials
    size_t total;
};

inline Ws carve(void *base, const Geom &g, int backward)
{
    Carver c(base);
    Ws w;
    const size_t x = (size_t)g.N * g.H * g.W * g.C, wt = (size_t)g.kk * g.C * g.Co;
    w.xn = c.take<float>(x);
    w.wr = c.take<float>(wt);
    w.gin = backward ? c.take<float>(x) : nullptr;
    w.part = backward ? c.take<float>(wt * (size_t)wg_slices(g)) : nullptr;
    w.total = c.bytes();
    return w;
}

// One (pixel, tap, deform group) sample: the channels-last row of each of the four corners (-1: contributes nothing), the
// unmodulated bilinear weights, the fractional parts and the mask.  Outside the strict window (-1, H) x (-1, W) every corner
// is -1, which also zeroes the offset and mask gradients there (mmcv's dmcn_get_coordinate_weight).
struct Sample {
    int4 idx;
    float4 w;
    float lh, lw, m;
};

__device__ __forceinline__ Sample sample_at(const Geom &g, const float *offset, const float *mask, int p, int tap, int grp)
{
    Sample s;
    s.idx = make_int4(-1, -1, -1, -1);
    s.w = make_float4(0.f, 0.f, 0.f, 0.f);
    s.lh = s.lw = s.m = 0.f;
    if (p >= g.NP) return s;
    const int n = p / g.HoWo, hw = p - n * g.HoWo, ho = hw / g.Wo, wo = hw - ho * g.Wo;
    const int i = tap / g.kw, j = tap - i * g.kw;
    const size_t ob = ((size_t)n * 2 * g.dg * g.kk + (size_t)grp * 2 * g.kk + 2 * tap) * g.HoWo + hw;
    const float dy = offset[ob], dx = offset[ob + g.HoWo];
    s.m = mask[((size_t)n * g.dg * g.kk + (size_t)grp * g.kk + tap) * g.HoWo + hw];
    // one fp32 add per coordinate: the integer base is exact
    const float y = __fadd_rn((float)(ho * g.sh - g.ph + i * g.dh), dy);
    const float x = __fadd_rn((float)(wo * g.sw - g.pw + j * g.dw), dx);
    if (!(y > -1.f && x > -1.f && y < (float)g.H && x < (float)g.W)) return s;
    const int h0 = (int)floorf(y), w0 = (int)floorf(x), h1 = h0 + 1, w1 = w0 + 1;
    s.lh = y - (float)h0;
    s.lw = x - (float)w0;
    const float hh = 1.f - s.lh, hw_ = 1.f - s.lw;
    s.w = make_float4(hh * hw_, hh * s.lw, s.lh * hw_, s.lh * s.lw);
    const int rb = n * g.H * g.W;
    const bool r0 = h0 >= 0, r1 = h1 <= g.H - 1, c0 = w0 >= 0, c1 = w1 <= g.W - 1;
    s.idx.x = (r0 && c0) ? rb + h0 * g.W + w0 : -1;
    s.idx.y = (r0 && c1) ? rb + h0 * g.W + w1 : -1;
    s.idx.z = (r1 && c0) ? rb + h1 * g.W + w0 : -1;
    s.idx.w = (r1 && c1) ? rb + h1 * g.W + w1 : -1;
    return s;
}

__device__ __forceinline__ float4 ld4(const float *base, int row, int C, int c)
{
    if (row < 0) return make_float4(0.f, 0.f, 0.f, 0.f);
    return *(const float4 *)(base + (size_t)row * C + c);
}

// ---- relayouts -----------------------------------------------------------------------------------------------------------
// dst[b][j][i] = src[b][i][j] for src [B][I][J]; 32 x 32 tiles through LDS, grid (ceil(J/32), ceil(I/32), B)
__global__ __launch_bounds__(kThreads) void gf_dcn_transpose_kernel(const float *__restrict__ src, float *__restrict__ dst, int I,
                                                                     int J)
{
    __shared__ float s[32][33];
    const int b = blockIdx.z, i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float *sb = src + (size_t)b * I * J;
    float *db = dst + (size_t)b * I * J;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = i0 + ty + 8 * k, j = j0 + tx;
        if (i < I && j < J) s[ty + 8 * k][tx] = sb[(size_t)i * J + j];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = j0 + ty + 8 * k, i = i0 + tx;
        if (i < I && j < J) db[(size_t)j * I + i] = s[tx][ty + 8 * k];
    }
}

// weight [Co][C][kk] -> [kk][C][Co] (co_fastest) or [kk][Co][C]
__global__ __launch_bounds__(kThreads) void gf_dcn_weight_kernel(const float *__restrict__ w, float *__restrict__ wr, int Co, int C,
                                                                  int kk, int co_fastest)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= Co * C * kk) return;
    const int co = e / (C * kk), r = e - co * C * kk, c = r / kk, tap = r - c * kk;
    wr[co_fastest ? ((size_t)tap * C + c) * Co + co : ((size_t)tap * Co + co) * C + c] = w[e];
}

// ---- forward -------------------------------------------------------------------------------------------------------------
struct FwdArgs {
    Geom g;
    const float *xn, *offset, *mask, *wr, *bias;
    float *out;
};

__global__ __launch_bounds__(kThreads) void gf_dcn_fwd_kernel(FwdArgs a)
{
    const Geom &g = a.g;
    __shared__ int4 s_idx[kFwdBM];
    __shared__ float4 s_w[kFwdBM];
    __shared__ float s_m[kFwdBM];
    __shared__ float s_col[kGran * kColS];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6;
    const int p0 = blockIdx.x * kFwdBM;
    const int co0 = blockIdx.y * kFwdBN + (wv & 1) * 32;
    const bool co_ok = co0 < g.Co;
    const int pt0 = (wv >> 1) * 64;   // the wave's two 32-pixel tiles: pt0, pt0 + 32
    f32x16 acc0 = {}, acc1 = {};
    for (int tap = 0; tap < g.kk; ++tap) {
        for (int grp = 0; grp < g.dg; ++grp) {
            if (t < kFwdBM) {
                const Sample s = sample_at(g, a.offset, a.mask, p0 + t, tap, grp);
                s_idx[t] = s.idx;
                s_w[t] = s.w;
                s_m[t] = s.m;
            }
            __syncthreads();
            for (int c0 = grp * g.Cg; c0 < (grp + 1) * g.Cg; c0 += kGran) {
                // column tile: s_col[c][p] = (w1 v1 + w2 v2 + w3 v3 + w4 v4) m; eight lanes read one corner row's 128 bytes
                const int c4 = t & 7;
#pragma unroll
                for (int pass = 0; pass < kFwdBM / 32; ++pass) {
                    const int pl = pass * 32 + (t >> 3);
                    const int4 id = s_idx[pl];
                    const float4 w = s_w[pl];
                    const float m = s_m[pl];
                    const int c = c0 + c4 * 4;
                    const float4 v1 = ld4(a.xn, id.x, g.C, c), v2 = ld4(a.xn, id.y, g.C, c);
                    const float4 v3 = ld4(a.xn, id.z, g.C, c), v4 = ld4(a.xn, id.w, g.C, c);
                    s_col[(c4 * 4 + 0) * kColS + pl] = (w.x * v1.x + w.y * v2.x + w.z * v3.x + w.w * v4.x) * m;
                    s_col[(c4 * 4 + 1) * kColS + pl] = (w.x * v1.y + w.y * v2.y + w.z * v3.y + w.w * v4.y) * m;
                    s_col[(c4 * 4 + 2) * kColS + pl] = (w.x * v1.z + w.y * v2.z + w.z * v3.z + w.w * v4.z) * m;
                    s_col[(c4 * 4 + 3) * kColS + pl] = (w.x * v1.w + w.y * v2.w + w.z * v3.w + w.w * v4.w) * m;
                }
                __syncthreads();
                if (co_ok) {
                    // D[co][p] += W[co][c] col[c][p]: A = the weight slice (lane: co0 + l%32, c0 + k), B = the column tile
                    const float *wa = a.wr + ((size_t)tap * g.C + c0 + (l >> 5)) * g.Co + co0 + (l & 31);
                    const float *cb = s_col + (l >> 5) * kColS + pt0 + (l & 31);
#pragma unroll
                    for (int ks = 0; ks < kGran / 2; ++ks) {
                        const float av = wa[(size_t)2 * ks * g.Co];
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, cb[2 * ks * kColS], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, cb[2 * ks * kColS + 32], acc1, 0, 0, 0);
                    }
                }
                __syncthreads();
            }
        }
    }
    if (!co_ok) return;
    // accumulator: column = pixel (lane % 32), row = output channel (r & 3) + 8 (r >> 2) + 4 (lane / 32)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = p0 + pt0 + 32 * h + (l & 31);
        if (p >= g.NP) continue;
        const int n = p / g.HoWo, hw = p - n * g.HoWo;
        float *o = a.out + (size_t)n * g.Co * g.HoWo + hw;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
            const float v = h ? acc1[r] : acc0[r];
            o[(size_t)co * g.HoWo] = a.bias ? v + a.bias[co] : v;
        }
    }
}

// ---- backward: input, offset and mask ------------------------------------------------------------------------------------
struct BwdDataArgs {
    Geom g;
    const float *xn, *offset, *mask, *wrt, *gout;
    float *gin;            // channels-last accumulator or null
    float *goff, *gmask;   // or null
};

__global__ __launch_bounds__(kThreads) void gf_dcn_bwd_data_kernel(BwdDataArgs a)
{
    const Geom &g = a.g;
    constexpr int kPer = kBdBM / 8;   // pixels per thread in the element phase
    __shared__ int4 s_idx[kBdBM];
    __shared__ float4 s_w[kBdBM];
    __shared__ float s_lh[kBdBM], s_lw[kBdBM], s_m[kBdBM];
    __shared__ float s_g[kBdBM * 33];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6;
    const int p0 = blockIdx.x * kBdBM;
    // MFMA phase: the wave's 32 pixels, one per lane % 32
    const int pm = p0 + wv * 32 + (l & 31);
    const bool pm_ok = pm < g.NP;
    const int nm = pm_ok ? pm / g.HoWo : 0;
    const float *gb = a.gout + (size_t)nm * g.Co * g.HoWo + (pm_ok ? pm - nm * g.HoWo : 0);
    // element phase: channel lane c = t % 32, pixels (t / 32) + 8 i
    const int ce = t & 31;
    for (int tap = 0; tap < g.kk; ++tap) {
        for (int grp = 0; grp < g.dg; ++grp) {
            if (t < kBdBM) {
                const Sample s = sample_at(g, a.offset, a.mask, p0 + t, tap, grp);
                s_idx[t] = s.idx;
                s_w[t] = s.w;
                s_lh[t] = s.lh;
                s_lw[t] = s.lw;
                s_m[t] = s.m;
            }
            float am[kPer], ay[kPer], ax[kPer];
#pragma unroll
            for (int i = 0; i < kPer; ++i) am[i] = ay[i] = ax[i] = 0.f;
            for (int c0 = grp * g.Cg; c0 < (grp + 1) * g.Cg; c0 += kGran) {
                // grad_col[c][p] = sum_co W[co][c][tap] grad_out[co][p]: A = W^T (lane: c0 + l%32, co), B = grad_out
                f32x16 acc = {};
                const float *wa = a.wrt + (size_t)tap * g.Co * g.C + (size_t)(l >> 5) * g.C + c0 + (l & 31);
                const float *gp = gb + (size_t)(l >> 5) * g.HoWo;
                for (int k0 = 0; k0 < g.Co; k0 += kGran) {   // Co is a multiple of the granule: 16 steps per pass
                    float av[kGran / 2], bv[kGran / 2];
#pragma unroll
                    for (int ks = 0; ks < kGran / 2; ++ks) {
                        av[ks] = wa[(size_t)(k0 + 2 * ks) * g.C];
                        bv[ks] = pm_ok ? gp[(size_t)(k0 + 2 * ks) * g.HoWo] : 0.f;
                    }
#pragma unroll
                    for (int ks = 0; ks < kGran / 2; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks], bv[ks], acc, 0, 0, 0);
                }
                // accumulator: column = pixel (lane % 32), row = channel (r & 3) + 8 (r >> 2) + 4 (lane / 32)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    s_g[(wv * 32 + (l & 31)) * 33 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)] = acc[r];
                __syncthreads();
                const int c = c0 + ce;
#pragma unroll
                for (int i = 0; i < kPer; ++i) {   // fully unrolled: am / ay / ax stay in registers
                    const int pl = (t >> 5) + 8 * i;
                    const int4 id = s_idx[pl];
                    if ((id.x & id.y & id.z & id.w) < 0) continue;   // no corner in the image: nothing to add
                    const float gc = s_g[pl * 33 + ce];
                    const float4 w = s_w[pl];
                    const float m = s_m[pl], lh = s_lh[pl], lw = s_lw[pl];
                    const float v1 = id.x >= 0 ? a.xn[(size_t)id.x * g.C + c] : 0.f;
                    const float v2 = id.y >= 0 ? a.xn[(size_t)id.y * g.C + c] : 0.f;
                    const float v3 = id.z >= 0 ? a.xn[(size_t)id.z * g.C + c] : 0.f;
                    const float v4 = id.w >= 0 ? a.xn[(size_t)id.w * g.C + c] : 0.f;
                    const float val = w.x * v1 + w.y * v2 + w.z * v3 + w.w * v4;
                    const float wy = -(1.f - lw) * v1 - lw * v2 + (1.f - lw) * v3 + lw * v4;
                    const float wx = -(1.f - lh) * v1 + (1.f - lh) * v2 - lh * v3 + lh * v4;
                    am[i] += gc * val;
                    ay[i] += wy * gc * m;
                    ax[i] += wx * gc * m;
                    if (a.gin) {
                        const float tg = gc * m;
                        if (id.x >= 0) atomicAdd(a.gin + (size_t)id.x * g.C + c, w.x * tg);
                        if (id.y >= 0) atomicAdd(a.gin + (size_t)id.y * g.C + c, w.y * tg);
                        if (id.z >= 0) atomicAdd(a.gin + (size_t)id.z * g.C + c, w.z * tg);
                        if (id.w >= 0) atomicAdd(a.gin + (size_t)id.w * g.C + c, w.w * tg);
                    }
                }
                __syncthreads();
            }
            // fixed-order sum over the 32 channel lanes of each half-wave (per lane the chunks were added in order)
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
#pragma unroll
                for (int o = 16; o >= 1; o >>= 1) {
                    am[i] += __shfl_xor(am[i], o);
                    ay[i] += __shfl_xor(ay[i], o);
                    ax[i] += __shfl_xor(ax[i], o);
                }
                const int p = p0 + (t >> 5) + 8 * i;
                if (ce == 0 && p < g.NP) {
                    const int n = p / g.HoWo, hw = p - n * g.HoWo;
                    if (a.gmask) a.gmask[((size_t)n * g.dg * g.kk + (size_t)grp * g.kk + tap) * g.HoWo + hw] = am[i];
                    if (a.goff) {
                        const size_t ob = ((size_t)n * 2 * g.dg * g.kk + (size_t)grp * 2 * g.kk + 2 * tap) * g.HoWo + hw;
                        a.goff[ob] = ay[i];
                        a.goff[ob + g.HoWo] = ax[i];
                    }
                }
            }
            // the next (tap, group) rewrites s_idx..s_m: every lane has passed the last chunk's trailing barrier
        }
    }
}

// ---- backward: weight ----------------------------------------------------------------------------------------------------
struct BwdWeightArgs {
    Geom g;
    const float *xn, *offset, *mask, *gout;
    float *part;   // [slices][kk][Co][C]
    int per;       // pixels per slice (a multiple of kWgBP)
};

__global__ __launch_bounds__(kThreads) void gf_dcn_bwd_weight_kernel(BwdWeightArgs a)
{
    const Geom &g = a.g;
    __shared__ int4 s_idx[kWgBP];
    __shared__ float4 s_w[kWgBP];
    __shared__ float s_m[kWgBP];
    __shared__ float s_col[kWgBP * 33];      // [p][c]
    __shared__ float s_go[kWgBN * (kWgBP + 1)];   // [co][p]
    const int t = threadIdx.x, l = t & 63, wv = t >> 6;
    const int slice = blockIdx.x;
    const int cot = blockIdx.y;
    const int nchunk = g.C / kGran;
    const int tap = blockIdx.z / nchunk, c0 = (blockIdx.z - tap * nchunk) * kGran;
    const int grp = c0 / g.Cg;
    const int co0 = cot * kWgBN + wv * 32;
    const bool co_ok = co0 < g.Co;
    const int pb0 = slice * a.per, pb1 = min(g.NP, pb0 + a.per);
    f32x16 acc = {};
    for (int pb = pb0; pb < pb1; pb += kWgBP) {
        if (t < kWgBP) {
            const Sample s = sample_at(g, a.offset, a.mask, pb + t < pb1 ? pb + t : g.NP, tap, grp);
            s_idx[t] = s.idx;
            s_w[t] = s.w;
            s_m[t] = s.m;
        }
        {   // grad_out [co][p], coalesced along the pixels
            const int pl = t & 63, p = pb + pl;
            const bool ok = p < pb1;
            const int n = ok ? p / g.HoWo : 0;
            const float *src = a.gout + (size_t)n * g.Co * g.HoWo + (ok ? p - n * g.HoWo : 0);
#pragma unroll 8
            for (int r = t >> 6; r < kWgBN; r += 4) {
                const int co = cot * kWgBN + r;
                s_go[r * (kWgBP + 1) + pl] = (ok && co < g.Co) ? src[(size_t)co * g.HoWo] : 0.f;
            }
        }
        __syncthreads();
        {   // columns [p][c] of this tap and chunk
            const int c4 = t & 7;
#pragma unroll
            for (int pass = 0; pass < kWgBP / 32; ++pass) {
                const int pl = pass * 32 + (t >> 3);
                const int4 id = s_idx[pl];
                const float4 w = s_w[pl];
                const float m = s_m[pl];
                const int c = c0 + c4 * 4;
                const float4 v1 = ld4(a.xn, id.x, g.C, c), v2 = ld4(a.xn, id.y, g.C, c);
                const float4 v3 = ld4(a.xn, id.z, g.C, c), v4 = ld4(a.xn, id.w, g.C, c);
                float *d = s_col + pl * 33 + c4 * 4;
                d[0] = (w.x * v1.x + w.y * v2.x + w.z * v3.x + w.w * v4.x) * m;
                d[1] = (w.x * v1.y + w.y * v2.y + w.z * v3.y + w.w * v4.y) * m;
                d[2] = (w.x * v1.z + w.y * v2.z + w.z * v3.z + w.w * v4.z) * m;
                d[3] = (w.x * v1.w + w.y * v2.w + w.z * v3.w + w.w * v4.w) * m;
            }
        }
        __syncthreads();
        if (co_ok) {
            // D[co][c] += sum_p grad_out[co][p] col[p][c]: A = s_go (lane: co0 + l%32, p), B = s_col (lane: p, c0 + l%32)
            const float *ga = s_go + (wv * 32 + (l & 31)) * (kWgBP + 1) + (l >> 5);
            const float *cb = s_col + (l >> 5) * 33 + (l & 31);
#pragma unroll
            for (int ks = 0; ks < kWgBP / 2; ++ks)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[2 * ks], cb[2 * ks * 33], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    if (!co_ok) return;
    float *pp = a.part + (((size_t)slice * g.kk + tap) * g.Co) * g.C + c0 + (l & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) pp[(size_t)(co0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)) * g.C] = acc[r];
}

// grad_weight [Co][C][kk] = sum over slices, in slice order
__global__ __launch_bounds__(kThreads) void gf_dcn_wgrad_sum_kernel(const float *__restrict__ part, float *__restrict__ gw, int Co,
                                                                     int C, int kk, int slices)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= Co * C * kk) return;
    const int co = e / (C * kk), r = e - co * C * kk, c = r / kk, tap = r - c * kk;
    const size_t stride = (size_t)kk * Co * C;
    const float *p = part + ((size_t)tap * Co + co) * C + c;
    float s = 0.f;
    for (int k = 0; k < slices; ++k) s += p[k * stride];
    gw[e] = s;
}

// grad_bias[co] = sum over n and pixels of grad_out[n][co][.], fixed-order tree
__global__ __launch_bounds__(kThreads) void gf_dcn_bias_kernel(const float *__restrict__ gout, float *__restrict__ gbias, int N,
                                                                int Co, int HoWo)
{
    __shared__ float s[kThreads];
    const int co = blockIdx.x, t = threadIdx.x;
    float acc = 0.f;
    for (int n = 0; n < N; ++n) {
        const float *src = gout + ((size_t)n * Co + co) * HoWo;
        for (int i = t; i < HoWo; i += kThreads) acc += src[i];
    }
    s[t] = acc;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (t < o) s[t] += s[t + o];
        __syncthreads();
    }
    if (t == 0) gbias[co] = s[0];
}

// ---- host ----------------------------------------------------------------------------------------------------------------
static int make_geom(const char *fn, Geom *g, int N, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                     int dh, int dw, int groups, int dg)
{
    if (groups != 1) { set_error("%s: groups = %d; only groups = 1 is supported", fn, groups); return GF_EINVAL; }
    if (N < 0 || H < 1 || W < 1) { set_error("%s: N = %d, H = %d, W = %d; N >= 0, H >= 1, W >= 1", fn, N, H, W); return GF_EINVAL; }
    if (kh < 1 || kw < 1 || kh > GF_DCN_MAX_KERNEL || kw > GF_DCN_MAX_KERNEL) {
        set_error("%s: kernel %d x %d; each side in 1..%d", fn, kh, kw, GF_DCN_MAX_KERNEL);
        return GF_EINVAL;
    }
    if (sh < 1 || sw < 1 || dh < 1 || dw < 1 || ph < 0 || pw < 0) {
        set_error("%s: stride (%d, %d), dilation (%d, %d) >= 1 and padding (%d, %d) >= 0 needed", fn, sh, sw, dh, dw, ph, pw);
        return GF_EINVAL;
    }
    if (dg < 1 || C < 1 || C % dg != 0) { set_error("%s: deform_groups = %d must divide Cin = %d", fn, dg, C); return GF_EINVAL; }
    if ((C / dg) % GF_DCN_CHANNEL_GRANULE != 0 || Co < 1 || Co % GF_DCN_CHANNEL_GRANULE != 0) {
        set_error("%s: Cin / deform_groups = %d and Cout = %d must be multiples of %d", fn, C / dg, Co, GF_DCN_CHANNEL_GRANULE);
        return GF_EINVAL;
    }
    const int Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1, Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
    if (H + 2 * ph < dh * (kh - 1) + 1 || W + 2 * pw < dw * (kw - 1) + 1 || Ho < 1 || Wo < 1) {
        set_error("%s: empty output (%d x %d input, kernel %d x %d, padding (%d, %d), dilation (%d, %d))", fn, H, W, kh, kw, ph, pw,
                  dh, dw);
        return GF_EINVAL;
    }
    const long long lim = 1ll << 31;
    if ((long long)N * C * H * W >= lim || (long long)N * Co * Ho * Wo >= lim || (long long)N * 2 * dg * kh * kw * Ho * Wo >= lim ||
        (long long)kWgMaxSlices * kh * kw * C * Co >= lim) {
        set_error("%s: tensors of 2^31 elements or more", fn);
        return GF_EINVAL;
    }
    *g = Geom{N, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg, Ho, Wo, Ho * Wo, N * Ho * Wo, C / dg, kh * kw};
    return GF_OK;
}

static void relayout(const Geom &g, const float *input, const float *weight, const Ws &w, int co_fastest, hipStream_t stream)
{
    if (g.N > 0)
        hipLaunchKernelGGL(gf_dcn_transpose_kernel, dim3((g.H * g.W + 31) / 32, (g.C + 31) / 32, g.N), dim3(kThreads), 0, stream,
                           input, w.xn, g.C, g.H * g.W);
    const int nw = g.Co * g.C * g.kk;
    hipLaunchKernelGGL(gf_dcn_weight_kernel, dim3((nw + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, weight, w.wr, g.Co,
                       g.C, g.kk, co_fastest);
}

}  // namespace dcn
}  // namespace gf

#define GF_DCN_GEOM_ARGS N, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, groups, dg

extern "C" size_t gf_dcn_workspace_bytes(int N, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                                         int dw, int groups, int dg, int backward)
{
    gf::dcn::Geom g;
    if (gf::dcn::make_geom(__func__, &g, GF_DCN_GEOM_ARGS) != GF_OK) return 0;
    return gf::dcn::carve(nullptr, g, backward ? 1 : 0).total;
}

extern "C" int gf_dcn_forward(int N, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                              int groups, int dg, const float *input, const float *offset, const float *mask, const float *weight,
                              const float *bias, float *out, void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace gf;
    using namespace gf::dcn;
    Geom g;
    int rc = make_geom(__func__, &g, GF_DCN_GEOM_ARGS);
    if (rc != GF_OK) return rc;
    GF_CHECK_ARG(weight, "null weight");
    GF_CHECK_ARG(N == 0 || (input && offset && mask && out), "null input, offset, mask or output");
    const Ws w = carve(workspace, g, 0);
    if (!workspace) return refuse_workspace(__func__, "workspace", workspace_bytes, w.total);  // (a null one: refused like a short one)
    GF_CHECK_WORKSPACE(workspace_bytes, w.total);
    if (N == 0) return GF_OK;
    const hipStream_t stream = (hipStream_t)stream_;
    relayout(g, input, weight, w, 1, stream);
    FwdArgs a{g, w.xn, offset, mask, w.wr, bias, out};
    hipLaunchKernelGGL(gf_dcn_fwd_kernel, dim3((g.NP + kFwdBM - 1) / kFwdBM, (g.Co + kFwdBN - 1) / kFwdBN), dim3(kThreads), 0,
                       stream, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_dcn_backward(int N, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                               int groups, int dg, const float *input, const float *offset, const float *mask, const float *weight,
                               const float *grad_out, float *grad_input, float *grad_offset, float *grad_mask, float *grad_weight,
                               float *grad_bias, void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace gf;
    using namespace gf::dcn;
    Geom g;
    int rc = make_geom(__func__, &g, GF_DCN_GEOM_ARGS);
    if (rc != GF_OK) return rc;
    GF_CHECK_ARG(weight, "null weight");
    GF_CHECK_ARG(N == 0 || (input && offset && mask && grad_out), "null input, offset, mask or grad_out");
    const Ws w = carve(workspace, g, 1);
    if (!workspace) return refuse_workspace(__func__, "workspace", workspace_bytes, w.total);  // (a null one: refused like a short one)
    GF_CHECK_WORKSPACE(workspace_bytes, w.total);
    const hipStream_t stream = (hipStream_t)stream_;
    if (N == 0) {
        if ((grad_weight && hipMemsetAsync(grad_weight, 0, (size_t)Co * C * kh * kw * 4, stream) != hipSuccess) ||
            (grad_bias && hipMemsetAsync(grad_bias, 0, (size_t)Co * 4, stream) != hipSuccess)) {
            set_error("%s: hipMemsetAsync failed", __func__);
            return GF_ELAUNCH;
        }
        return GF_OK;
    }
    relayout(g, input, weight, w, 0, stream);
    if (grad_input || grad_offset || grad_mask) {
        if (grad_input && hipMemsetAsync(w.gin, 0, (size_t)N * H * W * C * 4, stream) != hipSuccess) {
            set_error("%s: hipMemsetAsync failed", __func__);
            return GF_ELAUNCH;
        }
        BwdDataArgs a{g, w.xn, offset, mask, w.wr, grad_out, grad_input ? w.gin : nullptr, grad_offset, grad_mask};
        hipLaunchKernelGGL(gf_dcn_bwd_data_kernel, dim3((g.NP + kBdBM - 1) / kBdBM), dim3(kThreads), 0, stream, a);
        if (grad_input)
            hipLaunchKernelGGL(gf_dcn_transpose_kernel, dim3((C + 31) / 32, (H * W + 31) / 32, N), dim3(kThreads), 0, stream, w.gin,
                               grad_input, H * W, C);
    }
    if (grad_weight) {
        const int slices = wg_slices(g);
        const int per = (((g.NP + slices - 1) / slices) + kWgBP - 1) / kWgBP * kWgBP;
        BwdWeightArgs a{g, w.xn, offset, mask, grad_out, w.part, per};
        hipLaunchKernelGGL(gf_dcn_bwd_weight_kernel, dim3(slices, (Co + kWgBN - 1) / kWgBN, g.kk * (C / kGran)), dim3(kThreads), 0,
                           stream, a);
        const int nw = Co * C * g.kk;
        hipLaunchKernelGGL(gf_dcn_wgrad_sum_kernel, dim3((nw + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, w.part,
                           grad_weight, Co, C, g.kk, slices);
    }
    if (grad_bias) hipLaunchKernelGGL(gf_dcn_bias_kernel, dim3(Co), dim3(kThreads), 0, stream, grad_out, grad_bias, N, Co, g.HoWo);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
