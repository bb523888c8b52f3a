// GaussianLifterV2's per-frame pixel work (model/lifter/gaussian_lifter_v2.py:169-233, model/utils/sampler.py) and
// PixelDistributionLoss (loss/bce_loss.py:60-87).  The contract: include/gf_hip.h and gaussianformer_amd/lifter.py; the
// design and the measured numbers: DESIGN.md §3.10.
//
// Lifting, three launches, no host synchronisation, no float atomics:
//   lift      one wave per pixel (16 pixels per wave, 64 per workgroup): reads the pixel's S + 1 logits once (entry
//             e = lane + 64 r), softmax, argmax of the pdf (ties to the lower index), the normalised cdf by a wave scan in a
//             fixed lane order, and per sample the searchsorted count (stochastic) or the top-a choice (deterministic).  Only
//             the chosen bin's point is evaluated for the candidate; it goes to the workspace with a keep byte, and the
//             workgroup's keep count to blk.  With pixel_gt, every one of the S points is evaluated and looked up in the
//             packed occupancy table, and the S + 1 bytes are written
//   scan      one workgroup per batch element: exclusive scan of the workgroup counts -> offsets; counts[b]
//   write     per lift workgroup: a workgroup scan of the keep bytes in slot order places each candidate at its offset (row-
//             major (camera, row, column, sample) order is kept); the slots that are not candidates fill the padding behind
//             counts[b] in the same order (points 0, src -1), so every output element has exactly one writer
// Pixel loss: one wave per pixel row; the forward leaves one fp64 partial per workgroup and a one-workgroup finalise sums them
// in a fixed order (bitwise reproducible); the backward is one pass that writes every element of grad_logits.
#include <float.h>

#include "gf_common.hpp"

namespace gf {
namespace lift {   // a named namespace: every kernel has external linkage and a stable name

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPixPerWave = 16;     // measured against 1 and 4: 16 is the fastest whole call
constexpr int kPixPerBlock = kWaves * kPixPerWave;   // 64 pixels per workgroup
constexpr int kFin = 256;

inline int num_blocks(int npix) { return (npix + kPixPerBlock - 1) / kPixPerBlock; }

struct LiftParams {
    int npix, hw, w, h, S, a;
    float pc[6], vs;
    int X, Y, Z;
    const float *logits;         // [b][npix][S + 1]
    const float *img2lidar;      // [b][n][4][4]
    const float *image_wh;       // [b][n][2]
    const float *depth;          // [S]
    const unsigned char *occ;    // [b][X][Y][Z] or null
    const float *uniforms;       // [b][npix][a] or null (top-a)
    unsigned char *gt;           // [b][npix][S + 1] or null
    float *pts;                  // workspace [b][npix * a][3]
    unsigned char *keep;         // workspace [b][npix * a]
    int *blk;                    // workspace [b][nblk]
};

// the workspace's size; with a base, its sections as the kernels' parameters hold them
inline size_t carve(LiftParams *p, void *base, int b, int npix, int a)
{
    const size_t slots = (size_t)b * npix * a, nb = (size_t)b * num_blocks(npix);
    Carver c(base);
    float *pts = c.take<float>(slots * 3);
    unsigned char *keep = c.take<unsigned char>(slots);
    int *blk = c.take<int>(nb);
    if (p) { p->pts = pts; p->keep = keep; p->blk = blk; }
    return c.bytes();
}

// img2lidar @ (u d, v d, d, 1), first three rows
__device__ __forceinline__ void lift_point(const float *M, float ud, float vd, float d, float &x, float &y, float &z)
{
    x = M[0] * ud + M[1] * vd + M[2] * d + M[3];
    y = M[4] * ud + M[5] * vd + M[6] * d + M[7];
    z = M[8] * ud + M[9] * vd + M[10] * d + M[11];
}

__device__ __forceinline__ bool in_range(const LiftParams &a, float x, float y, float z)
{
    return x >= a.pc[0] && x < a.pc[3] && y >= a.pc[1] && y < a.pc[4] && z >= a.pc[2] && z < a.pc[5];
}

__device__ __forceinline__ int voxel(float p, float lo, float vs, int n)
{
    int i = (int)((p - lo) / vs);   // truncation, as .to(torch.int)
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// R = ceil((S + 1) / 64) entries per lane
template <int R>
__global__ void __launch_bounds__(kThreads) gf_lift_kernel(LiftParams a)
{
    __shared__ int wave_count[kWaves];
    const int bi = blockIdx.y, lane = lane_id(), wave = threadIdx.x >> 6;
    const int nb = a.S + 1;
    int count = 0;
    for (int t = 0; t < kPixPerWave; ++t) {
        const int q = blockIdx.x * kPixPerBlock + wave * kPixPerWave + t;
        if (q >= a.npix) break;   // wave-uniform
        const size_t pix = (size_t)bi * a.npix + q;
        const float *row = a.logits + pix * nb;
        float x[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = lane + 64 * r;
            x[r] = e < nb ? row[e] : -INFINITY;
        }
        // softmax over the S + 1 entries
        float m = x[0];
#pragma unroll
        for (int r = 1; r < R; ++r) m = fmaxf(m, x[r]);
        m = wave_xor_reduce(m, Max());
        float p[R], s = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            p[r] = lane + 64 * r < nb ? expf(x[r] - m) : 0.f;
            s += p[r];
        }
        s = wave_xor_reduce(s, Sum());
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            p[r] = p[r] / s;
            ps += p[r];
        }
        // argmax of the pdf, ties to the lower index; disables the pixel when it is the "no surface" bin S
        float bv = -1.f;
        int bidx = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (lane + 64 * r < nb && p[r] > bv) { bv = p[r]; bidx = lane + 64 * r; }
        wave_argmax(bv, bidx);
        const bool disabled = bidx == a.S;

        // camera of this pixel and its ray
        const int cam = q / a.hw, rem = q - cam * a.hw, ri = rem / a.w, cj = rem - ri * a.w;
        const float *M = a.img2lidar + ((size_t)bi * (a.npix / a.hw) + cam) * 16;
        const float *wh = a.image_wh + ((size_t)bi * (a.npix / a.hw) + cam) * 2;
        const float U = ((float)cj + 0.5f) / (float)a.w * wh[0];
        const float V = ((float)ri + 0.5f) / (float)a.h * wh[1];

        float cdf[R];
        if (a.uniforms) {
            // normalised pdf p / (eps + sum p), cdf by a wave scan per 64-entry chunk (fixed order)
            ps = wave_xor_reduce(ps, Sum());
            const float den = FLT_EPSILON + ps;
            float carry = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float incl = wave_incl_scan_shfl(p[r] / den) + carry;
                cdf[r] = incl;
                carry = __shfl(incl, 63, 64);
            }
        }
        unsigned taken = 0;   // deterministic: entries already chosen (bit r of lane l = entry l + 64 r)
        for (int j = 0; j < a.a; ++j) {
            int idx;
            if (a.uniforms) {
                const float u = a.uniforms[pix * a.a + j];
                int c = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) c += __popcll(__ballot(lane + 64 * r < nb && cdf[r] <= u));
                idx = c < a.S ? c : a.S;   // searchsorted(right=True).clip(max=S)
            } else if (j == 0) {
                idx = bidx;                // top-a of the pdf in descending order, ties to the lower index
            } else {
                float v = -1.f;
                idx = 0x7fffffff;
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (lane + 64 * r < nb && !(taken >> r & 1u) && p[r] > v) { v = p[r]; idx = lane + 64 * r; }
                wave_argmax(v, idx);
            }
            if ((idx & 63) == lane && idx < 64 * R) taken |= 1u << (idx >> 6);
            const int k = idx < a.S - 1 ? idx : a.S - 1;
            const float d = a.depth[k];
            float px, py, pz;
            lift_point(M, U * d, V * d, d, px, py, pz);
            const bool keep = !disabled && in_range(a, px, py, pz);
            count += keep;
            if (lane == j) {
                const size_t slot = pix * a.a + j;
                a.pts[slot * 3 + 0] = px;
                a.pts[slot * 3 + 1] = py;
                a.pts[slot * 3 + 2] = pz;
                a.keep[slot] = keep;
            }
        }

        if (a.gt) {
            const unsigned char *occ = a.occ + (size_t)bi * a.X * a.Y * a.Z;
            unsigned char *g = a.gt + pix * nb;
            bool any = false;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int k = lane + 64 * r;
                bool hit = false;
                if (k < a.S) {
                    const float d = a.depth[k];
                    float px, py, pz;
                    lift_point(M, U * d, V * d, d, px, py, pz);
                    if (in_range(a, px, py, pz)) {
                        const int ix = voxel(px, a.pc[0], a.vs, a.X), iy = voxel(py, a.pc[1], a.vs, a.Y),
                                  iz = voxel(pz, a.pc[2], a.vs, a.Z);
                        hit = occ[((size_t)ix * a.Y + iy) * a.Z + iz] != 0;
                    }
                    g[k] = hit;
                }
                any = any || __ballot(hit) != 0ull;
            }
            if (lane == (a.S & 63)) g[a.S] = !any;
        }
    }
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) c += wave_count[i];
        a.blk[(size_t)bi * gridDim.x + blockIdx.x] = c;
    }
}

// one workgroup per batch element: workgroup counts -> exclusive offsets, counts[b] = total
__global__ void __launch_bounds__(kThreads) gf_lift_scan_kernel(int nblk, int *blk, int *counts)
{
    __shared__ int lds[kWaves];
    int *c = blk + (size_t)blockIdx.x * nblk;
    int carry = 0;
    for (int base = 0; base < nblk; base += kThreads) {
        const int i = base + threadIdx.x;
        const int v = i < nblk ? c[i] : 0;
        int total;
        const int ex = block_excl_scan<kWaves>(v, lds, total);
        if (i < nblk) c[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kThreads) gf_lift_write_kernel(int npix, int A, const float *pts, const unsigned char *keep,
                                                                 const int *blk, const int *counts, float *points, int *src)
{
    __shared__ int lds[kWaves];
    const int bi = blockIdx.y;
    const long long per = (long long)npix * A;
    const long long s0 = (long long)blockIdx.x * kPixPerBlock * A;
    const long long s1 = min(per, s0 + (long long)kPixPerBlock * A);
    const long long off = blk[(size_t)bi * gridDim.x + blockIdx.x];
    const long long total = counts[bi];
    const size_t base = (size_t)bi * per;
    long long kept = 0;
    for (long long c0 = s0; c0 < s1; c0 += kThreads) {
        const long long s = c0 + threadIdx.x;
        const int k = s < s1 ? keep[base + s] : 0;
        int tot;
        const int ex = block_excl_scan<kWaves>(k, lds, tot);
        if (s < s1) {
            // candidates in slot order at off + ..., the other slots in slot order behind all candidates
            const long long pos = k ? off + kept + ex : total + s - (off + kept + ex);
            float *o = points + (base + pos) * 3;
            o[0] = k ? pts[(base + s) * 3 + 0] : 0.f;
            o[1] = k ? pts[(base + s) * 3 + 1] : 0.f;
            o[2] = k ? pts[(base + s) * 3 + 2] : 0.f;
            if (src) src[base + pos] = k ? (int)s : -1;
        }
        kept += tot;
    }
}

// ---- pixel loss ------------------------------------------------------------------------------------------------------
struct LossParams {
    int rows, nb, flags;
    const float *logits;        // [rows][nb]
    const unsigned char *gt;    // [rows][nb]
};

// p of the R entries of a lane (softmax over the row, or the elementwise sigmoid); entries past the row give 0
template <int R>
__device__ __forceinline__ void row_probs(const LossParams &a, const float *row, float p[R])
{
    const int lane = lane_id();
    if (a.flags & GF_PIXEL_LOSS_SOFTMAX) {
        float x[R], m = -INFINITY;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            x[r] = lane + 64 * r < a.nb ? row[lane + 64 * r] : -INFINITY;
            m = fmaxf(m, x[r]);
        }
        m = wave_xor_reduce(m, Max());
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            p[r] = lane + 64 * r < a.nb ? expf(x[r] - m) : 0.f;
            s += p[r];
        }
        s = wave_xor_reduce(s, Sum());
#pragma unroll
        for (int r = 0; r < R; ++r) p[r] = p[r] / s;
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) p[r] = lane + 64 * r < a.nb ? 1.f / (1.f + expf(-row[lane + 64 * r])) : 0.f;
    }
}

template <int R>
__global__ void __launch_bounds__(kThreads) gf_pixel_loss_fwd_kernel(LossParams a, double *part)
{
    __shared__ double lds[kWaves];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    double acc = 0.0;
    for (int t = 0; t < kPixPerWave; ++t) {
        const long long q = (long long)blockIdx.x * kPixPerBlock + wave * kPixPerWave + t;
        if (q >= a.rows) break;
        const float *row = a.logits + q * a.nb;
        const unsigned char *g = a.gt + q * a.nb;
        float p[R];
        row_probs<R>(a, row, p);
        float rs = 0.f;   // per lane: at most R terms of this row
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = lane + 64 * r;
            if (e < a.nb) {
                // torch's binary_cross_entropy: -(t log p + (1 - t) log1p(-p)), each log clamped at -100
                const float l = g[e] ? fmaxf(logf(p[r]), -100.f) : fmaxf(log1pf(-p[r]), -100.f);
                rs -= l;
            }
        }
        acc += (double)rs;
    }
    acc = wave_xor_reduce(acc, Sum());
    if (lane == 0) lds[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) s += lds[i];
        part[blockIdx.x] = s;
    }
}

// one workgroup: the fixed-order sum of the partials; loss = sum / numel in fp32
__global__ void __launch_bounds__(kFin) gf_pixel_loss_finalise_kernel(int nparts, const double *part, double numel, float *loss)
{
    __shared__ double lds[kFin];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kFin) s += part[i];
    lds[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int st = kFin / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) lds[threadIdx.x] += lds[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(lds[0] / numel);
}

template <int R>
__global__ void __launch_bounds__(kThreads) gf_pixel_loss_bwd_kernel(LossParams a, const float *grad_loss, float numel,
                                                                     float *grad)
{
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const float gl = *grad_loss;
    for (int t = 0; t < kPixPerWave; ++t) {
        const long long q = (long long)blockIdx.x * kPixPerBlock + wave * kPixPerWave + t;
        if (q >= a.rows) break;
        const float *row = a.logits + q * a.nb;
        const unsigned char *g = a.gt + q * a.nb;
        float p[R], gp[R];
        row_probs<R>(a, row, p);
        float dot = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = lane + 64 * r;
            // torch's BCE backward: grad * (p - t) / max((1 - p) p, 1e-12), then / numel (mean)
            gp[r] = e < a.nb ? gl * (p[r] - (g[e] ? 1.f : 0.f)) / fmaxf((1.f - p[r]) * p[r], 1e-12f) / numel : 0.f;
            dot += gp[r] * p[r];
        }
        float *o = grad + q * a.nb;
        if (a.flags & GF_PIXEL_LOSS_SOFTMAX) {
            dot = wave_xor_reduce(dot, Sum());
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (lane + 64 * r < a.nb) o[lane + 64 * r] = p[r] * (gp[r] - dot);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (lane + 64 * r < a.nb) o[lane + 64 * r] = gp[r] * (1.f - p[r]) * p[r];
        }
    }
}

inline int loss_parts(int rows) { return (rows + kPixPerBlock - 1) / kPixPerBlock; }
inline double *loss_carve(Carver &c, int rows) { return c.take<double>((size_t)loss_parts(rows)); }  // the pixel loss's workspace: a partial sum per block

int check_loss(const char *fn, int rows, int nb, int flags, const float *logits, const unsigned char *gt)
{
    if (rows < 1) { set_error("%s: rows = %d; rows >= 1", fn, rows); return GF_EINVAL; }
    if (nb < 1 || nb > GF_LIFT_MAX_BINS) { set_error("%s: bins = %d; 1 <= bins <= %d", fn, nb, GF_LIFT_MAX_BINS); return GF_EINVAL; }
    if (flags != GF_PIXEL_LOSS_SOFTMAX && flags != GF_PIXEL_LOSS_SIGMOID) {
        set_error("%s: flags 0x%x; exactly one of GF_PIXEL_LOSS_SOFTMAX and GF_PIXEL_LOSS_SIGMOID", fn, flags);
        return GF_EINVAL;
    }
    if ((long long)rows * nb >= (1ll << 40)) { set_error("%s: rows x bins too large", fn); return GF_EINVAL; }
    if (!logits || !gt) { set_error("%s: null pointer", fn); return GF_EINVAL; }
    return GF_OK;
}

#define GF_LIFT_DISPATCH(R_, launch) \
    switch (R_) {                     \
    case 1: launch(1); break;         \
    case 2: launch(2); break;         \
    case 3: launch(3); break;         \
    default: launch(4); break;        \
    }

}  // namespace lift
}  // namespace gf

extern "C" size_t gf_lift_workspace_bytes(int b, int npix, int a)
{
    if (b < 1 || npix < 1 || a < 1 || a > GF_LIFT_MAX_ANCHORS || (long long)npix * a >= (1ll << 31)) return 0;
    return gf::lift::carve(nullptr, nullptr, b, npix, a);
}

extern "C" int gf_lift_pixels(int b, int n, int h, int w, int S, int a, const float *logits, const float *img2lidar,
                              const float *image_wh, const float *depth_bins, const float *pc_range_host, float voxel_size,
                              int X, int Y, int Z, const unsigned char *occ, const float *uniforms, float *points, int *counts,
                              int *src, unsigned char *pixel_gt, void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace gf;
    using namespace gf::lift;
    if (b < 1 || b > 65535 || n < 1 || h < 1 || w < 1) {
        set_error("%s: b = %d, n = %d, h = %d, w = %d; each >= 1, b <= 65535", __func__, b, n, h, w);
        return GF_EINVAL;
    }
    if ((long long)n * h * w >= (1ll << 31)) { set_error("%s: n x h x w too large", __func__); return GF_EINVAL; }
    const int npix = n * h * w;
    if (S < 1 || S + 1 > GF_LIFT_MAX_BINS) {
        set_error("%s: S = %d; 1 <= S and S + 1 <= %d", __func__, S, GF_LIFT_MAX_BINS);
        return GF_EINVAL;
    }
    if (a < 1 || a > GF_LIFT_MAX_ANCHORS || a > S + 1) {
        set_error("%s: anchors_per_pixel = %d; 1 <= a <= %d and a <= S + 1", __func__, a, GF_LIFT_MAX_ANCHORS);
        return GF_EINVAL;
    }
    if ((long long)npix * a >= (1ll << 31)) { set_error("%s: n x h x w x a too large", __func__); return GF_EINVAL; }
    GF_CHECK_ARG(logits && img2lidar && image_wh && depth_bins && pc_range_host, "null input pointer");
    GF_CHECK_ARG((points == nullptr) == (counts == nullptr), "points and counts must be given together");
    GF_CHECK_ARG(!src || points, "src needs points");
    GF_CHECK_ARG(points || pixel_gt, "nothing to compute (points and pixel_gt both null)");
    GF_CHECK_ARG(workspace, "null workspace");
    for (int i = 0; i < 3; ++i)
        if (!(pc_range_host[i] < pc_range_host[i + 3])) {
            set_error("%s: pc_range axis %d: min %g must be below max %g", __func__, i, pc_range_host[i], pc_range_host[i + 3]);
            return GF_EINVAL;
        }
    if (pixel_gt) {
        GF_CHECK_ARG(occ, "pixel_gt needs the packed occupancy table");
        if (!(voxel_size > 0.f) || X < 1 || Y < 1 || Z < 1 || (long long)X * Y * Z >= (1ll << 31)) {
            set_error("%s: voxel_size = %g, grid %d x %d x %d; a positive size and grid needed", __func__, voxel_size, X, Y, Z);
            return GF_EINVAL;
        }
    }
    LiftParams p{};
    const size_t need = carve(&p, workspace, b, npix, a);
    GF_CHECK_WORKSPACE(workspace_bytes, need);
    p.npix = npix; p.hw = h * w; p.w = w; p.h = h; p.S = S; p.a = a;
    for (int i = 0; i < 6; ++i) p.pc[i] = pc_range_host[i];
    p.vs = voxel_size; p.X = X; p.Y = Y; p.Z = Z;
    p.logits = logits; p.img2lidar = img2lidar; p.image_wh = image_wh; p.depth = depth_bins;
    p.occ = occ; p.uniforms = uniforms; p.gt = pixel_gt;
    const hipStream_t stream = (hipStream_t)stream_;
    const int nblk = num_blocks(npix), R = (S + 1 + 63) / 64;
#define GF_LIFT_LAUNCH(r) hipLaunchKernelGGL(gf_lift_kernel<r>, dim3(nblk, b), dim3(kThreads), 0, stream, p)
    GF_LIFT_DISPATCH(R, GF_LIFT_LAUNCH)
#undef GF_LIFT_LAUNCH
    if (points) {
        hipLaunchKernelGGL(gf_lift_scan_kernel, dim3(b), dim3(kThreads), 0, stream, nblk, p.blk, counts);
        hipLaunchKernelGGL(gf_lift_write_kernel, dim3(nblk, b), dim3(kThreads), 0, stream, npix, a, p.pts, p.keep, p.blk,
                           counts, points, src);
    }
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" size_t gf_pixel_loss_workspace_bytes(int rows, int bins)
{
    if (rows < 1 || bins < 1 || bins > GF_LIFT_MAX_BINS) return 0;
    gf::Carver c(nullptr);
    gf::lift::loss_carve(c, rows);
    return c.bytes();
}

extern "C" int gf_pixel_loss_forward(int rows, int bins, int flags, const float *logits, const unsigned char *pixel_gt,
                                     float *loss, void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace gf;
    using namespace gf::lift;
    int rc = check_loss(__func__, rows, bins, flags, logits, pixel_gt);
    if (rc != GF_OK) return rc;
    GF_CHECK_ARG(loss && workspace, "null loss or workspace pointer");
    Carver c(workspace);
    double *part = loss_carve(c, rows);
    GF_CHECK_WORKSPACE(workspace_bytes, c.bytes());
    const hipStream_t stream = (hipStream_t)stream_;
    const LossParams a{rows, bins, flags, logits, pixel_gt};
    const int np = loss_parts(rows), R = (bins + 63) / 64;
#define GF_LOSS_FWD(r) hipLaunchKernelGGL(gf_pixel_loss_fwd_kernel<r>, dim3(np), dim3(kThreads), 0, stream, a, part)
    GF_LIFT_DISPATCH(R, GF_LOSS_FWD)
#undef GF_LOSS_FWD
    hipLaunchKernelGGL(gf_pixel_loss_finalise_kernel, dim3(1), dim3(kFin), 0, stream, np, part, (double)rows * bins, loss);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_pixel_loss_backward(int rows, int bins, int flags, const float *logits, const unsigned char *pixel_gt,
                                      const float *grad_loss, float *grad_logits, void *stream_)
{
    using namespace gf;
    using namespace gf::lift;
    int rc = check_loss(__func__, rows, bins, flags, logits, pixel_gt);
    if (rc != GF_OK) return rc;
    GF_CHECK_ARG(grad_loss && grad_logits, "null gradient pointer");
    const hipStream_t stream = (hipStream_t)stream_;
    const LossParams a{rows, bins, flags, logits, pixel_gt};
    const int np = loss_parts(rows), R = (bins + 63) / 64;
    const float numel = (float)((double)rows * bins);
#define GF_LOSS_BWD(r) \
    hipLaunchKernelGGL(gf_pixel_loss_bwd_kernel<r>, dim3(np), dim3(kThreads), 0, stream, a, grad_loss, numel, grad_logits)
    GF_LIFT_DISPATCH(R, GF_LOSS_BWD)
#undef GF_LOSS_BWD
    GF_CHECK_LAUNCH();
    return GF_OK;
}
