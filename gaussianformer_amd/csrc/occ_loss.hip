// Occupancy loss: what OccupancyLoss.loss_voxel (loss/occupancy_loss.py:104-149) computes for the shipped configs -- weighted
// cross-entropy + Lovász-softmax (loss/utils/lovasz_softmax.py:157-204) over L decoder layers -- with its backward.  The
// contract: include/gf_hip.h and gaussianformer_amd/occupancy_loss.py; the algorithm and the measured numbers: DESIGN.md §3.9.
//
// Forward, one stream, kernels only (no host synchronisation, no memset):
//   clear     zeroes the header words
//   prep      per voxel: mask / empty / label checks, Lovász keep flag; per-workgroup keep counts and class counts
//   offsets   one workgroup: exclusive scan of the keep counts -> each workgroup's first compacted position; M = kept count;
//             class counts G_c
//   main      per (voxel block, layer): reads each [C] row once in the input's layout, softmax, CE partials per workgroup, and
//             one (key, payload) pair per kept voxel and present class into segment (layer, class) in voxel order:
//             key = ~bits(e) (e = |fg - p_c| >= 0, so an ascending sort of ~bits is a descending sort of e), payload =
//             compacted position | fg << 31
//   sort      4 stable LSD passes of 8 bits over all L x C segments at once: upsweep (tile histograms), scan (per segment and
//             digit, over tiles), downsweep (stable rank by wave match + per-wave digit counts)
//   lovasz    per tile: fg counts; then cumulative fg / bg counts in sorted order -> J_i - J_{i-1} (lovasz_grad, in fp32 as the
//             reference), per-tile partial dot products and the derivative per (layer, compacted voxel, class)
//   finalise  one workgroup sums every partial in a fixed order (no float atomics: the loss is bitwise reproducible)
// Backward: one thread per (voxel, layer) writes its gradient row in the input's layout; every element has one producer.
#include "gf_common.hpp"

namespace gf {
namespace occ {   // a named namespace: every kernel has external linkage and a stable name

constexpr int kVox = 256;                  // voxel kernels: one voxel per thread
constexpr int kTile = 2048;                // sort / scan tiles: 256 threads x 8 keys
constexpr int kItems = kTile / 256;
constexpr int kFin = 1024;                 // finalise: 16 waves

struct OccPreds { const float *p[GF_OCC_MAX_LAYERS]; };
struct OccGrads { float *p[GF_OCC_MAX_LAYERS]; };

struct OccParams {
    int L, N, flags, lovasz_ignore, ignore_index, empty_label;
    long long sc, sn;                      // element (c, n) of a layer is at p[c * sc + n * sn]
    const long long *label;
    const unsigned char *mask;
    const float *cw;
    float ce_weight, lovasz_weight;
};

// two regions, each cut into 256-byte aligned sections: the workspace (what the backward reads; it lives from the forward to
// the backward) and the scratch (the forward's own: keys, histograms, partials; free once the forward has run)
struct OccWs {
    // workspace
    int *hdr;          // [0] M, [1] bad label, [2] non-finite input, [3] present classes; [8 + c] G_c
    int *pos;          // [N] compacted Lovász position; -1 kept but not in the Lovász term; -2 not kept
    float *deriv;      // [L][N][C]      d lovasz_c / d e by compacted position
    double *res;       // [2L] CE numerator / denominator per layer, [L*C] Lovász sums
    // scratch
    int *blk;          // [NB] kept voxels per voxel block -> exclusive offsets
    int *blkg;         // [NB][C] Lovász voxels per voxel block and class
    double *ce_part;   // [L][NB][2] weighted CE numerator, denominator
    uint2 *keys[2];    // [L*C][N]
    int *hist;         // [L*C][256][T]  tile histograms -> exclusive offsets within each digit
    int *tot;          // [L*C][256]     digit totals
    int *fgt;          // [L*C][T]       fg per sorted tile
    double *lov_part;  // [L*C][T]
};

inline int num_blocks(int N) { return (N + kVox - 1) / kVox; }
inline int num_tiles(int N) { return (N + kTile - 1) / kTile; }

// the sections of both regions (null for a null base) and, where asked for, the regions' sizes
inline OccWs carve(void *workspace, void *scratch, int L, int N, size_t *workspace_bytes = nullptr, size_t *scratch_bytes = nullptr)
{
    const size_t S = (size_t)L * kC, NB = num_blocks(N), T = num_tiles(N);
    OccWs ws;
    Carver a(workspace);
    ws.hdr = a.take<int>(64);
    ws.pos = a.take<int>((size_t)N);
    ws.deriv = a.take<float>((size_t)L * N * kC);
    ws.res = a.take<double>(2 * (size_t)L + S);
    Carver b(scratch);
    ws.blk = b.take<int>(NB);
    ws.blkg = b.take<int>(NB * kC);
    ws.ce_part = b.take<double>((size_t)L * NB * 2);
    ws.keys[0] = b.take<uint2>(S * N);
    ws.keys[1] = b.take<uint2>(S * N);
    ws.hist = b.take<int>(S * 256 * T);
    ws.tot = b.take<int>(S * 256);
    ws.fgt = b.take<int>(S * T);
    ws.lov_part = b.take<double>(S * T);
    if (workspace_bytes) *workspace_bytes = a.bytes();
    if (scratch_bytes) *scratch_bytes = b.bytes();
    return ws;
}

struct VoxelState { int y; bool kept, lov, ce; };

__device__ __forceinline__ VoxelState voxel_state(const OccParams &a, int n)
{
    VoxelState v{0, false, false, false};
    if (n >= a.N) return v;
    v.y = (int)a.label[n];
    const long long y = a.label[n];
    v.kept = (!(a.flags & GF_OCC_MASK) || a.mask[n]) && !((a.flags & GF_OCC_IGNORE_EMPTY) && y == a.empty_label);
    v.lov = v.kept && !(a.flags & GF_OCC_NO_LOVASZ) && !((a.flags & GF_OCC_LOVASZ_IGNORE) && y == a.lovasz_ignore);
    v.ce = v.kept && y != a.ignore_index && y >= 0 && y < kC;
    if (y < 0 || y >= kC) v.y = -1;     // fg for no class
    return v;
}

__global__ void __launch_bounds__(64) gf_occ_clear_kernel(OccWs ws)
{
    ws.hdr[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(kVox) gf_occ_prep_kernel(OccParams a, OccWs ws)
{
    __shared__ int g[kC];
    const int n = blockIdx.x * kVox + threadIdx.x;
    if (threadIdx.x < kC) g[threadIdx.x] = 0;
    __syncthreads();
    const VoxelState v = voxel_state(a, n);
    if (v.kept && v.y < 0 && a.label[n] != a.ignore_index) atomicOr(&ws.hdr[1], 1);
    if (v.lov && v.y >= 0) atomicAdd(&g[v.y], 1);
    const unsigned long long m = __ballot(v.lov);
    __shared__ int wc[kVox / 64];
    if (lane_id() == 0) wc[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int i = 0; i < kVox / 64; ++i) s += wc[i];
        ws.blk[blockIdx.x] = s;
    }
    if (threadIdx.x < kC) ws.blkg[(size_t)blockIdx.x * kC + threadIdx.x] = g[threadIdx.x];
}

__global__ void __launch_bounds__(1024) gf_occ_offsets_kernel(int NB, OccWs ws)
{
    __shared__ int lds[16];
    __shared__ int g[kC];
    if (threadIdx.x < kC) g[threadIdx.x] = 0;
    __syncthreads();
    // G_c: integer sums, exact in any order
    int gc[kC];
#pragma unroll
    for (int c = 0; c < kC; ++c) gc[c] = 0;
    for (int b = threadIdx.x; b < NB; b += 1024)
#pragma unroll
        for (int c = 0; c < kC; ++c) gc[c] += ws.blkg[(size_t)b * kC + c];
#pragma unroll
    for (int c = 0; c < kC; ++c) {
        int v = gc[c];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
        if (lane_id() == 0 && v) atomicAdd(&g[c], v);
    }
    __syncthreads();
    if (threadIdx.x < kC) ws.hdr[8 + threadIdx.x] = g[threadIdx.x];
    const int per = (NB + 1023) / 1024, b0 = threadIdx.x * per;
    int s = 0;
    for (int i = 0; i < per; ++i)
        if (b0 + i < NB) s += ws.blk[b0 + i];
    int total;
    int run = block_excl_scan<16>(s, lds, total);
    for (int i = 0; i < per; ++i)
        if (b0 + i < NB) {
            const int c = ws.blk[b0 + i];
            ws.blk[b0 + i] = run;
            run += c;
        }
    if (threadIdx.x == 0) ws.hdr[0] = total;
}

// rows of one voxel block: the head's layout (sc = 1, sn = C) is staged through LDS with coalesced loads; any other layout is read
// in place (a contiguous [C, N] layer is already coalesced across the block)
__device__ __forceinline__ bool rows_staged(const OccParams &a) { return a.sc == 1 && a.sn == kC; }

__device__ __forceinline__ void stage_rows(const OccParams &a, const float *pred, float *tile)
{
    const size_t base = (size_t)blockIdx.x * kVox * kC, end = (size_t)a.N * kC;
#pragma unroll
    for (int k = 0; k < kC; ++k) {
        const int i = k * kVox + threadIdx.x;
        if (base + i < end) tile[i] = pred[base + i];
    }
    __syncthreads();
}

__device__ __forceinline__ void unstage_rows(const OccParams &a, float *out, const float *tile)
{
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * kVox * kC, end = (size_t)a.N * kC;
#pragma unroll
    for (int k = 0; k < kC; ++k) {
        const int i = k * kVox + threadIdx.x;
        if (base + i < end) out[base + i] = tile[i];
    }
}

__device__ __forceinline__ void load_probs(const OccParams &a, const float *pred, const float *tile, int n, float (&x)[kC],
                                           float (&p)[kC], float &lse)
{
    if (tile) {
#pragma unroll
        for (int c = 0; c < kC; ++c) x[c] = tile[threadIdx.x * kC + c];
    } else {
#pragma unroll
        for (int c = 0; c < kC; ++c) x[c] = pred[c * a.sc + (long long)n * a.sn];
    }
    if (a.flags & GF_OCC_PROB) {
#pragma unroll
        for (int c = 0; c < kC; ++c) p[c] = x[c];
        lse = 0.f;
        return;
    }
    float m = x[0];
#pragma unroll
    for (int c = 1; c < kC; ++c) m = fmaxf(m, x[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < kC; ++c) {
        p[c] = expf(x[c] - m);
        s += p[c];
    }
#pragma unroll
    for (int c = 0; c < kC; ++c) p[c] = p[c] / s;
    lse = m + logf(s);
}

// float(1e-6) and float(1 - 1e-6): torch.clamp's bounds on an fp32 tensor
constexpr float kProbLo = (float)1e-6, kProbHi = (float)(1.0 - 1e-6);

__global__ void __launch_bounds__(kVox) gf_occ_main_kernel(OccParams a, OccPreds preds, OccWs ws)
{
    __shared__ double red[kVox];
    __shared__ int lds[kVox / 64];
    __shared__ float tile[kVox * kC];
    const int l = blockIdx.y, n = blockIdx.x * kVox + threadIdx.x;
    const bool staged = rows_staged(a);
    if (staged) stage_rows(a, preds.p[l], tile);
    const VoxelState v = voxel_state(a, n);
    float x[kC], p[kC], lse = 0.f;
    double num = 0.0, den = 0.0;
    if (v.kept) {
        load_probs(a, preds.p[l], staged ? tile : nullptr, n, x, p, lse);
        bool finite = true;
#pragma unroll
        for (int c = 0; c < kC; ++c) finite = finite && isfinite(x[c]);
        if (!finite && (v.ce || v.lov)) atomicOr(&ws.hdr[2], 1);
        if (v.ce) {
            float xy = 0.f;
#pragma unroll
            for (int c = 0; c < kC; ++c) xy = c == v.y ? x[c] : xy;
            const float term = (a.flags & GF_OCC_PROB) ? -logf(fminf(fmaxf(xy, kProbLo), kProbHi)) : lse - xy;
            const float w = a.cw[v.y];
            num = (double)w * (double)term;
            den = (double)w;
        }
    }
    int total;
    const int rank = block_excl_scan<kVox / 64>(v.lov ? 1 : 0, lds, total);
    const int gpos = ws.blk[blockIdx.x] + rank;
    if (l == 0 && n < a.N) ws.pos[n] = v.lov ? gpos : (v.kept ? -1 : -2);
    if (v.lov) {
        const size_t N = (size_t)a.N;
#pragma unroll
        for (int c = 0; c < kC; ++c) {
            if (ws.hdr[8 + c] == 0) continue;          // absent class: no segment
            const bool fg = v.y == c;
            const float e = fabsf((fg ? 1.f : 0.f) - p[c]);
            ws.keys[0][((size_t)l * kC + c) * N + gpos] = make_uint2(~__float_as_uint(e), (unsigned)gpos | (fg ? 0x80000000u : 0u));
        }
    }
    const double sn = block_sum256(num, red);
    __syncthreads();
    const double sd = block_sum256(den, red);
    if (threadIdx.x == 0) {
        double *o = ws.ce_part + ((size_t)l * gridDim.x + blockIdx.x) * 2;
        o[0] = sn;
        o[1] = sd;
    }
}

// ---- segmented LSD radix sort: segment s = layer * C + class, length M (the same for every segment), capacity N

__global__ void __launch_bounds__(256) gf_occ_upsweep_kernel(int N, int T, int shift, const uint2 *in, OccWs ws)
{
    __shared__ int h[256];
    const int t = blockIdx.x, s = blockIdx.y, c = s % kC, M = ws.hdr[0], base = t * kTile;
    if (ws.hdr[8 + c] == 0 || base >= M) return;
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint2 *seg = in + (size_t)s * N;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < M) atomicAdd(&h[(seg[i].x >> shift) & 255u], 1);
    }
    __syncthreads();
    ws.hist[((size_t)s * 256 + threadIdx.x) * T + t] = h[threadIdx.x];
}

// one wave per (digit, segment): exclusive scan of the digit's tile counts in tile order, and the digit total
__global__ void __launch_bounds__(64) gf_occ_digit_scan_kernel(int T, OccWs ws)
{
    const int d = blockIdx.x, s = blockIdx.y, c = s % kC, M = ws.hdr[0];
    if (ws.hdr[8 + c] == 0) return;
    const int nt = (M + kTile - 1) / kTile;
    int *h = ws.hist + ((size_t)s * 256 + d) * T;
    int run = 0;
    for (int t0 = 0; t0 < nt; t0 += 64) {
        const int t = t0 + lane_id();
        const int v = t < nt ? h[t] : 0;
        const int incl = wave_incl_scan_shfl(v);
        if (t < nt) h[t] = run + incl - v;
        run += __shfl(incl, 63, 64);
    }
    if (lane_id() == 0) ws.tot[s * 256 + d] = run;
}

__global__ void __launch_bounds__(256) gf_occ_downsweep_kernel(int N, int T, int shift, const uint2 *in, uint2 *out, OccWs ws)
{
    __shared__ int gbase[256];
    __shared__ int cnt[4][256];
    __shared__ int lds[4];
    const int t = blockIdx.x, s = blockIdx.y, c = s % kC, M = ws.hdr[0], base = t * kTile;
    if (ws.hdr[8 + c] == 0 || base >= M) return;
    const int tid = threadIdx.x, w = tid >> 6;
    int total;
    const int dbase = block_excl_scan<4>(ws.tot[s * 256 + tid], lds, total);
    gbase[tid] = dbase + ws.hist[((size_t)s * 256 + tid) * T + t];
    const uint2 *src = in + (size_t)s * N;
    uint2 *dst = out + (size_t)s * N;
    // all of the tile's keys in flight at once, before the serial rank steps
    uint2 kvs[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int i = base + k * 256 + tid;
        kvs[k] = i < M ? src[i] : make_uint2(0u, 0u);
    }
    int run = 0;    // thread tid: elements of digit tid already placed by this tile
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const bool valid = base + k * 256 + tid < M;
        const uint2 kv = kvs[k];
        const unsigned d = (kv.x >> shift) & 255u;
#pragma unroll
        for (int r = 0; r < 4; ++r) cnt[r][tid] = 0;
        __syncthreads();
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bb = __ballot(bit);
            m &= bit ? bb : ~bb;
        }
        const int rank = mbcnt(m);
        if (valid && rank == 0) cnt[w][d] = __popcll(m);
        __syncthreads();
        const int c0 = cnt[0][tid], c1 = cnt[1][tid], c2 = cnt[2][tid], c3 = cnt[3][tid];
        cnt[0][tid] = run;
        cnt[1][tid] = run + c0;
        cnt[2][tid] = run + c0 + c1;
        cnt[3][tid] = run + c0 + c1 + c2;
        run += c0 + c1 + c2 + c3;
        __syncthreads();
        if (valid) dst[gbase[d] + cnt[w][d] + rank] = kv;
        __syncthreads();
    }
}

// ---- Lovász gradient in sorted order

__global__ void __launch_bounds__(256) gf_occ_fg_count_kernel(int N, int T, const uint2 *sorted, OccWs ws)
{
    __shared__ int lds[4];
    const int t = blockIdx.x, s = blockIdx.y, c = s % kC, M = ws.hdr[0], base = t * kTile;
    if (ws.hdr[8 + c] == 0 || base >= M) return;
    const uint2 *seg = sorted + (size_t)s * N;
    int f = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < M) f += seg[i].y >> 31;
    }
    int total;
    block_excl_scan<4>(f, lds, total);
    if (threadIdx.x == 0) ws.fgt[(size_t)s * T + t] = total;
}

__global__ void __launch_bounds__(256) gf_occ_lovasz_kernel(int N, int T, const uint2 *sorted, OccWs ws)
{
    __shared__ int lds[4];
    __shared__ double red[256];
    const int t = blockIdx.x, s = blockIdx.y, l = s / kC, c = s % kC, M = ws.hdr[0], base = t * kTile;
    const int G = ws.hdr[8 + c];
    if (G == 0 || base >= M) return;
    const int tid = threadIdx.x;
    // fg count of the tiles before this one
    int before = 0;
    for (int u = tid; u < t; u += 256) before += ws.fgt[(size_t)s * T + u];
    int total;
    block_excl_scan<4>(before, lds, total);
    before = total;
    // the tile's keys: coalesced loads into LDS, then eight consecutive keys per thread for the scan
    __shared__ uint2 keys[kTile];
    const uint2 *seg = sorted + (size_t)s * N;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int j = k * 256 + tid;
        keys[j] = base + j < M ? seg[base + j] : make_uint2(0xffffffffu, 0u);
    }
    __syncthreads();
    uint2 kv[kItems];
    int f = 0;
    const int i0 = base + tid * kItems;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        kv[k] = keys[tid * kItems + k];
        f += kv[k].y >> 31;
    }
    int F = before + block_excl_scan<4>(f, lds, total);   // fg among sorted elements [0, i0)
    const float Gf = (float)G;
    float *deriv = ws.deriv + (size_t)l * N * kC + c;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int i = i0 + k;
        if (i >= M) break;
        const int fg = (int)(kv[k].y >> 31);
        const int Fp = F, Bp = i - Fp;          // counts among the first i elements
        F += fg;
        const int B = i + 1 - F;
        // lovasz_grad: jaccard_i = 1 - (G - F_i) / (G + B_i), then jaccard[1:] -= jaccard[:-1], in fp32
        const float J = 1.f - (Gf - (float)F) / (Gf + (float)B);
        const float Jp = i == 0 ? 0.f : 1.f - (Gf - (float)Fp) / (Gf + (float)Bp);
        const float dj = J - Jp;
        const float e = __uint_as_float(~kv[k].x);
        acc += (double)e * (double)dj;
        deriv[(size_t)(kv[k].y & 0x7fffffffu) * kC] = dj;
    }
    const double sum = block_sum256(acc, red);
    if (tid == 0) ws.lov_part[(size_t)s * T + t] = sum;
}

__global__ void __launch_bounds__(kFin) gf_occ_finalise_kernel(OccParams a, int NB, int T, OccWs ws, float *loss)
{
    __shared__ double res[2 * GF_OCC_MAX_LAYERS + GF_OCC_MAX_LAYERS * kC];
    const int L = a.L, S = L * kC, M = ws.hdr[0], nt = (M + kTile - 1) / kTile;
    const int w = threadIdx.x >> 6, lane = lane_id();
    for (int j = w; j < 2 * L + S; j += kFin / 64) {
        double v = 0.0;
        const double *src = nullptr;
        size_t stride = 1;
        int count = 0;
        if (j < 2 * L) {
            src = ws.ce_part + (size_t)(j >> 1) * NB * 2 + (j & 1);
            stride = 2;
            count = NB;
        } else if (ws.hdr[8 + (j - 2 * L) % kC] != 0) {
            src = ws.lov_part + (size_t)(j - 2 * L) * T;
            count = nt;
        }
        // eight independent loads in flight per lane, summed in a fixed order
        for (int b0 = 0; b0 < count; b0 += 8 * 64) {
            double t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int b = b0 + k * 64 + lane;
                t[k] = b < count ? src[stride * b] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) v += t[k];
        }
        v = wave_sum_f64(v);
        if (lane == 0) res[j] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int present = 0;
    for (int c = 0; c < kC; ++c) present += ws.hdr[8 + c] != 0;
    double total = 0.0;
    for (int l = 0; l < L; ++l) {
        const double ce = res[2 * l] / res[2 * l + 1];
        double lov = 0.0;
        for (int c = 0; c < kC; ++c) lov += res[2 * L + l * kC + c];
        lov = present ? lov / present : 0.0;
        total += (double)a.ce_weight * ce + (double)a.lovasz_weight * lov;
    }
    total /= L;
    if (ws.hdr[1] || ws.hdr[2]) total = __builtin_nan("");
    for (int j = 0; j < 2 * L + S; ++j) ws.res[j] = res[j];
    ws.hdr[3] = present;
    *loss = (float)total;
}

__global__ void __launch_bounds__(kVox) gf_occ_backward_kernel(OccParams a, OccPreds preds, OccGrads grads,
                                                               const float *grad_loss, OccWs ws)
{
    __shared__ float tile[kVox * kC];
    const int l = blockIdx.y, n = blockIdx.x * kVox + threadIdx.x;
    const bool staged = rows_staged(a);
    if (staged) stage_rows(a, preds.p[l], tile);
    float *gout = grads.p[l];
    const int pos = n < a.N ? ws.pos[n] : -2;
    float g[kC];
#pragma unroll
    for (int c = 0; c < kC; ++c) g[c] = 0.f;
    if (pos != -2) {
        const VoxelState v = voxel_state(a, n);
        const bool prob = a.flags & GF_OCC_PROB;
        const float go = *grad_loss / (float)a.L;
        float x[kC], p[kC], lse;
        load_probs(a, preds.p[l], staged ? tile : nullptr, n, x, p, lse);
        if (v.ce) {
            const float sc = (float)((double)(go * a.ce_weight) * (double)a.cw[v.y] / ws.res[2 * l + 1]);
            if (prob) {
                float xy = 0.f;
#pragma unroll
                for (int c = 0; c < kC; ++c) xy = c == v.y ? x[c] : xy;
                const float gy = (xy >= kProbLo && xy <= kProbHi) ? -sc / xy : 0.f;
#pragma unroll
                for (int c = 0; c < kC; ++c) g[c] = c == v.y ? gy : 0.f;
            } else {
#pragma unroll
                for (int c = 0; c < kC; ++c) g[c] = sc * (p[c] - (c == v.y ? 1.f : 0.f));
            }
        }
        const int present = ws.hdr[3];
        if (pos >= 0 && present > 0) {
            const float lw = go * a.lovasz_weight / (float)present;
            const float *d = ws.deriv + ((size_t)l * a.N + pos) * kC;
            float gl[kC], dot = 0.f;
#pragma unroll
            for (int c = 0; c < kC; ++c) {
                const float diff = (v.y == c ? 1.f : 0.f) - p[c];
                const float sgn = diff > 0.f ? -1.f : (diff < 0.f ? 1.f : 0.f);   // d|fg - p| / dp, 0 at 0 as torch
                gl[c] = ws.hdr[8 + c] != 0 ? lw * d[c] * sgn : 0.f;
                dot += gl[c] * p[c];
            }
#pragma unroll
            for (int c = 0; c < kC; ++c) g[c] += prob ? gl[c] : p[c] * (gl[c] - dot);
        }
    }
    if (staged) {
        __syncthreads();     // every thread has read its row of the input tile
#pragma unroll
        for (int c = 0; c < kC; ++c) tile[threadIdx.x * kC + c] = g[c];
        unstage_rows(a, gout, tile);
    } else if (n < a.N) {
#pragma unroll
        for (int c = 0; c < kC; ++c) gout[c * a.sc + (long long)n * a.sn] = g[c];
    }
}

int check_common(const char *fn, int L, int N, int C, int flags, const float *const *pred, long long sc, long long sn,
                 const long long *label, const unsigned char *mask, const float *cw, void *workspace, size_t workspace_bytes)
{
    if (C != kC) { set_error("%s: C = %d; only %d channels are supported", fn, C, kC); return GF_EINVAL; }
    if (L < 1 || L > GF_OCC_MAX_LAYERS) { set_error("%s: L = %d; 1 <= L <= %d", fn, L, GF_OCC_MAX_LAYERS); return GF_EINVAL; }
    if (N < 1 || N > (1 << 28)) { set_error("%s: N = %d; 1 <= N <= 2^28", fn, N); return GF_EINVAL; }
    if (flags & ~(GF_OCC_PROB | GF_OCC_MASK | GF_OCC_LOVASZ_IGNORE | GF_OCC_IGNORE_EMPTY | GF_OCC_NO_LOVASZ)) {
        set_error("%s: unknown flags 0x%x", fn, flags);
        return GF_EINVAL;
    }
    if (sc < 1 || sn < 1) { set_error("%s: strides must be positive (got %lld, %lld)", fn, sc, sn); return GF_EINVAL; }
    if (!pred || !label || !cw || !workspace) { set_error("%s: null pointer", fn); return GF_EINVAL; }
    for (int l = 0; l < L; ++l)
        if (!pred[l]) { set_error("%s: null prediction pointer of layer %d", fn, l); return GF_EINVAL; }
    if ((flags & GF_OCC_MASK) && !mask) { set_error("%s: GF_OCC_MASK without a mask", fn); return GF_EINVAL; }
    size_t need = 0;
    carve(nullptr, nullptr, L, N, &need);
    GF_CHECK_WORKSPACE_AS(fn, "workspace", workspace_bytes, need);
    return GF_OK;
}

OccParams make_params(int L, int N, int flags, long long sc, long long sn, const long long *label, const unsigned char *mask,
                      const float *cw, float ce_weight, float lovasz_weight, int lovasz_ignore, int ignore_index, int empty_label)
{
    OccParams a{};
    a.L = L; a.N = N; a.flags = flags; a.lovasz_ignore = lovasz_ignore; a.ignore_index = ignore_index;
    a.empty_label = empty_label; a.sc = sc; a.sn = sn; a.label = label; a.mask = mask; a.cw = cw;
    a.ce_weight = ce_weight; a.lovasz_weight = lovasz_weight;
    return a;
}

}  // namespace occ
}  // namespace gf

extern "C" size_t gf_occ_loss_workspace_bytes(int L, int N, int C, int flags)
{
    (void)flags;
    if (C != GF_NUM_CHANNELS || L < 1 || L > GF_OCC_MAX_LAYERS || N < 1 || N > (1 << 28)) return 0;
    size_t w = 0;
    gf::occ::carve(nullptr, nullptr, L, N, &w);
    return w;
}

extern "C" size_t gf_occ_loss_scratch_bytes(int L, int N, int C, int flags)
{
    (void)flags;
    if (C != GF_NUM_CHANNELS || L < 1 || L > GF_OCC_MAX_LAYERS || N < 1 || N > (1 << 28)) return 0;
    size_t b = 0;
    gf::occ::carve(nullptr, nullptr, L, N, nullptr, &b);
    return b;
}

extern "C" int gf_occ_loss_forward(int L, int N, int C, int flags, const float *const *pred, long long stride_c,
                                   long long stride_n, const long long *label, const unsigned char *mask,
                                   const float *class_weights, float ce_weight, float lovasz_weight, int lovasz_ignore,
                                   int ignore_index, int empty_label, float *loss, void *workspace, size_t workspace_bytes,
                                   void *scratch, size_t scratch_bytes, void *stream_)
{
    using namespace gf;
    using namespace gf::occ;
    int rc = check_common(__func__, L, N, C, flags, pred, stride_c, stride_n, label, mask, class_weights, workspace,
                          workspace_bytes);
    if (rc != GF_OK) return rc;
    GF_CHECK_ARG(loss, "null loss pointer");
    GF_CHECK_ARG(scratch, "null scratch pointer");
    size_t need = 0;
    const OccWs ws = carve(workspace, scratch, L, N, nullptr, &need);
    GF_CHECK_WORKSPACE_AS(__func__, "scratch", scratch_bytes, need);
    const hipStream_t stream = (hipStream_t)stream_;
    const OccParams a = make_params(L, N, flags, stride_c, stride_n, label, mask, class_weights, ce_weight, lovasz_weight,
                                    lovasz_ignore, ignore_index, empty_label);
    OccPreds preds{};
    for (int l = 0; l < L; ++l) preds.p[l] = pred[l];
    const int NB = num_blocks(N), T = num_tiles(N), S = L * kC;
    hipLaunchKernelGGL(gf_occ_clear_kernel, dim3(1), dim3(64), 0, stream, ws);
    hipLaunchKernelGGL(gf_occ_prep_kernel, dim3(NB), dim3(kVox), 0, stream, a, ws);
    hipLaunchKernelGGL(gf_occ_offsets_kernel, dim3(1), dim3(1024), 0, stream, NB, ws);
    hipLaunchKernelGGL(gf_occ_main_kernel, dim3(NB, L), dim3(kVox), 0, stream, a, preds, ws);
    // without the Lovász term no voxel has a key (M = 0, no present class): the sort and the Lovász pass are not launched
    for (int pass = 0; pass < 4 && !(flags & GF_OCC_NO_LOVASZ); ++pass) {
        const uint2 *in = ws.keys[pass & 1];
        uint2 *out = ws.keys[(pass & 1) ^ 1];
        hipLaunchKernelGGL(gf_occ_upsweep_kernel, dim3(T, S), dim3(256), 0, stream, N, T, 8 * pass, in, ws);
        hipLaunchKernelGGL(gf_occ_digit_scan_kernel, dim3(256, S), dim3(64), 0, stream, T, ws);
        hipLaunchKernelGGL(gf_occ_downsweep_kernel, dim3(T, S), dim3(256), 0, stream, N, T, 8 * pass, in, out, ws);
    }
    // four passes: the sorted keys are back in keys[0]
    if (!(flags & GF_OCC_NO_LOVASZ)) {
        hipLaunchKernelGGL(gf_occ_fg_count_kernel, dim3(T, S), dim3(256), 0, stream, N, T, ws.keys[0], ws);
        hipLaunchKernelGGL(gf_occ_lovasz_kernel, dim3(T, S), dim3(256), 0, stream, N, T, ws.keys[0], ws);
    }
    hipLaunchKernelGGL(gf_occ_finalise_kernel, dim3(1), dim3(kFin), 0, stream, a, NB, T, ws, loss);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_occ_loss_backward(int L, int N, int C, int flags, const float *const *pred, long long stride_c,
                                    long long stride_n, const long long *label, const unsigned char *mask,
                                    const float *class_weights, float ce_weight, float lovasz_weight, int lovasz_ignore,
                                    int ignore_index, int empty_label, const float *grad_loss, float *const *grad_pred,
                                    void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace gf;
    using namespace gf::occ;
    int rc = check_common(__func__, L, N, C, flags, pred, stride_c, stride_n, label, mask, class_weights, workspace,
                          workspace_bytes);
    if (rc != GF_OK) return rc;
    GF_CHECK_ARG(grad_loss && grad_pred, "null gradient pointer");
    for (int l = 0; l < L; ++l) GF_CHECK_ARG(grad_pred[l], "null gradient pointer of a layer");
    const OccWs ws = carve(workspace, nullptr, L, N);
    const OccParams a = make_params(L, N, flags, stride_c, stride_n, label, mask, class_weights, ce_weight, lovasz_weight,
                                    lovasz_ignore, ignore_index, empty_label);
    OccPreds preds{};
    OccGrads grads{};
    for (int l = 0; l < L; ++l) {
        preds.p[l] = pred[l];
        grads.p[l] = grad_pred[l];
    }
    hipLaunchKernelGGL(gf_occ_backward_kernel, dim3(num_blocks(N), L), dim3(kVox), 0, (hipStream_t)stream_, a, preds, grads,
                       grad_loss, ws);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
