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
// With GF_OCC_SCAL (gf_occ_loss_scal_*) the scene-class affinity terms sem_scal / geo_scal (loss/occupancy_loss.py:185-268) ride
// along in instantiations of main, finalise and backward of their own: main adds per-workgroup column sums S_c, N_c, T_c of
// the rows it holds; scal_sums adds them over the workgroups; finalise evaluates the terms and leaves a_c, b_c; the backward
// adds a_c + b_c [y = c] before its softmax Jacobian.  The instantiations without the terms are the kernels as they were.
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

// the sections of the scene-class affinity terms (GF_OCC_SCAL), carved behind the others: one of the workspace, two of the scratch
struct OccScalWs {
    float *ab;         // [L][2][C]   d loss_l / d S_c and d loss_l / d N_c, weights and 1/count folded in
    double *sn_part;   // [L][2C][NB] per voxel block: S_c = sum of p_c over V, then N_c = the same over the voxels labelled c
    int *t_part;       // [C][NB]     voxels of V labelled c per voxel block
    double *sums;      // [L*2C + C]  the partials summed over the voxel blocks: S_c, N_c per layer, then T_c (exact in a double)
    float sem_w, geo_w;
};
// the kernels that have an instantiation with these terms take the sections as a parameter pack: empty without them, so that
// instantiation's arguments and code are those of the kernel without the terms
__device__ __forceinline__ const OccScalWs &scal_ws(const OccScalWs &sw) { return sw; }

inline int num_blocks(int N) { return (N + kVox - 1) / kVox; }
inline int num_tiles(int N) { return (N + kTile - 1) / kTile; }

// the sections of both regions (null for a null base) and, where asked for, the regions' sizes
inline OccWs carve(void *workspace, void *scratch, int L, int N, size_t *workspace_bytes = nullptr, size_t *scratch_bytes = nullptr,
                   OccScalWs *scal = nullptr)
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
    if (scal) {
        scal->ab = a.take<float>(2 * S);
        scal->sn_part = b.take<double>(2 * S * NB);
        scal->t_part = b.take<int>(kC * NB);
        scal->sums = b.take<double>(2 * S + kC);
    }
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

// Column sums of the block's rows of p in the tile (zero outside V; ylds = the label, -1 outside V), in a fixed order: lanes
// 8c .. 8c + 7 take class c, lane j of them the rows j, j + 8, ..., summed in row order in double; the eight are then added by a
// butterfly, which gives every lane the same bits.
__device__ __forceinline__ void scal_block_sums(const float *tile, const int *ylds, int l, const OccScalWs &sw)
{
    const int c = threadIdx.x >> 3, seg = threadIdx.x & 7, NB = gridDim.x;
    double s = 0.0, sy = 0.0;
    int t = 0;
    if (c < kC)
#pragma unroll
        for (int k = 0; k < kVox / 8; ++k) {
            const int r = k * 8 + seg;
            const float pv = tile[r * kC + c];
            const bool fg = ylds[r] == c;
            s += (double)pv;
            sy += fg ? (double)pv : 0.0;
            t += fg ? 1 : 0;
        }
#pragma unroll
    for (int d = 4; d > 0; d >>= 1) {
        s += __shfl_xor(s, d, 64);
        sy += __shfl_xor(sy, d, 64);
        t += __shfl_xor(t, d, 64);
    }
    if (c < kC && seg == 0) {
        sw.sn_part[((size_t)l * 2 * kC + c) * NB + blockIdx.x] = s;
        sw.sn_part[((size_t)l * 2 * kC + kC + c) * NB + blockIdx.x] = sy;
        if (l == 0) sw.t_part[(size_t)c * NB + blockIdx.x] = t;
    }
}

// Scal = OccScalWs: with the affinity terms' block sums; empty: without (the instantiation of gf_occ_loss_forward)
template <class... Scal>
__global__ void __launch_bounds__(kVox) gf_occ_main_kernel(OccParams a, OccPreds preds, OccWs ws, Scal... sw_)
{
    constexpr bool kScal = sizeof...(Scal) != 0;
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
    if constexpr (kScal) {
        // every thread puts its row of p back into its own row of the tile (it alone has read that row)
        __shared__ int ylds[kVox];
#pragma unroll
        for (int c = 0; c < kC; ++c) tile[threadIdx.x * kC + c] = 0.f;
        if (v.ce) {
#pragma unroll
            for (int c = 0; c < kC; ++c) tile[threadIdx.x * kC + c] = p[c];
        }
        ylds[threadIdx.x] = v.ce ? v.y : -1;
        __syncthreads();
        scal_block_sums(tile, ylds, l, scal_ws(sw_...));
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

// ---- scene-class affinity terms (sem_scal_loss, geo_scal_loss of loss/occupancy_loss.py:185-268) from the sums of one layer

// binary_cross_entropy_with_logits(inverse_sigmoid(x), 1) on an fp32 scalar and its derivative -1 / x' at the shifted x'.  The
// reference's two while loops, each cut off after kScalSteps steps: a ratio of probabilities needs three at the most, and one
// that is still out of range then (inputs that are no probabilities) is reported as bad instead of looping on.
constexpr int kScalSteps = 8;

__device__ __forceinline__ float scal_f(float x, float &dfdx, bool &bad)
{
    const float hi = (float)(1.0 - 1e-5), eps = 1e-5f;
    for (int i = 0; i < kScalSteps && x >= hi; ++i) x -= eps;
    for (int i = 0; i < kScalSteps && x < eps; ++i) x += eps;
    if (!(x >= eps && x < hi)) bad = true;        // NaN included
    dfdx = -1.f / x;
    const float u = logf(1.f / x - 1.f);          // -inverse_sigmoid(x); the loss is softplus(u)
    return fmaxf(u, 0.f) + log1pf(expf(-fabsf(u)));
}

// Thread i of a layer's C: i < C - 1 evaluates class i's precision, recall and specificity (0 for a class absent from V), i = C - 1
// the geo term of class `empty`.  From S_c, N_c (sums: [2C] doubles, each rounded to fp32 once), T_c and |V|.  Returns the
// term and, unweighted, its derivatives by S and N of its class.
__device__ __forceinline__ float scal_class_term(int i, const double *sums, const int *tc, int V, int empty, float &da, float &db,
                                                 bool &bad)
{
    const float eps = 1e-5f;
    float d;
    da = db = 0.f;
    if (i < kC - 1) {
        if (tc[i] == 0) return 0.f;
        const float S = (float)sums[i], Ny = (float)sums[kC + i], Tf = (float)tc[i];
        float cls = 0.f;
        if (S > 0.f) {
            const float den = S + eps, x = Ny / den;
            cls += scal_f(x, d, bad);
            da -= d * x / den;
            db += d / den;
        }
        {
            const float den = Tf + eps, x = Ny / den;
            cls += scal_f(x, d, bad);
            db += d / den;
        }
        if (V - tc[i] > 0) {
            const float R = (float)(V - tc[i]), den = R + eps, x = (R - (S - Ny)) / den;
            cls += scal_f(x, d, bad);
            da -= d / den;
            db += d / den;
        }
        return cls;
    }
    const float S = (float)sums[empty], Ny = (float)sums[kC + empty], Tf = (float)tc[empty], R = (float)(V - tc[empty]);
    const float I = R - (S - Ny), d1 = ((float)V - S) + eps, d2 = R + eps, d3 = Tf + eps;
    const float x1 = I / d1, x2 = I / d2, x3 = Ny / d3;
    float f1, f2, f3;
    float geo = scal_f(x1, f1, bad);
    geo += scal_f(x2, f2, bad);
    geo += scal_f(x3, f3, bad);
    da = f1 * (x1 - 1.f) / d1 - f2 / d2;
    db = f1 / d1 + f2 / d2 + f3 / d3;
    return geo;
}

// finalise's LDS for the terms: only the instantiation with them refers to it
struct ScalLds {
    double sums[GF_OCC_MAX_LAYERS * 2 * kC];   // S_c, N_c per layer
    int tc[kC];                                // T_c
    float term[GF_OCC_MAX_LAYERS][kC];         // per layer: the sem term of the classes 0 .. C-2, then geo
    float geo_d[GF_OCC_MAX_LAYERS][2];         // d geo / d S_e, d geo / d N_e
    double scal[GF_OCC_MAX_LAYERS];            // sem_w sem + geo_w geo
    int bad;
};
__device__ __forceinline__ ScalLds &scal_lds()
{
    __shared__ ScalLds lds;
    return lds;
}

// One workgroup per sum: thread t adds the voxel blocks t, t + 256, ... in that order, then the workgroup's fixed tree.
__global__ void __launch_bounds__(256) gf_occ_scal_sums_kernel(int NB, int nsn, OccScalWs sw)
{
    __shared__ double red[256];
    const int j = blockIdx.x;
    double v = 0.0;
    if (j < nsn) {
        const double *src = sw.sn_part + (size_t)j * NB;
        for (int b = threadIdx.x; b < NB; b += 256) v += src[b];
    } else {
        const int *src = sw.t_part + (size_t)(j - nsn) * NB;
        for (int b = threadIdx.x; b < NB; b += 256) v += (double)src[b];
    }
    v = block_sum256(v, red);
    if (threadIdx.x == 0) sw.sums[j] = v;
}

template <class... Scal>
__global__ void __launch_bounds__(kFin) gf_occ_finalise_kernel(OccParams a, int NB, int T, OccWs ws, float *loss, Scal... sw_)
{
    constexpr bool kScal = sizeof...(Scal) != 0;
    __shared__ double res[2 * GF_OCC_MAX_LAYERS + GF_OCC_MAX_LAYERS * kC];
    if constexpr (kScal) {
        const OccScalWs &sw = scal_ws(sw_...);
        ScalLds &sl = scal_lds();
        if (threadIdx.x == 0) sl.bad = 0;
        const int nsn = a.L * 2 * kC;
        if ((int)threadIdx.x < nsn) sl.sums[threadIdx.x] = sw.sums[threadIdx.x];
        if ((int)threadIdx.x < kC) sl.tc[threadIdx.x] = (int)sw.sums[nsn + threadIdx.x];
    }
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
    if constexpr (kScal) {
        // C threads per layer: one per class of the sem term, the last one the geo term; then one store of a and b per class
        const OccScalWs &sw = scal_ws(sw_...);
        ScalLds &sl = scal_lds();
        const bool active = (int)threadIdx.x < L * kC;
        const int l = threadIdx.x / kC, i = threadIdx.x % kC;
        int V = 0, count = 0;
        float da = 0.f, db = 0.f;
        if (active) {
            for (int c = 0; c < kC; ++c) V += sl.tc[c];
            for (int c = 0; c < kC - 1; ++c) count += sl.tc[c] > 0;
            bool bad = count == 0;                    // the reference divides by zero in Python here
            sl.term[l][i] = scal_class_term(i, sl.sums + l * 2 * kC, sl.tc, V, a.empty_label, da, db, bad);
            if (i == kC - 1) {
                sl.geo_d[l][0] = da;
                sl.geo_d[l][1] = db;
            }
            if (bad) atomicOr(&sl.bad, 1);
        }
        __syncthreads();
        if (active) {
            const float inv = sw.sem_w / (float)count;
            float ga = i < kC - 1 ? inv * da : 0.f, gb = i < kC - 1 ? inv * db : 0.f;
            if (i == a.empty_label) {
                ga += sw.geo_w * sl.geo_d[l][0];
                gb += sw.geo_w * sl.geo_d[l][1];
            }
            sw.ab[l * 2 * kC + i] = ga;
            sw.ab[l * 2 * kC + kC + i] = gb;
            if (i == 0) {
                float total = 0.f;                    // in class order, as the reference's loop (an absent class adds 0)
                for (int c = 0; c < kC - 1; ++c) total += sl.term[l][c];
                const float sem = total / (float)count;
                sl.scal[l] = (double)sw.sem_w * (double)sem + (double)sw.geo_w * (double)sl.term[l][kC - 1];
            }
        }
        __syncthreads();
    }
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
        if constexpr (kScal) total += scal_lds().scal[l];
    }
    total /= L;
    if (ws.hdr[1] || ws.hdr[2]) total = __builtin_nan("");
    if constexpr (kScal)
        if (scal_lds().bad) total = __builtin_nan("");
    for (int j = 0; j < 2 * L + S; ++j) ws.res[j] = res[j];
    ws.hdr[3] = present;
    *loss = (float)total;
}

template <class... Scal>
__global__ void __launch_bounds__(kVox) gf_occ_backward_kernel(OccParams a, OccPreds preds, OccGrads grads, const float *grad_loss,
                                                               OccWs ws, Scal... sw_)
{
    constexpr bool kScal = sizeof...(Scal) != 0;
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
        if constexpr (kScal) {
            // the affinity terms' gradient in p-space, a_c + b_c [y = c], on every voxel of V (Lovász voxel or not)
            if (v.ce) {
                const float *ab = scal_ws(sw_...).ab + l * 2 * kC;
                float gs[kC], dot = 0.f;
#pragma unroll
                for (int c = 0; c < kC; ++c) {
                    gs[c] = go * (ab[c] + (c == v.y ? ab[kC + c] : 0.f));
                    dot += gs[c] * p[c];
                }
#pragma unroll
                for (int c = 0; c < kC; ++c) g[c] += prob ? gs[c] : p[c] * (gs[c] - dot);
            }
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

// `scal`: the caller is one of the gf_occ_loss_scal_* entry points, which take (and require) GF_OCC_SCAL
int check_common(const char *fn, bool scal, int L, int N, int C, int flags, const float *const *pred, long long sc, long long sn,
                 const long long *label, const unsigned char *mask, const float *cw, int empty_label, void *workspace,
                 size_t workspace_bytes)
{
    if (C != kC) { set_error("%s: C = %d; only %d channels are supported", fn, C, kC); return GF_EINVAL; }
    if (L < 1 || L > GF_OCC_MAX_LAYERS) { set_error("%s: L = %d; 1 <= L <= %d", fn, L, GF_OCC_MAX_LAYERS); return GF_EINVAL; }
    if (N < 1 || N > (1 << 28)) { set_error("%s: N = %d; 1 <= N <= 2^28", fn, N); return GF_EINVAL; }
    if (flags & ~(GF_OCC_PROB | GF_OCC_MASK | GF_OCC_LOVASZ_IGNORE | GF_OCC_IGNORE_EMPTY | GF_OCC_NO_LOVASZ | (scal ? GF_OCC_SCAL : 0))) {
        set_error("%s: unknown flags 0x%x", fn, flags);
        return GF_EINVAL;
    }
    if (scal && !(flags & GF_OCC_SCAL)) { set_error("%s: flags 0x%x lack GF_OCC_SCAL", fn, flags); return GF_EINVAL; }
    if (scal && (empty_label < 0 || empty_label >= kC)) {
        set_error("%s: empty_label = %d; the geo term needs a class in [0, %d)", fn, empty_label, kC);
        return GF_EINVAL;
    }
    if (sc < 1 || sn < 1) { set_error("%s: strides must be positive (got %lld, %lld)", fn, sc, sn); return GF_EINVAL; }
    if (!pred || !label || !cw || !workspace) { set_error("%s: null pointer", fn); return GF_EINVAL; }
    for (int l = 0; l < L; ++l)
        if (!pred[l]) { set_error("%s: null prediction pointer of layer %d", fn, l); return GF_EINVAL; }
    if ((flags & GF_OCC_MASK) && !mask) { set_error("%s: GF_OCC_MASK without a mask", fn); return GF_EINVAL; }
    size_t need = 0;
    OccScalWs sw{};
    carve(nullptr, nullptr, L, N, &need, nullptr, scal ? &sw : nullptr);
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

size_t region_bytes(int L, int N, int C, int flags, bool scratch)
{
    if (C != GF_NUM_CHANNELS || L < 1 || L > GF_OCC_MAX_LAYERS || N < 1 || N > (1 << 28)) return 0;
    size_t w = 0, b = 0;
    OccScalWs sw{};
    carve(nullptr, nullptr, L, N, &w, &b, (flags & GF_OCC_SCAL) ? &sw : nullptr);
    return scratch ? b : w;
}

// both forwards: the kernels of the affinity terms (`scal`) are instantiations of their own, chosen here on the host
int forward(const char *fn, bool scal, int L, int N, int C, int flags, const float *const *pred, long long stride_c,
            long long stride_n, const long long *label, const unsigned char *mask, const float *class_weights, float ce_weight,
            float lovasz_weight, float sem_scal_weight, float geo_scal_weight, int lovasz_ignore, int ignore_index, int empty_label,
            float *loss, void *workspace, size_t workspace_bytes, void *scratch, size_t scratch_bytes, void *stream_)
{
    int rc = check_common(fn, scal, L, N, C, flags, pred, stride_c, stride_n, label, mask, class_weights, empty_label, workspace,
                          workspace_bytes);
    if (rc != GF_OK) return rc;
    GF_CHECK_ARG_AS(fn, loss, "null loss pointer");
    GF_CHECK_ARG_AS(fn, scratch, "null scratch pointer");
    size_t need = 0;
    OccScalWs sw{};
    const OccWs ws = carve(workspace, scratch, L, N, nullptr, &need, scal ? &sw : nullptr);
    GF_CHECK_WORKSPACE_AS(fn, "scratch", scratch_bytes, need);
    sw.sem_w = sem_scal_weight;
    sw.geo_w = geo_scal_weight;
    const hipStream_t stream = (hipStream_t)stream_;
    const OccParams a = make_params(L, N, flags, stride_c, stride_n, label, mask, class_weights, ce_weight, lovasz_weight,
                                    lovasz_ignore, ignore_index, empty_label);
    OccPreds preds{};
    for (int l = 0; l < L; ++l) preds.p[l] = pred[l];
    const int NB = num_blocks(N), T = num_tiles(N), S = L * kC;
    hipLaunchKernelGGL(gf_occ_clear_kernel, dim3(1), dim3(64), 0, stream, ws);
    hipLaunchKernelGGL(gf_occ_prep_kernel, dim3(NB), dim3(kVox), 0, stream, a, ws);
    hipLaunchKernelGGL(gf_occ_offsets_kernel, dim3(1), dim3(1024), 0, stream, NB, ws);
    if (scal)
        hipLaunchKernelGGL(gf_occ_main_kernel<OccScalWs>, dim3(NB, L), dim3(kVox), 0, stream, a, preds, ws, sw);
    else
        hipLaunchKernelGGL(gf_occ_main_kernel<>, dim3(NB, L), dim3(kVox), 0, stream, a, preds, ws);
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
    if (scal)
        hipLaunchKernelGGL(gf_occ_scal_sums_kernel, dim3(2 * S + kC), dim3(256), 0, stream, NB, 2 * S, sw);
    if (scal)
        hipLaunchKernelGGL(gf_occ_finalise_kernel<OccScalWs>, dim3(1), dim3(kFin), 0, stream, a, NB, T, ws, loss, sw);
    else
        hipLaunchKernelGGL(gf_occ_finalise_kernel<>, dim3(1), dim3(kFin), 0, stream, a, NB, T, ws, loss);
    GF_CHECK_LAUNCH_AS(fn);
    return GF_OK;
}

int backward(const char *fn, bool scal, int L, int N, int C, int flags, const float *const *pred, long long stride_c,
             long long stride_n, const long long *label, const unsigned char *mask, const float *class_weights, float ce_weight,
             float lovasz_weight, int lovasz_ignore, int ignore_index, int empty_label, const float *grad_loss,
             float *const *grad_pred, void *workspace, size_t workspace_bytes, void *stream_)
{
    int rc = check_common(fn, scal, L, N, C, flags, pred, stride_c, stride_n, label, mask, class_weights, empty_label, workspace,
                          workspace_bytes);
    if (rc != GF_OK) return rc;
    GF_CHECK_ARG_AS(fn, grad_loss && grad_pred, "null gradient pointer");
    for (int l = 0; l < L; ++l) GF_CHECK_ARG_AS(fn, grad_pred[l], "null gradient pointer of a layer");
    OccScalWs sw{};
    const OccWs ws = carve(workspace, nullptr, L, N, nullptr, nullptr, scal ? &sw : nullptr);
    const OccParams a = make_params(L, N, flags, stride_c, stride_n, label, mask, class_weights, ce_weight, lovasz_weight,
                                    lovasz_ignore, ignore_index, empty_label);
    OccPreds preds{};
    OccGrads grads{};
    for (int l = 0; l < L; ++l) {
        preds.p[l] = pred[l];
        grads.p[l] = grad_pred[l];
    }
    if (scal)
        hipLaunchKernelGGL(gf_occ_backward_kernel<OccScalWs>, dim3(num_blocks(N), L), dim3(kVox), 0, (hipStream_t)stream_, a,
                           preds, grads, grad_loss, ws, sw);
    else
        hipLaunchKernelGGL(gf_occ_backward_kernel<>, dim3(num_blocks(N), L), dim3(kVox), 0, (hipStream_t)stream_, a, preds,
                           grads, grad_loss, ws);
    GF_CHECK_LAUNCH_AS(fn);
    return GF_OK;
}

}  // namespace occ
}  // namespace gf

extern "C" size_t gf_occ_loss_workspace_bytes(int L, int N, int C, int flags)
{
    return gf::occ::region_bytes(L, N, C, flags, false);
}

extern "C" size_t gf_occ_loss_scratch_bytes(int L, int N, int C, int flags)
{
    return gf::occ::region_bytes(L, N, C, flags, true);
}

extern "C" int gf_occ_loss_forward(int L, int N, int C, int flags, const float *const *pred, long long stride_c,
                                   long long stride_n, const long long *label, const unsigned char *mask,
                                   const float *class_weights, float ce_weight, float lovasz_weight, int lovasz_ignore,
                                   int ignore_index, int empty_label, float *loss, void *workspace, size_t workspace_bytes,
                                   void *scratch, size_t scratch_bytes, void *stream)
{
    return gf::occ::forward(__func__, false, L, N, C, flags, pred, stride_c, stride_n, label, mask, class_weights, ce_weight,
                            lovasz_weight, 0.f, 0.f, lovasz_ignore, ignore_index, empty_label, loss, workspace, workspace_bytes,
                            scratch, scratch_bytes, stream);
}

extern "C" int gf_occ_loss_backward(int L, int N, int C, int flags, const float *const *pred, long long stride_c,
                                    long long stride_n, const long long *label, const unsigned char *mask,
                                    const float *class_weights, float ce_weight, float lovasz_weight, int lovasz_ignore,
                                    int ignore_index, int empty_label, const float *grad_loss, float *const *grad_pred,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    return gf::occ::backward(__func__, false, L, N, C, flags, pred, stride_c, stride_n, label, mask, class_weights, ce_weight,
                             lovasz_weight, lovasz_ignore, ignore_index, empty_label, grad_loss, grad_pred, workspace,
                             workspace_bytes, stream);
}

extern "C" int gf_occ_loss_scal_forward(int L, int N, int C, int flags, const float *const *pred, long long stride_c,
                                        long long stride_n, const long long *label, const unsigned char *mask,
                                        const float *class_weights, float ce_weight, float lovasz_weight, float sem_scal_weight,
                                        float geo_scal_weight, int lovasz_ignore, int ignore_index, int empty_label, float *loss,
                                        void *workspace, size_t workspace_bytes, void *scratch, size_t scratch_bytes, void *stream)
{
    return gf::occ::forward(__func__, true, L, N, C, flags, pred, stride_c, stride_n, label, mask, class_weights, ce_weight,
                            lovasz_weight, sem_scal_weight, geo_scal_weight, lovasz_ignore, ignore_index, empty_label, loss,
                            workspace, workspace_bytes, scratch, scratch_bytes, stream);
}

// the weights are folded into what the forward left in the workspace; they are taken here for the symmetry of the two lists
extern "C" int gf_occ_loss_scal_backward(int L, int N, int C, int flags, const float *const *pred, long long stride_c,
                                         long long stride_n, const long long *label, const unsigned char *mask,
                                         const float *class_weights, float ce_weight, float lovasz_weight, float sem_scal_weight,
                                         float geo_scal_weight, int lovasz_ignore, int ignore_index, int empty_label,
                                         const float *grad_loss, float *const *grad_pred, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    (void)sem_scal_weight;
    (void)geo_scal_weight;
    return gf::occ::backward(__func__, true, L, N, C, flags, pred, stride_c, stride_n, label, mask, class_weights, ce_weight,
                             lovasz_weight, lovasz_ignore, ignore_index, empty_label, grad_loss, grad_pred, workspace,
                             workspace_bytes, stream);
}
