// Farthest point sampling: what pointops.farthest_point_sampling computes for GaussianLifterV2 with random_sampling=False
// (model/lifter/gaussian_lifter_v2.py:233-251).  The contract, the exactness argument and the measured numbers: DESIGN.md §3.8.
//
// One workgroup per segment, one launch per call, no inter-workgroup waits.  The workgroup
//   1. takes the segment's bounding box,
//   2. counting-sorts the points by a 32^3 Morton cell (LDS histogram) into a working copy {x, y, z, index} + d in the workspace,
//   3. cuts the sorted order into buckets of 64 points (one wave-load each) and keeps, per bucket, its exact box and its exact
//      best key (largest d, then lowest index) with that point's coordinates -- in registers of the lane that owns the bucket,
//   4. per pick: every lane bounds the squared distance from the pick to each of its buckets' boxes from below; only buckets whose
//      bound is below their largest d are loaded and updated (by the whole wave), then the next pick is the workgroup's argmax of
//      the bucket keys: one wave reduction, one LDS exchange, one barrier.
// Bucket j belongs to wave j mod 16, so the Morton-adjacent buckets one pick touches land on different waves.
//
// Exactness: dist2 and the box bound are evaluated in the same fp32 operation order without contraction; rounding is monotone,
// so the bound never exceeds the distance of any point in the box and a skipped bucket holds no point whose d would change.
// The result does not depend on the sort order (which is not deterministic: LDS atomics) or on the bucket cut.
#include "gf_common.hpp"

namespace gf {

constexpr int kFpsThreads = 1024;                         // 16 waves
constexpr int kFpsWaves = kFpsThreads / 64;
constexpr int kFpsSlots = 4;                              // buckets per lane
constexpr int kFpsBucket = 64;                            // points per bucket
constexpr int kFpsMaxPoints = kFpsThreads * kFpsSlots * kFpsBucket;   // 262 144 per segment
constexpr int kFpsCells = 32 * 32 * 32;                   // Morton cells of the counting sort
constexpr int kFpsHistWords = kFpsCells + kFpsCells / 32; // one pad word per 32 bins: the scan reads them conflict-free
constexpr float kFpsInit = 1e10f;                         // initial d, as in pointops

static_assert(kFpsMaxPoints == 262144, "segment limit");

struct FpsArgs {
    const float *xyz;          // [n, 3]
    const int *offset;         // [b] device copies of the segment ends
    const int *new_offset;     // [b]
    int *idx;                  // [new_offset[b-1]]
    float4 *pts;               // workspace: [n] sorted {x, y, z, local index bits}
    float *d;                  // workspace: [n] running minimum squared distance, sorted order
    int exhaustive;            // gf_set_option("fps.exhaustive", 1): every bucket is updated on every pick
};

__device__ __forceinline__ int hist_slot(int bin) { return bin + (bin >> 5); }

// The contract's distance: ((dx*dx + dy*dy) + dz*dz), every operation rounded to fp32, no FMA.
__device__ __forceinline__ float fps_dist2(float px, float py, float pz, float cx, float cy, float cz)
{
#pragma clang fp contract(off)
    const float dx = px - cx, dy = py - cy, dz = pz - cz;
    return dx * dx + dy * dy + dz * dz;
}

// Lower bound of fps_dist2 over a box [lo, hi]: the same expression on the gaps.  If c < lo <= p then fl(p - c) >= fl(lo - c) >= 0,
// if p <= hi < c then |fl(p - c)| >= fl(c - hi) >= 0 (rounding is monotone and symmetric), and squares and sums of non-negative
// numbers round monotonically -- so the bound is <= fps_dist2(p, c) for every p in the box.
__device__ __forceinline__ float fps_box_bound(float lx, float ly, float lz, float hx, float hy, float hz, float cx, float cy, float cz)
{
#pragma clang fp contract(off)
    const float gx = fmaxf(fmaxf(lx - cx, cx - hx), 0.f);
    const float gy = fmaxf(fmaxf(ly - cy, cy - hy), 0.f);
    const float gz = fmaxf(fmaxf(lz - cz, cz - hz), 0.f);
    return gx * gx + gy * gy + gz * gz;
}

// A candidate: d as bits (d >= 0, so the bits order like the values), local index, coordinates.
struct Key {
    uint32_t d, i;
    float x, y, z;
};
__device__ __forceinline__ bool key_better(uint32_t d, uint32_t i, uint32_t bd, uint32_t bi) { return d > bd || (d == bd && i < bi); }

// The wave's best key (largest d, then lowest index), uniform over the wave.  Lanes without a point pass d = 0, i = ~0u.
__device__ __forceinline__ Key wave_best(uint32_t d, uint32_t i, float x, float y, float z)
{
    Key k;
    k.d = wave_reduce(d, MaxU());
    k.i = wave_reduce(d == k.d ? i : ~0u, MinU());
    const uint64_t hit = __ballot(d == k.d && i == k.i);
    const int l = hit ? __builtin_ctzll(hit) : 0;
    k.x = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), l));
    k.y = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(y), l));
    k.z = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(z), l));
    return k;
}

__device__ __forceinline__ int morton_cell(float v, float lo, float scale)
{
    return (int)fminf(fmaxf((v - lo) * scale, 0.f), 31.f);
}
__device__ __forceinline__ uint32_t spread3(uint32_t v)   // 5 bits -> every third bit
{
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 5; ++b) r |= ((v >> b) & 1u) << (3 * b);
    return r;
}

__global__ __launch_bounds__(kFpsThreads) void gf_fps_kernel(FpsArgs a)
{
    __shared__ uint32_t s_hist[kFpsHistWords];
    __shared__ float s_box[kFpsWaves][6];
    __shared__ uint32_t s_scan[kFpsWaves];
    __shared__ float s_slot[2][kFpsWaves][8];   // per pick, double-buffered: {d bits, index, x, y, z}

    const int seg = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int s0 = seg ? a.offset[seg - 1] : 0, n = a.offset[seg] - s0;
    const int o0 = seg ? a.new_offset[seg - 1] : 0, m = a.new_offset[seg] - o0;
    if (m <= 0 || n < 1 || n > kFpsMaxPoints) return;   // the host validated the offsets; a device copy that disagrees writes nothing
    const float *P = a.xyz + 3 * (size_t)s0;
    float4 *pts = a.pts + s0;
    float *dw = a.d + s0;
    int *out = a.idx + o0;
    if (t == 0) out[0] = s0;   // the first pick is the segment's first point
    if (m == 1) return;

    // ---- 1. bounding box
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int p = t; p < n; p += kFpsThreads) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = P[3 * p + c];
            lo[c] = fminf(lo[c], v);
            hi[c] = fmaxf(hi[c], v);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = __uint_as_float(wave_reduce(__float_as_uint(lo[c]), MinF()));
        hi[c] = __uint_as_float(wave_reduce(__float_as_uint(hi[c]), MaxF()));
    }
    if (lane == 0)
        for (int c = 0; c < 3; ++c) { s_box[w][c] = lo[c]; s_box[w][3 + c] = hi[c]; }
    for (int i = t; i < kFpsHistWords; i += kFpsThreads) s_hist[i] = 0;
    __syncthreads();
    float scale[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float l = s_box[0][c], h = s_box[0][3 + c];
        for (int v = 1; v < kFpsWaves; ++v) { l = fminf(l, s_box[v][c]); h = fmaxf(h, s_box[v][3 + c]); }
        lo[c] = l;
        scale[c] = h > l ? 32.f / (h - l) : 0.f;
    }
    auto cell_of = [&](float x, float y, float z) {
        return (int)(spread3(morton_cell(x, lo[0], scale[0])) | (spread3(morton_cell(y, lo[1], scale[1])) << 1) |
                     (spread3(morton_cell(z, lo[2], scale[2])) << 2));
    };

    // ---- 2. counting sort by Morton cell
    for (int p = t; p < n; p += kFpsThreads) atomicAdd(&s_hist[hist_slot(cell_of(P[3 * p], P[3 * p + 1], P[3 * p + 2]))], 1u);
    __syncthreads();
    {
        constexpr int kPer = kFpsCells / kFpsThreads;   // 32 consecutive bins per thread
        uint32_t v[kPer], sum = 0;
#pragma unroll
        for (int i = 0; i < kPer; ++i) { v[i] = s_hist[hist_slot(t * kPer + i)]; sum += v[i]; }
        uint32_t incl = sum;   // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o);
            if (lane >= o) incl += u;
        }
        if (lane == 63) s_scan[w] = incl;
        __syncthreads();
        uint32_t base = incl - sum;
        for (int v2 = 0; v2 < w; ++v2) base += s_scan[v2];
#pragma unroll
        for (int i = 0; i < kPer; ++i) { s_hist[hist_slot(t * kPer + i)] = base; base += v[i]; }
    }
    __syncthreads();
    for (int p = t; p < n; p += kFpsThreads) {
        const float x = P[3 * p], y = P[3 * p + 1], z = P[3 * p + 2];
        const uint32_t q = atomicAdd(&s_hist[hist_slot(cell_of(x, y, z))], 1u);
        pts[q] = make_float4(x, y, z, __uint_as_float((uint32_t)p));
        dw[q] = kFpsInit;
    }
    __syncthreads();   // the working copy is written by this workgroup only: workgroup-scope visibility suffices

    // ---- 3. buckets: lane l of wave w owns buckets j = k * 1024 + l * 16 + w, k < 4
    const int nbk = (n + kFpsBucket - 1) / kFpsBucket;
    float blo[kFpsSlots][3], bhi[kFpsSlots][3];
    Key bk[kFpsSlots];
#pragma unroll
    for (int k = 0; k < kFpsSlots; ++k) {
        for (int c = 0; c < 3; ++c) { blo[k][c] = INFINITY; bhi[k][c] = -INFINITY; }
        bk[k] = Key{0u, ~0u, 0.f, 0.f, 0.f};   // an empty bucket: d = 0 is never above a bound
        for (int l = 0; l < 64; ++l) {
            const int j = k * kFpsThreads + l * kFpsWaves + w;
            if (j >= nbk) break;   // uniform over the wave
            const int p = j * kFpsBucket + lane;
            const bool ok = p < n;
            const float4 q = ok ? pts[p] : make_float4(0.f, 0.f, 0.f, 0.f);
            float bl[3], bh[3];
            const float qc[3] = {q.x, q.y, q.z};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                bl[c] = __uint_as_float(wave_reduce(__float_as_uint(ok ? qc[c] : INFINITY), MinF()));
                bh[c] = __uint_as_float(wave_reduce(__float_as_uint(ok ? qc[c] : -INFINITY), MaxF()));
            }
            const Key key = wave_best(ok ? __float_as_uint(kFpsInit) : 0u, ok ? __float_as_uint(q.w) : ~0u, q.x, q.y, q.z);
            if (lane == l) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { blo[k][c] = bl[c]; bhi[k][c] = bh[c]; }
                bk[k] = key;
            }
        }
    }

    // ---- 4. picks
    float cx = P[0], cy = P[1], cz = P[2];
    for (int it = 1; it < m; ++it) {
#pragma unroll
        for (int k = 0; k < kFpsSlots; ++k) {
            const bool need = a.exhaustive ? blo[k][0] <= bhi[k][0]   // every non-empty bucket
                                           : fps_box_bound(blo[k][0], blo[k][1], blo[k][2], bhi[k][0], bhi[k][1], bhi[k][2], cx, cy, cz) <
                                                 __uint_as_float(bk[k].d);
            uint64_t mask = __ballot(need);
            while (mask) {
                const int l = __builtin_ctzll(mask);
                mask &= mask - 1;
                const int p = (k * kFpsThreads + l * kFpsWaves + w) * kFpsBucket + lane;
                const bool ok = p < n;
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                float d = 0.f;
                if (ok) {
                    q = pts[p];
                    const float old = dw[p];
                    d = fminf(old, fps_dist2(q.x, q.y, q.z, cx, cy, cz));
                    if (d < old) dw[p] = d;
                }
                const Key key = wave_best(__float_as_uint(d), ok ? __float_as_uint(q.w) : ~0u, q.x, q.y, q.z);
                if (lane == l) bk[k] = key;
            }
        }
        // the lane's best bucket, the wave's, then the workgroup's
        Key b = bk[0];
#pragma unroll
        for (int k = 1; k < kFpsSlots; ++k)
            if (key_better(bk[k].d, bk[k].i, b.d, b.i)) b = bk[k];
        const Key wb = wave_best(b.d, b.i, b.x, b.y, b.z);
        float *slot = s_slot[it & 1][w];
        if (lane == 0) {
            slot[0] = __uint_as_float(wb.d); slot[1] = __uint_as_float(wb.i);
            slot[2] = wb.x; slot[3] = wb.y; slot[4] = wb.z;
        }
        __syncthreads();
        uint32_t gd = __float_as_uint(s_slot[it & 1][0][0]), gi = __float_as_uint(s_slot[it & 1][0][1]);
        int gw = 0;
#pragma unroll
        for (int v = 1; v < kFpsWaves; ++v) {
            const uint32_t d = __float_as_uint(s_slot[it & 1][v][0]), i = __float_as_uint(s_slot[it & 1][v][1]);
            if (key_better(d, i, gd, gi)) { gd = d; gi = i; gw = v; }
        }
        cx = s_slot[it & 1][gw][2]; cy = s_slot[it & 1][gw][3]; cz = s_slot[it & 1][gw][4];
        if (t == 0) out[it] = s0 + (int)gi;
    }
}

}  // namespace gf

// the workspace is ONE section: the points as float4 and, where they end (no rounding up in between), their distances
static size_t fps_carve(void *workspace, int n, gf::FpsArgs *a)
{
    gf::Carver c(workspace);
    char *s = c.take<char>((size_t)n * (sizeof(float4) + sizeof(float)));
    if (s) { a->pts = (float4 *)s; a->d = (float *)(s + (size_t)n * sizeof(float4)); }
    return c.bytes();
}

extern "C" size_t gf_fps_workspace_bytes(int n)
{
    return n < 0 ? 0 : fps_carve(nullptr, n, nullptr);
}

extern "C" int gf_farthest_point_sampling(int n, int b, const int *offset_host, const int *new_offset_host, const float *xyz,
                                          const int *offset, const int *new_offset, int *idx, void *workspace,
                                          size_t workspace_bytes, void *stream_)
{
    using namespace gf;
    GF_CHECK_ARG(n >= 0 && b >= 1, "bad sizes (n >= 0, b >= 1)");
    GF_CHECK_ARG(offset_host && new_offset_host, "null host offsets");
    int prev = 0, prev_new = 0;
    for (int s = 0; s < b; ++s) {
        const int ns = offset_host[s] - prev, ms = new_offset_host[s] - prev_new;
        if (ns < 0 || ms < 0) {
            set_error("gf_farthest_point_sampling: offsets must be non-decreasing (segment %d: offset %d after %d, new_offset %d after %d)",
                      s, offset_host[s], prev, new_offset_host[s], prev_new);
            return GF_EINVAL;
        }
        if (ns == 0 && ms > 0) {
            set_error("gf_farthest_point_sampling: segment %d is empty but asks for %d picks", s, ms);
            return GF_EINVAL;
        }
        if (ns > kFpsMaxPoints) {
            set_error("gf_farthest_point_sampling: segment %d has %d points; the limit is %d points per segment", s, ns, kFpsMaxPoints);
            return GF_EINVAL;
        }
        prev = offset_host[s];
        prev_new = new_offset_host[s];
    }
    GF_CHECK_ARG(prev == n, "offset[b-1] must equal n");
    if (prev_new == 0) return GF_OK;
    GF_CHECK_ARG(xyz && offset && new_offset && idx && workspace, "null pointer");
    FpsArgs a{};
    const size_t need = fps_carve(workspace, n, &a);
    GF_CHECK_WORKSPACE(workspace_bytes, need);
    a.xyz = xyz; a.offset = offset; a.new_offset = new_offset; a.idx = idx;
    a.exhaustive = option(kOptFpsExhaustive) != 0;
    hipLaunchKernelGGL(gf_fps_kernel, dim3(b), dim3(kFpsThreads), 0, (hipStream_t)stream_, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
