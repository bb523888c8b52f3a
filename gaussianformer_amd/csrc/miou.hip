// The evaluation metric's per-frame step (misc/metric_util.py:35-66, MeanIoU._after_step) without a host read: the reference
// compacts outputs and targets by boolean indexing and then, per class, reads three torch.sum(...).item() back -- 51 round trips a
// frame -- and with filter_minmax two nonzero() calls.  Here a frame is two launches on the caller's stream:
//   counting pass  every workgroup walks one contiguous run of voxels and counts, per z slice (z = n % D), in a table in LDS
//                  (integer LDS adds), then stores the table plainly to its own slot of the workspace: no global atomics, and
//                  nothing in the workspace has to be zero beforehand.  The prediction is an int64 label tensor, or it is formed
//                  from the head's [N,18] logits by gf_head_labels' own rule (gf_labels.hpp) and never written.
//   finish pass    one workgroup sums the slots, takes min_z / max_z from the occupancy words, applies the z
//                  filter by arithmetic, maps the table onto class_indices and the occupied / empty aggregate and ADDS the result
//                  to the caller's int64 totals.
// Everything is integer arithmetic: any order of the adds gives the same bits.
//
// What a slice's table holds (kZW words): over the KEPT voxels (mask) the marginal counts by target and by prediction, the
// diagonal target == prediction, and the three aggregate counts; over ALL voxels whether any target is occupied -- the reference
// takes min_z / max_z from the unmasked targets (:44-46) and masks afterwards (:49-51).  Marginals and diagonal are all of the
// joint (target, prediction) table that the totals need, with or without the filter: in a slice outside [min_z, max_z] every
// kept prediction counts as empty_label (:47-48), which moves the slice's whole kept count to that class and leaves of the
// diagonal the targets that are empty_label.
#include "gf_labels.hpp"

namespace gf {

constexpr int kMiouBuckets = GF_MIOU_MAX_CLASSES + 1;   // label values 0..31, and one bucket for every other value (255 occurs in the data)
constexpr int kZT = 0, kZO = kMiouBuckets, kZDiag = 2 * kMiouBuckets;            // [33] by target, [33] by prediction, [32] both equal
constexpr int kZTOcc = kZDiag + GF_MIOU_MAX_CLASSES, kZOOcc = kZTOcc + 1, kZBoth = kZTOcc + 2;   // target / prediction / both != empty_label
constexpr int kZAny = kZTOcc + 3;                       // any target of the slice occupied, masked or not (0 / 1)
constexpr int kZW = 104;                                // words per slice (kZAny + 1 = 102, rounded up to whole 16-byte pieces)
static_assert(kZAny < kZW && kZW % 4 == 0, "the slice's words fit");
constexpr int kMiouThreads = 1024;                      // the counting pass on labels (two voxels per thread and step) and the finish pass
constexpr int kMiouLogitThreads = 512;                  // the counting pass on logits: 8 waves' rows (36 864 B) and the largest table fit 64 KB of LDS
constexpr int kMiouRun = 2 * kMiouThreads;              // a workgroup's run of voxels is a multiple of this
constexpr long long kMiouMaxN = (1ll << 31) - 2 * kMiouRun;   // voxel indices, one step past the end included, stay ints
constexpr int kMiouSlotWords = 128 * 16 * kZW;          // the finish pass, one workgroup, reads at most so many words of slots (832 KB): 128 slots
                                                        // of 16 slices, more of fewer -- 1024 at most -- so that without the filter (one slice) the
                                                        // evaluation's 640 000 voxels are 313 workgroups of one step each

struct MiouArgs {
    const long long *outputs;   // [N] labels, or null: the logits path
    const float *logits;        // [N,18]
    const float *bin_logits;    // [N] (prob modes)
    const void *targets;        // [N] int64, or uint8 with GF_MIOU_TARGETS_U8
    const unsigned char *mask;  // [N] or null
    uint32_t *slots;            // [blocks][D * kZW]
    long long *totals;          // [3][num_classes + 1]: seen, correct, positive
    long long *status;          // [2]: frames counted, frames whose filter found no occupied target
    int N, D, run, blocks;      // D: 1 unless the filter is on
    int flags, mode, empty_label, dataset_empty_label, num_classes;
    float threshold;
    int cls[GF_MIOU_MAX_CLASSES];
};

__device__ __forceinline__ void count_voxel(uint32_t *tab, int z, long long o, long long t, bool kept, const MiouArgs &a)
{
    if ((a.flags & GF_MIOU_REMAP) && t == a.dataset_empty_label) t = a.empty_label;   // :43
    uint32_t *s = tab + z * kZW;
    const bool t_occ = t != a.empty_label, o_occ = o != a.empty_label;
    if (t_occ) atomicOr(&s[kZAny], 1u);
    if (!kept) return;
    const int tb = (unsigned long long)t < (unsigned long long)GF_MIOU_MAX_CLASSES ? (int)t : GF_MIOU_MAX_CLASSES;
    const int ob = (unsigned long long)o < (unsigned long long)GF_MIOU_MAX_CLASSES ? (int)o : GF_MIOU_MAX_CLASSES;
    atomicAdd(&s[kZT + tb], 1u);
    atomicAdd(&s[kZO + ob], 1u);
    if (t == o && tb < GF_MIOU_MAX_CLASSES) atomicAdd(&s[kZDiag + tb], 1u);
    if (t_occ) atomicAdd(&s[kZTOcc], 1u);
    if (o_occ) atomicAdd(&s[kZOOcc], 1u);
    if (t_occ && o_occ) atomicAdd(&s[kZBoth], 1u);
}

__device__ __forceinline__ long long target_at(const MiouArgs &a, int n)
{
    return (a.flags & GF_MIOU_TARGETS_U8) ? (long long)((const unsigned char *)a.targets)[n] : ((const long long *)a.targets)[n];
}

// Two neighbouring voxels n, n + 1 (n even; the second only where n + 1 < last): an int64 pair is one 16-byte load where the tensor's base allows it.
struct VoxelPair {
    long long o0, o1, t0, t1;
    bool k0, k1;
};
__device__ __forceinline__ VoxelPair load_pair(const MiouArgs &a, int n, int last, bool vec_o, bool vec_t)
{
    VoxelPair p{};
    const bool two = n + 1 < last;
    if (two && vec_o) {
        const longlong2 v = *reinterpret_cast<const longlong2 *>(a.outputs + n);
        p.o0 = v.x; p.o1 = v.y;
    } else {
        p.o0 = a.outputs[n];
        if (two) p.o1 = a.outputs[n + 1];
    }
    if (two && vec_t) {
        const longlong2 v = *reinterpret_cast<const longlong2 *>((const long long *)a.targets + n);
        p.t0 = v.x; p.t1 = v.y;
    } else {
        p.t0 = target_at(a, n);
        if (two) p.t1 = target_at(a, n + 1);
    }
    p.k0 = a.mask ? a.mask[n] != 0 : true;
    p.k1 = a.mask && two ? a.mask[n + 1] != 0 : true;
    return p;
}

// LOGITS: the prediction is row_label() of the logits' row (the wave stages 64 rows at a time, one voxel per lane); otherwise two
// int64 labels per lane and step, one 16-byte load where the tensor's base allows it.
template <bool LOGITS, int THREADS>
__global__ __launch_bounds__(THREADS) void gf_miou_count_kernel(MiouArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
    uint32_t *tab = s_dyn;                                   // [D * kZW]
    const int words = a.D * kZW;
    for (int w = threadIdx.x; w < words; w += THREADS) tab[w] = 0u;
    __syncthreads();
    const int first = blockIdx.x * a.run;                    // < N
    const int last = (int)min((long long)a.N, (long long)first + a.run);
    if (LOGITS) {
        float *rows_lds = reinterpret_cast<float *>(s_dyn + words);   // [waves][kLabelRowsLds]
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        float *mine = rows_lds + wave * kLabelRowsLds;
        const bool vec_ok = ((uintptr_t)a.logits & 15) == 0;
        for (int n0 = first + wave * 64; n0 < last; n0 += THREADS) {
            const int rows = min(64, last - n0);
            const int n = n0 + min(lane, rows - 1);
            const float bin = a.mode != 0 ? a.bin_logits[n] : 0.f;
            const long long t = target_at(a, n);
            const bool kept = a.mask ? a.mask[n] != 0 : true;
            stage_label_rows(a.logits + (long long)n0 * kC, rows, vec_ok, lane, mine);
            if (lane < rows) count_voxel(tab, n % a.D, row_label(mine + lane * kC, bin, a.mode, a.threshold, a.empty_label), t, kept, a);
            wave_lds_handover();   // the rows are read before the next step's overwrite them
        }
    } else {
        const bool vec_o = ((uintptr_t)a.outputs & 15) == 0;
        const bool vec_t = !(a.flags & GF_MIOU_TARGETS_U8) && ((uintptr_t)a.targets & 15) == 0;
        // the next step's loads are requested before this step's voxels are counted
        int n = first + 2 * (int)threadIdx.x;   // even: first is a multiple of kMiouRun
        VoxelPair cur = n < last ? load_pair(a, n, last, vec_o, vec_t) : VoxelPair{};
        while (n < last) {
            const int next = n + 2 * THREADS;
            const VoxelPair nxt = next < last ? load_pair(a, next, last, vec_o, vec_t) : VoxelPair{};
            const int z0 = n % a.D;
            count_voxel(tab, z0, cur.o0, cur.t0, cur.k0, a);
            if (n + 1 < last) count_voxel(tab, z0 + 1 == a.D ? 0 : z0 + 1, cur.o1, cur.t1, cur.k1, a);
            cur = nxt;
            n = next;
        }
    }
    __syncthreads();
    uint32_t *slot = a.slots + (size_t)blockIdx.x * words;
    for (int w = threadIdx.x; w < words; w += THREADS) slot[w] = tab[w];
}

__global__ __launch_bounds__(kMiouThreads) void gf_miou_finish_kernel(MiouArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
    uint32_t *tab = s_dyn;   // [D * kZW]: the frame's table (a count is at most N < 2^31)
    __shared__ int s_min, s_max;
    const int words = a.D * kZW;
    for (int w = threadIdx.x; w < words; w += kMiouThreads) tab[w] = 0u;
    __syncthreads();
    // the slots as one run of 16-byte pieces over all threads (a word per thread summing its column slot by slot was one dependent
    // load after the other: 26 us at 105 slots); most words are 0, the others go to the table by LDS integer adds
    const int pieces = a.blocks * (words / 4), wrap = words / 4, step = kMiouThreads % wrap;
    const uint4 *src = reinterpret_cast<const uint4 *>(a.slots);
    int w4 = threadIdx.x % wrap;   // the piece's place in its slot
#pragma unroll 4
    for (int i = threadIdx.x; i < pieces; i += kMiouThreads) {
        const uint4 v = src[i];
        if (v.x) atomicAdd(&tab[4 * w4], v.x);
        if (v.y) atomicAdd(&tab[4 * w4 + 1], v.y);
        if (v.z) atomicAdd(&tab[4 * w4 + 2], v.z);
        if (v.w) atomicAdd(&tab[4 * w4 + 3], v.w);
        w4 += step;
        if (w4 >= wrap) w4 -= wrap;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int lo = a.D, hi = -1;   // min_z / max_z of the occupied targets (:45-46); none: hi < lo
        for (int z = 0; z < a.D; ++z)
            if (tab[z * kZW + kZAny]) { lo = min(lo, z); hi = z; }
        const bool filter = (a.flags & GF_MIOU_FILTER_MINMAX) != 0;
        // no occupied target: the reference raises on .max() of an empty tensor; the frame is counted without the filter
        s_min = filter && hi >= 0 ? lo : 0;
        s_max = filter && hi >= 0 ? hi : a.D - 1;
        a.status[0] += 1;
        if (filter && hi < 0) a.status[1] += 1;
    }
    __syncthreads();
    const int K1 = a.num_classes + 1;
    if ((int)threadIdx.x >= 3 * K1) return;
    const int r = threadIdx.x / K1, i = threadIdx.x % K1;   // row: 0 seen, 1 correct, 2 positive; i == num_classes: the aggregate
    const int c = i < a.num_classes ? a.cls[i] : -1;
    long long sum = 0;
    for (int z = 0; z < a.D; ++z) {
        const uint32_t *s = tab + z * kZW;
        const bool inside = z >= s_min && z <= s_max;
        if (r == 0) {
            sum += c >= 0 ? s[kZT + c] : s[kZTOcc];
        } else if (inside) {
            sum += r == 1 ? (c >= 0 ? s[kZDiag + c] : s[kZBoth]) : (c >= 0 ? s[kZO + c] : s[kZOOcc]);
        } else if (c >= 0 && c == a.empty_label) {   // every kept prediction of the slice reads empty_label (:47-48)
            if (r == 1) {
                sum += s[kZT + c];
            } else {
                for (int b = 0; b < kMiouBuckets; ++b) sum += s[kZT + b];
            }
        }
    }
    a.totals[r * K1 + i] += sum;
}

// the workgroups of a frame of D slices and the voxels each takes
inline void miou_grid(long long N, int D, int &blocks, int &run)
{
    const int slots = kMiouSlotWords / (D * kZW) < 1024 ? kMiouSlotWords / (D * kZW) : 1024;   // >= 32 (D <= GF_MIOU_MAX_D)
    const long long steps = (N + kMiouRun - 1) / kMiouRun, per = (steps + slots - 1) / slots;
    run = (int)(per * kMiouRun);
    blocks = N > 0 ? (int)((N + run - 1) / run) : 0;
}

inline bool miou_sizes_ok(long long N, int D, int flags)
{
    if (N < 0 || N > kMiouMaxN || (flags & ~(GF_MIOU_TARGETS_U8 | GF_MIOU_FILTER_MINMAX | GF_MIOU_REMAP))) return false;
    return !(flags & GF_MIOU_FILTER_MINMAX) || (D >= 1 && D <= GF_MIOU_MAX_D && N % D == 0);
}

inline size_t miou_carve(void *base, long long N, int D, int flags, uint32_t *&slots)
{
    int blocks, run;
    D = (flags & GF_MIOU_FILTER_MINMAX) ? D : 1;
    miou_grid(N, D, blocks, run);
    Carver c(base);
    slots = c.take<uint32_t>((size_t)(blocks > 0 ? blocks : 1) * D * kZW);   // (never empty: a size of 0 is the query's refusal)
    return c.bytes();
}

static int miou_step(const char *fn, bool from_logits, long long N, int D, int flags, const long long *outputs, int C, int mode, const float *logits,
                     const float *bin_logits, float threshold, const void *targets, const unsigned char *mask, int num_classes,
                     const int *class_indices_host, int empty_label, int dataset_empty_label, long long *totals, long long *status,
                     void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    GF_CHECK_ARG_AS(fn, N >= 0 && N <= kMiouMaxN, "bad size");
    GF_CHECK_ARG_AS(fn, !(flags & ~(GF_MIOU_TARGETS_U8 | GF_MIOU_FILTER_MINMAX | GF_MIOU_REMAP)), "unknown flag");
    if (from_logits) {
        GF_CHECK_ARG_AS(fn, C == kC, "only 18 semantic channels are supported (NUM_CHANNELS)");
        GF_CHECK_ARG_AS(fn, mode == GF_LABELS_ARGMAX || mode == GF_LABELS_PROB_THRESHOLD || mode == GF_LABELS_PROB_GEOSEM, "unknown mode");
    }
    GF_CHECK_ARG_AS(fn, num_classes >= 1 && num_classes <= GF_MIOU_MAX_CLASSES, "num_classes must be 1..32");
    GF_CHECK_ARG_AS(fn, class_indices_host && totals && status, "null pointer");
    for (int i = 0; i < num_classes; ++i)
        GF_CHECK_ARG_AS(fn, class_indices_host[i] >= 0 && class_indices_host[i] < GF_MIOU_MAX_CLASSES, "a class index is outside [0, 32)");
    if (flags & GF_MIOU_FILTER_MINMAX) {
        GF_CHECK_ARG_AS(fn, D >= 1 && D <= GF_MIOU_MAX_D, "filter_minmax needs 1 <= D <= 64");
        GF_CHECK_ARG_AS(fn, N % D == 0, "filter_minmax needs N to be a multiple of D");
    }
    if (N > 0) {
        GF_CHECK_ARG_AS(fn, targets && (from_logits ? (const void *)logits : (const void *)outputs), "null pointer");
        GF_CHECK_ARG_AS(fn, !from_logits || mode == GF_LABELS_ARGMAX || bin_logits, "the prob modes need bin_logits");
    }
    MiouArgs a{};
    uint32_t *slots;
    GF_CHECK_WORKSPACE_AS(fn, "workspace", workspace ? workspace_bytes : (size_t)0, miou_carve(nullptr, N, D, flags, slots));
    miou_carve(workspace, N, D, flags, slots);
    a.outputs = outputs; a.logits = logits; a.bin_logits = bin_logits; a.targets = targets; a.mask = mask; a.slots = slots;
    a.totals = totals; a.status = status; a.N = (int)N; a.D = (flags & GF_MIOU_FILTER_MINMAX) ? D : 1;
    miou_grid(N, a.D, a.blocks, a.run);
    a.flags = flags; a.mode = mode; a.empty_label = empty_label; a.dataset_empty_label = dataset_empty_label;
    a.num_classes = num_classes; a.threshold = threshold;
    for (int i = 0; i < num_classes; ++i) a.cls[i] = class_indices_host[i];
    const size_t tab_bytes = (size_t)a.D * kZW * sizeof(uint32_t);   // <= 26 624
    if (a.blocks > 0) {
        if (from_logits) {
            const size_t lds = tab_bytes + (size_t)(kMiouLogitThreads / 64) * kLabelRowsLds * sizeof(float);   // (kZW: whole 16-byte pieces)
            hipLaunchKernelGGL((gf_miou_count_kernel<true, kMiouLogitThreads>), dim3((unsigned)a.blocks), dim3(kMiouLogitThreads), lds, stream, a);
        } else {
            hipLaunchKernelGGL((gf_miou_count_kernel<false, kMiouThreads>), dim3((unsigned)a.blocks), dim3(kMiouThreads), tab_bytes, stream, a);
        }
        GF_CHECK_LAUNCH_AS(fn);
    }
    hipLaunchKernelGGL(gf_miou_finish_kernel, dim3(1), dim3(kMiouThreads), tab_bytes, stream, a);   // N == 0: counts the frame
    GF_CHECK_LAUNCH_AS(fn);
    return GF_OK;
}

}  // namespace gf

extern "C" size_t gf_miou_workspace_size(long long N, int D, int flags)
{
    uint32_t *slots;
    return gf::miou_sizes_ok(N, D, flags) ? gf::miou_carve(nullptr, N, D, flags, slots) : 0;
}

extern "C" int gf_miou_step(long long N, int D, int flags, const long long *outputs, const void *targets, const unsigned char *mask,
                            int num_classes, const int *class_indices_host, int empty_label, int dataset_empty_label,
                            long long *totals, long long *status, void *workspace, size_t workspace_bytes, void *stream)
{
    return gf::miou_step(__func__, false, N, D, flags, outputs, 0, 0, nullptr, nullptr, 0.f, targets, mask, num_classes, class_indices_host,
                         empty_label, dataset_empty_label, totals, status, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int gf_miou_step_logits(long long N, int D, int flags, int C, int mode, const float *logits, const float *bin_logits,
                                   float threshold, const void *targets, const unsigned char *mask, int num_classes,
                                   const int *class_indices_host, int empty_label, int dataset_empty_label, long long *totals,
                                   long long *status, void *workspace, size_t workspace_bytes, void *stream)
{
    return gf::miou_step(__func__, true, N, D, flags, nullptr, C, mode, logits, bin_logits, threshold, targets, mask, num_classes,
                         class_indices_host, empty_label, dataset_empty_label, totals, status, workspace, workspace_bytes,
                         (hipStream_t)stream);
}
