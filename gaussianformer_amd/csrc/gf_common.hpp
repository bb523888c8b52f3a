// gf_common.hpp -- what is about the library and the splat workspace: options, constants, record layout, workspace carve-up,
// error macros, a splat call's inputs and grid arithmetic on the host (gfx950 only).  The kernels' shared device helpers are in gf_wave.hpp and gf_math.hpp, included here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gf_hip.h"
#include "gf_math.hpp"
#include "gf_wave.hpp"

namespace gf {

// ---- library options (gf_set_option, include/gf_hip.h): explicit calls, never the environment -- the library does not call getenv
enum Option {
    kOptSplatTileKernel = 0,   // "splat.mfma_tile_kernel": matrix-core forward on the tile kernel where the wave kernel would apply
    kOptDafBackwardTiles,      // "daf.backward_tiles": gf_daf_backward_sorted by pixel tiles (round 1) instead of by image regions
    kOptSubmF32Mfma,           // "subm.f32_mfma": gf_subm_conv_apply on the exact-f32 MFMA kernel instead of the 3 x bf16 split
    kOptSubmTileGemm,          // "subm.tile_gemm": gf_subm_conv_apply's gather-GEMM with one tile per workgroup also where runs of tiles apply
    kOptSubmBf16x3,            // "subm.bf16x3": gf_subm_conv_apply_scratch on the three-term bf16 split (six products) instead of two f16 terms (three)
    kOptFpsExhaustive,         // "fps.exhaustive": gf_farthest_point_sampling updates every bucket on every pick (no pruning; same bits)
    kOptCount
};
int option(int which);           // gf_api.hip; 0 unless set

// ---- geometry constants -------------------------------------------------------------
constexpr int kC = GF_NUM_CHANNELS;  // 18 semantic channels
constexpr int kSuper = 8;            // a supertile is 8x8 voxel columns (the binning granule)
constexpr int kTileX = 8, kTileY = 4;  // a tile (one workgroup) is 8x4 voxel columns x all z; a brick is 4x4x4
constexpr int kTilesPerSuper = (kSuper / kTileX) * (kSuper / kTileY);
constexpr int kRecDwords = 32;       // packed per-Gaussian record, 128 B
constexpr int kWRow = 618;           // bitmask row words (P <= 39 552) the wave-autonomous matrix-core kernels (forward and backward) hold in LDS
constexpr int kLongWords = 4096;     // ... and the longest rows (P <= 262 144) their long-row instantiations take: the records pass then leaves, per
                                     // supertile, a SUMMARY of its bitmask row -- one byte per four words, bit k = "word 4 i + k is not zero" -- and
                                     // a unit fetches the non-zero words only (round 6; splat_fwd.hip, "long rows")
constexpr int kBwdRowDwords = 32;    // matrix-core backward: one 128-B row of partial gradients per (Gaussian, double brick)
constexpr int kBwdBigRows = 512;     // ... a Gaussian with more rows than this is summed by whole workgroups (big list)
constexpr int kBwdBigCap = 4608;     // ... layout words: one per wave of 64 Gaussians (<= kLongWords), then the table of big Gaussians (splat_bwd_mfma.hip)
constexpr int kBwdList = 256;       // candidate-list entries of the matrix-core backward (and of a list the forward publishes for it)
constexpr int kBwdPubLong = 896;    // ... entries of a list the forward's long-row instantiation publishes (its whole one-pass list; the backward
                                    // takes it in pieces of kBwdList)

// ---- protocol words: the splat's state block and the workspace's flag section, each named here once (the two tables: DESIGN.md §3.3d)
// The state block (include/gf_hip.h, gf_splat_state_bytes): thread 0 of the forward's render kernel writes it, the backward's kernels read it.
constexpr int kStateNotDense = GF_STATE_NOT_DENSE, kStatePath = GF_STATE_PATH, kStateVerdict = GF_STATE_VERDICT, kStateGen = GF_STATE_GENERATION, kStateRows = GF_STATE_ROWS;
constexpr uint32_t kRowsReady = GF_ROWS_READY, kRowsOverflow = GF_ROWS_OVERFLOW;
constexpr uint32_t kVerdictPoint = GF_VERDICT_POINT, kVerdictLattice = GF_VERDICT_LATTICE, kVerdictTheta = GF_VERDICT_THETA, kVerdictOpaSem = GF_VERDICT_OPASEM;
constexpr uint32_t kVerdictRange = kVerdictTheta | kVerdictOpaSem, kVerdictAll = kVerdictPoint | kVerdictLattice | kVerdictRange;  // every call's; with the point scans'
// Two predicates on VALUES: a kernel that requests all its words in one round trip and pins them (asm volatile "+s") calls them on what
// it loaded.  "A matrix-core body rendered the forward" (the two retired paths included: the kernels compare against all four) ...
constexpr __host__ __device__ __forceinline__ bool on_matrix_cores(uint32_t not_dense, uint32_t path)
{
    return not_dense == 0u && (path == (uint32_t)GF_PATH_MATRIX_CORE || path == (uint32_t)GF_PATH_MATRIX_CORE_WAVE ||
                               path == (uint32_t)GF_PATH_MATRIX_CORE_PAIR || path == (uint32_t)GF_PATH_MATRIX_CORE_SOLO);
}
static_assert(!on_matrix_cores(0, 0) && on_matrix_cores(0, 1) && !on_matrix_cores(0, 2) && on_matrix_cores(0, 3) && on_matrix_cores(0, 4) &&
              on_matrix_cores(0, 5) && !on_matrix_cores(1, 1) && !on_matrix_cores(1, 3), "GF_PATH_* 0..5: all but the exact tile and the arbitrary-points body");
// ... and "the workspace still holds the records and rows of the forward that wrote this state block" (words kStateGen, kStateRows; kGenWord)
constexpr __host__ __device__ __forceinline__ bool records_still_there(uint32_t state_gen, uint32_t state_rows, uint32_t gen) { return state_gen == gen && (state_rows & kRowsReady) != 0u; }
// The same on the words where they lie, for the two kernels that decide on nothing else (the records pass run for a backward, the backward's
// set-up kernel).  Not a wrapper: it asks for word kStateRows only once the generations agree, and three eager loads are another instruction
// stream (profiles/splat_protocol_words.txt).
__device__ __forceinline__ bool records_still_there(const uint32_t *state, const uint32_t *gen_word) { return state[kStateGen] == *gen_word && (state[kStateRows] & kRowsReady) != 0u; }

// The flag section: the first kFlagWords uint32 of a workspace (SplatWorkspace::flags).  Word indices; what lies between the regions is unused.
constexpr int kFlagWords = GF_SPLAT_FLAG_BYTES / 4;   // 8192
constexpr int kVerifyBase = 64, kVerifyBlocks = 4096;  // [base, + blocks): one dense-grid verdict word (bits 1 | 2 | 4) per verification wave of the records
                                                       // pass, render thread t reads 16 of them; PrepArgs / RenderArgs::verify_flags point at the base
constexpr int kCounterWords = 8 * 64;  // a block of per-XCD counters: XCD x's at [+ 64 x] (one cache line each) ...
constexpr int kFwdCounters = 4608;     // ... the matrix-core forward's tiles / units (armed by the records pass)
constexpr int kBwdCounters = 5632;     // ... the matrix-core backward's units (armed by the records pass that lays out its rows, re-armed by its last kernel)
constexpr int kGenWord = 8100;         // the workspace's generation -- the same word whatever the call's shape; every launch that rewrites the records (or
                                       // the sections they share with other shapes) bumps it
constexpr int kListsBad = 8101;        // a supertile's list did not fit kBwdList (the backward then scans the bitmask rows itself)
constexpr int kVerdictWords = 8104, kVerdictA = 0, kVerdictB = 1, kVerdictV = 2;   // the verdict block [A, B, V0, V1] of a workspace that was handed over
                                                                                   // zeroed (GF_WORKSPACE_ZEROED; splat_fwd.hip, "one verdict word")
static_assert(kVerifyBase + kVerifyBlocks <= kFwdCounters && kFwdCounters + kCounterWords <= kBwdCounters && kBwdCounters + kCounterWords <= kGenWord &&
              kGenWord < kListsBad && kListsBad < kVerdictWords && kVerdictWords + 4 <= kFlagWords, "flag-section regions are disjoint and inside the section");
static_assert(kVerdictWords % 4 == 0, "the verdict block is read with one 16-byte load");
constexpr __host__ __device__ uint32_t verdict_slot_after(uint32_t a) { return kVerdictV + ((a + 1u) & 1u); }   // V[(a + 1) & 1]: collects the violations found while A == a
// flag word k seen through the pointer to the verify region: how the kernels that hold it reach kGenWord and kListsBad without a further argument
template <class T> __host__ __device__ __forceinline__ T *flag_word_via_verify(T *verify_flags, int k) { return verify_flags + (k - kVerifyBase); }

// record layout (dwords)
//  0..2 mean xyz | 3 opacity | 4..9 cov (xx,yy,zz,xy,yz,xz) | 10 box lo | 11 box hi (excl.)
//  12..29 semantics[18] | 30 prob: (2pi)^-1.5 * sqrt(det) | 31 matrix-core backward: first row of the Gaussian's partial-gradient rows (uint32; forward: 0)
constexpr int kRecMean = 0, kRecOpa = 3, kRecCov = 4, kRecLo = 10, kRecHi = 11, kRecSem = 12,
              kRecKdet = 30;


// packed voxel coordinate: x | y<<11 | z<<22   (H,W <= 2047, D <= 1023)
__host__ __device__ __forceinline__ uint32_t pack3(int x, int y, int z)
{
    return (uint32_t)x | ((uint32_t)y << 11) | ((uint32_t)z << 22);
}
__host__ __device__ __forceinline__ int ux(uint32_t p) { return (int)(p & 2047u); }
__host__ __device__ __forceinline__ int uy(uint32_t p) { return (int)((p >> 11) & 2047u); }
__host__ __device__ __forceinline__ int uz(uint32_t p) { return (int)(p >> 22); }

// workspace carve-up (all sections 256-B aligned)
struct SplatWorkspace {
    uint32_t *flags;        // [kFlagWords] the flag section: see the map above ("protocol words")
    float *records;         // [P][32]
    uint2 *boxes;           // [P]  (lo, hi) packed
    unsigned long long *bitmask;  // [nsuper][nrow]: rows of nwords words, padded to an even count (16-byte aligned rows)
    unsigned char *summary;       // [nsuper][sum_pitch] long rows (kWRow < nrow, nwords <= kLongWords): byte i of a row = which of its words
                                  // 4 i .. 4 i + 3 are not zero (low four bits); null otherwise
    int sum_pitch;                // bytes per summary row (a multiple of 16)
    int *voxel2pts;         // [V]   (backward, general pts only)
    uint32_t *vols;         // [P]  backward: box volumes
    uint32_t *bsum;         // [ceil(P/256)] backward: volume sums per 256 Gaussians (sorted order)
    uint32_t *vols_in;      // [P]  backward: box volumes in input order
    int *order;             // [P]  backward: Gaussian index at each sorted position
    int *seg;               // [P][8] backward: (index, volume, box lo[3], box hi[3]) of the Gaussian at each sorted position
    uint32_t *sort_hist;    // [64][ceil(P/256)] + [64] backward: per-(cell, block) counts -> offsets, cell totals
    float *dotlg;           // [N]  prob backward: sum_c dL/dlogits[n][c] * logits[n][c]
    uint32_t *range_flags;  // [nwords + 4] forward, matrix-core kernel: per 64 Gaussians, 4 = theta range, 8 = opacity * semantics range
    uint32_t *bwd_wave_total;  // [kBwdBigCap] matrix-core backward: rows needed by each wave of 64 Gaussians (bit 31: one needs > kBwdBigRows)
    uint32_t *bwd_row_local;   // [P] ... a Gaussian's offset among its wave's rows (records pass)
    uint32_t *bwd_row_first;   // [P] ... its first row in bwd_rows (0xFFFFFFFF: no room) = prefix of the totals + offset
    uint32_t *bwd_lists;       // [nsuper][3][bwd_pub] ... every supertile's candidate list (ids, packed box lo, packed box hi), published by the forward
    int bwd_pub;               // ... entries per piece: kBwdList, or kBwdPubLong for long rows
    uint32_t *bwd_list_len;    // [nsuper] ... its length
    float *bwd_rows;        // [bwd_cap][32] matrix-core backward: partial gradients per (Gaussian, double brick)
    uint32_t bwd_cap;       // rows available (0: the shape does not take the matrix-core backward)
    int nwords, nrow, nsx, nsy, nsuper;
    size_t total_bytes;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// How every op cuts a caller-allocated region into 256-byte aligned sections, in ONE function that both sizes and carves: with a
// null base (a *_bytes size query) every section is null and only bytes() counts -- no arithmetic is done on a null pointer.
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(void *region) : base((char *)region) {}
    template <class T> T *take(size_t count) { T *r = base ? (T *)(base + off) : nullptr; off += align256(count * sizeof(T)); return r; }
    void skip(size_t nbytes) { off += nbytes; }  // a fixed header, taken as it is (not rounded up)
    size_t bytes() const { return off; }
};

inline SplatWorkspace carve_workspace(void *base, int P, int N, int H, int W, int D)
{
    SplatWorkspace ws;
    ws.nwords = (P + 63) / 64;
    ws.nrow = (ws.nwords + 1) & ~1;
    ws.nsx = (H + kSuper - 1) / kSuper;
    ws.nsy = (W + kSuper - 1) / kSuper;
    ws.nsuper = ws.nsx * ws.nsy;
    Carver c(base);
    ws.flags = c.take<uint32_t>(0); c.skip((size_t)kFlagWords * 4);
    ws.records = c.take<float>((size_t)P * kRecDwords);
    ws.boxes = c.take<uint2>((size_t)P);
    ws.bitmask = c.take<unsigned long long>((size_t)ws.nsuper * ws.nrow);
    {
        const bool long_rows = ws.nrow > kWRow && ws.nwords <= kLongWords;
        ws.sum_pitch = long_rows ? (((ws.nwords + 3) / 4 + 15) & ~15) : 0;
        ws.summary = long_rows ? c.take<unsigned char>((size_t)ws.nsuper * ws.sum_pitch) : nullptr;
    }
    ws.voxel2pts = c.take<int>((size_t)H * W * D);
    ws.vols = c.take<uint32_t>((size_t)P);
    ws.bsum = c.take<uint32_t>((size_t)((P + 255) / 256));
    ws.vols_in = c.take<uint32_t>((size_t)P);
    ws.order = c.take<int>((size_t)P);
    ws.seg = c.take<int>((size_t)P * 8);
    ws.sort_hist = c.take<uint32_t>((size_t)64 * ((P + 255) / 256) + 64);
    ws.dotlg = c.take<float>((size_t)(N > 0 ? N : 0));
    ws.range_flags = c.take<uint32_t>((size_t)(ws.nwords + 4));
    // matrix-core backward (rows of <= kWRow bitmask words): a Gaussian whose box meets k double bricks (4 x 4 x 8 voxels)
    // owns k rows; 16 per Gaussian on average plus two whole-grid Gaussians are provided for (the nuScenes configs need
    // ~13.5), what does not fit is accumulated with atomics instead
    {
        const long long nunits = (long long)ws.nsuper * 4 * ((D + 7) / 8);
        // (long rows, round 6: P > 39 552 means smaller Gaussians -- 6 rows each at nuscenes_gs144000 --, ten are provided for)
        const long long cap = ws.nrow <= kWRow ? 16ll * P + 2 * nunits + 1024 : ws.nwords <= kLongWords ? 10ll * P + 2 * nunits + 1024 : 0;
        ws.bwd_cap = (uint32_t)(cap < (1ll << 31) ? cap : (1ll << 31) - 1);
    }
    ws.bwd_wave_total = c.take<uint32_t>((size_t)kBwdBigCap);
    ws.bwd_row_local = c.take<uint32_t>((size_t)(ws.bwd_cap ? P : 0));
    ws.bwd_row_first = c.take<uint32_t>((size_t)(ws.bwd_cap ? P : 0));
    ws.bwd_pub = ws.nrow <= kWRow ? kBwdList : kBwdPubLong;
    ws.bwd_lists = c.take<uint32_t>((size_t)(ws.bwd_cap ? ws.nsuper : 0) * 3 * ws.bwd_pub);
    ws.bwd_list_len = c.take<uint32_t>((size_t)(ws.bwd_cap ? ws.nsuper : 0));
    ws.bwd_rows = c.take<float>((size_t)ws.bwd_cap * kBwdRowDwords);
    ws.total_bytes = c.bytes();
    return ws;
}

// ---- prob variant: det(Sigma^-1) and (2 pi)^-1.5 sqrt(det) -----------------------------
// model/head/localagg_prob/src/forward.cu:77-78, backward.cu:78-79:
//     deter = c0*c1*c2 + 2*c3*c4*c5 - c0*c4*c4 - c1*c5*c5 - c2*c3*c3;   powf(2 * 3.1415926535, -1.5) * powf(deter, 0.5)
// For an ill-conditioned Sigma^-1 (the Prob config's scales go down to 0.01 m) this sum cancels by up to twelve
// orders of magnitude: in fp32 every digit depends on which products the compiler fuses, and it can round
// negative (NaN, in the reference too).  Default = the reference's fp32 value: the fusion the compiled reference
// applies (first two terms one FMA, the three subtractions unfused; read off the gfx950 ISA of oracle/_ref),
// spelled out under `contract(off)` so it does not depend on this file's own optimisation context.
// `exact` (GF_PROB_EXACT_DET) evaluates it in fp64 instead: the value the expression approximates.
__device__ __forceinline__ float prob_det32(float c0, float c1, float c2, float c3, float c4, float c5)
{
#pragma clang fp contract(off)
    const float t = __builtin_fmaf(c0 * c1, c2, ((c3 + c3) * c4) * c5);
    return ((t - (c0 * c4) * c4) - (c1 * c5) * c5) - (c2 * c3) * c3;
}
__device__ __forceinline__ void prob_det_kdet(float c0, float c1, float c2, float c3, float c4, float c5, int exact,
                                              float &deter, float &kdet)
{
    if (exact) {
        const double d = (double)c0 * c1 * c2 + 2.0 * c3 * c4 * c5 - (double)c0 * c4 * c4 - (double)c1 * c5 * c5 - (double)c2 * c3 * c3;
        deter = (float)d;
        kdet = (float)(0.063493635934240969 * sqrt(d));  // (2 pi)^-1.5 sqrt(det)
    } else {
        deter = prob_det32(c0, c1, c2, c3, c4, c5);
        kdet = powf(2 * 3.1415926535, -1.5) * powf(deter, 0.5);
    }
}

// ---- error reporting ----------------------------------------------------------------
void set_error(const char *fmt, ...);
bool profile_slot(hipEvent_t *before, hipEvent_t *after);  // gf_api.hip

// (the _AS forms report under the name of the entry point that was called, where the check sits in a function it shares)
#define GF_CHECK_ARG_AS(fn, cond, msg)         \
    do {                                       \
        if (!(cond)) {                         \
            gf::set_error("%s: %s", fn, msg);  \
            return GF_EINVAL;                  \
        }                                      \
    } while (0)
#define GF_CHECK_ARG(cond, msg) GF_CHECK_ARG_AS(__func__, cond, msg)
// ... with a formatted message, under the name `fn` of the entry point that was called
#define GF_REFUSE_AS(fn, cond, fmt, ...)                                \
    do {                                                               \
        if (!(cond)) {                                                 \
            gf::set_error("%s: " fmt, fn, ##__VA_ARGS__);              \
            return GF_EINVAL;                                          \
        }                                                              \
    } while (0)
// the kernels move rows as float4s: what every row pointer and parameter must not be (null is aligned)
inline bool misaligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

#define GF_CHECK_LAUNCH_AS(fn)                                                 \
    do {                                                                       \
        hipError_t e_ = hipGetLastError();                                     \
        if (e_ != hipSuccess) {                                                \
            gf::set_error("%s: HIP launch failed: %s", fn, hipGetErrorString(e_)); \
            return GF_ELAUNCH;                                                 \
        }                                                                      \
    } while (0)
#define GF_CHECK_LAUNCH() GF_CHECK_LAUNCH_AS(__func__)

// a caller-allocated region (`what`: "workspace", "scratch") shorter than the op's carve needs
inline int refuse_workspace(const char *fn, const char *what, size_t have, size_t need) { set_error("%s: %s of %zu bytes, %zu needed", fn, what, have, need); return GF_EWORKSPACE; }
#define GF_CHECK_WORKSPACE_AS(fn, what, have, need) do { if ((have) < (need)) return gf::refuse_workspace(fn, what, have, need); } while (0)
#define GF_CHECK_WORKSPACE(have, need) GF_CHECK_WORKSPACE_AS(__func__, "workspace", have, need)

// ---- a splat call on the host (splat_fwd.hip, splat_bwd.hip, splat_bwd_mfma.hip): its sizes and inputs, filled once by the C entry point
struct SplatInputs {
    int per_axis, P, N, H, W, D;
    const float *pts, *means3D, *opacity, *semantics, *cov3D;
    const int *points_int, *means3D_int, *radii;
};
// The backward's gradient of the logits and the four gradients it writes.
struct SplatGrads {
    const float *out_grad;
    float *means_grad, *opa_grad, *sem_grad, *cov_grad;
};

// The argument checks the forward and the backward share, reported under the entry point's name `fn`.
inline int check_splat_shape(const char *fn, int variant, int C, const SplatInputs &in)
{
    GF_CHECK_ARG_AS(fn, variant == GF_SPLAT_BASE || variant == GF_SPLAT_PROB, "unknown variant");
    GF_CHECK_ARG_AS(fn, C == kC, "only 18 semantic channels are supported (NUM_CHANNELS)");
    GF_CHECK_ARG_AS(fn, in.P >= 0 && in.N >= 0, "negative size");
    GF_CHECK_ARG_AS(fn, in.H > 0 && in.W > 0 && in.D > 0 && in.H <= 2047 && in.W <= 2047 && in.D <= 1023, "grid size out of range");
    GF_CHECK_ARG_AS(fn, (long long)in.H * in.W * in.D < (1ll << 31), "grid too large");
    return GF_OK;
}

int cu_count();   // gf_api.hip: compute units of the device current at the first call (cached); 256 if the query fails
// workgroups for `items` work items dealt to the eight XCDs, `per_cu` resident per CU: a multiple of 8, at most one per item slot
inline int xcd_grid(int items, int per_cu)
{
    const int per_xcd = (items + 7) / 8, resident = per_cu * cu_count() / 8, slots = resident > 1 ? resident : 1;
    return 8 * (per_xcd < slots ? per_xcd : slots);
}
// units (double bricks of 4 x 4 x 8 voxels) of the wave-autonomous kernels, forward and backward, for a grid
inline int splat_units(int nsuper, int D) { return nsuper * 4 * ((D + 7) / 8); }
// ... and the workgroups (= waves) that claim them: eight per CU (one 20 KB LDS block and 256 VGPRs each).  The forward's wave kernel and
// the backward's gradient kernel both launch with it, and the forward's records pass arms the backward's per-XCD unit counters with an
// eighth of it (PrepArgs::bwd_counter_init)
inline int splat_unit_grid(int nunits) { return xcd_grid(nunits, 8); }
// ceil(2^32 / d): the launch constants the wave kernels decode a unit with (m_ps: d = units per supertile, m_nsy: d = nsy)
inline uint32_t ceil_recip32(int d) { return (uint32_t)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); }

// The records pass of the forward (gf_splat_prep_kernel: records, packed boxes, supertile bitmask) run for the matrix-core
// backward: no point scans, no range verdicts, natural-log covariance; additionally every Gaussian is given its rows of
// the partial-gradient buffer (record dword 31; splat_bwd_mfma.hip).  Launches one kernel on `stream`.
void launch_prep_for_backward(const SplatInputs &in, const uint32_t *state, const SplatWorkspace &ws, hipStream_t stream);

// The matrix-core backward of the base variant (splat_bwd_mfma.hip): [records pass ->] set-up -> gradient kernel -> row sums.
// records_asserted: 1 = no records pass; every kernel checks the workspace's generation against the state block's instead.
// gate: 0 = unconditional; 1 = stands down unless the forward's state block says a matrix-core body rendered the call;
// 2 = writes NaN gradients in that case.
void launch_splat_backward_mfma(const SplatInputs &in, const SplatGrads &g, const uint32_t *state, const SplatWorkspace &ws, int gate,
                                int records_asserted, hipStream_t stream);

}  // namespace gf
