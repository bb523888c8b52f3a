// The prob head's geosem step (model/head/gaussian_head.py:166-168) for training and inference --
//   sem = logits[:, :-1] * bin[:, None];  geo = 1 - bin[:, None];  geosem = cat([sem, geo], -1)
// The reference runs it as three torch launches with two [N,17] / [N,18] intermediates, and autograd's backward as a zero-fill,
// two products and a strided sum.  Here each way is one pass: a wave stages its 64 rows (4608 contiguous bytes) in LDS with
// coalesced 16-byte pieces (stage_label_rows), then works in two shapes on the same staged floats -- FLAT for what is
// elementwise (the wave's 288 float4s go out as they came in, each element scaled by its row's bin), and ROW PER LANE for what
// needs a whole row (the forward's label, the backward's sum over the 17 products).  Every output element is one correctly
// rounded fp32 operation (a product or a difference: nothing for the compiler to contract), so the rows equal the torch
// expression's bit for bit; the backward's sum runs in ascending c in one lane, no atomics: it repeats bit for bit.
#include "gf_labels.hpp"

namespace gf {

constexpr int kGeoPieces = (64 * kC + 255) / 256;   // 16-byte pieces per lane that cover a wave's 64 rows: 5 (4.5 on average)

struct GeosemArgs {
    const float *logits;      // [N,18]
    const float *bin_logits;  // [N]
    const float *grad_out;    // [N,18] (backward)
    float *out;               // [N,18] forward: geosem; backward: grad_logits
    float *grad_bin;          // [N] (backward)
    long long *labels;        // [N] or null (forward)
    long long N;
};

// One staged element `x` of flat index `e` (row e / 18, channel e % 18) scaled for the output: x * bin[row] for c < 17, `last`
// for c == 17 (forward: 1 - bin[row]; backward: +0).
template <bool kBackward> __device__ __forceinline__ float geosem_element(float x, int e, const float *bins)
{
    const int r = e / kC, c = e - r * kC;
    const float b = bins[r];
    return c < kC - 1 ? x * b : (kBackward ? 0.f : 1.f - b);
}

// The flat half: the wave's staged floats `src` (LDS) to `dst` (global, the wave's first row), 16 bytes at a time where `vec_ok`.
template <bool kBackward> __device__ __forceinline__ void geosem_store_flat(const float *src, const float *bins, int rows, bool vec_ok, int lane, float *dst)
{
    const int nflt = rows * kC;
#pragma unroll
    for (int k = 0; k < kGeoPieces; ++k) {
        const int e0 = 4 * lane + 256 * k;
        if (e0 >= nflt) break;   // (rows * 18 is even, e0 a multiple of 4: a piece has 2 or 4 elements of the wave's)
        if (e0 + 3 < nflt) {
            const float4 x = *reinterpret_cast<const float4 *>(src + e0);
            float4 y;
            y.x = geosem_element<kBackward>(x.x, e0, bins);
            y.y = geosem_element<kBackward>(x.y, e0 + 1, bins);
            y.z = geosem_element<kBackward>(x.z, e0 + 2, bins);
            y.w = geosem_element<kBackward>(x.w, e0 + 3, bins);
            if (vec_ok) {
                *reinterpret_cast<float4 *>(dst + e0) = y;
            } else {
                dst[e0] = y.x; dst[e0 + 1] = y.y; dst[e0 + 2] = y.z; dst[e0 + 3] = y.w;
            }
        } else {
            for (int j = 0; e0 + j < nflt; ++j) dst[e0 + j] = geosem_element<kBackward>(src[e0 + j], e0 + j, bins);
        }
    }
}

template <bool kBackward> __global__ __launch_bounds__(256) void gf_head_geosem_kernel(GeosemArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_rows[4][kLabelRowsLds];
    __shared__ __attribute__((aligned(16))) float s_logits[kBackward ? 4 : 1][kBackward ? kLabelRowsLds : 4];   // backward: the logits' rows
    __shared__ float s_bins[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n0 = ((long long)blockIdx.x * 4 + wave) * 64;  // first row of this wave
    if (n0 >= a.N) return;
    const int rows = (int)min((long long)64, a.N - n0);
    float *mine = s_rows[wave], *bins = s_bins[wave];
    // (an unconditional, clamped load: a conditional one would put its wait inside the branch)
    const float bin = a.bin_logits[n0 + min(lane, rows - 1)];
    bins[lane] = bin;
    if (!kBackward) {
        stage_label_rows(a.logits + n0 * kC, rows, ((uintptr_t)a.logits & 15) == 0, lane, mine);   // (its handover covers `bins` too)
        geosem_store_flat<false>(mine, bins, rows, ((uintptr_t)a.out & 15) == 0, lane, a.out + n0 * kC);
        if (a.labels && lane < rows) a.labels[n0 + lane] = row_label(mine + lane * kC, bin, GF_LABELS_PROB_GEOSEM, 0.f, 0);
    } else {
        float *lg = s_logits[wave];
        stage_label_rows(a.grad_out + n0 * kC, rows, ((uintptr_t)a.grad_out & 15) == 0, lane, mine);
        stage_label_rows(a.logits + n0 * kC, rows, ((uintptr_t)a.logits & 15) == 0, lane, lg);
        geosem_store_flat<true>(mine, bins, rows, ((uintptr_t)a.out & 15) == 0, lane, a.out + n0 * kC);
        if (lane < rows) {
            const float *g = mine + lane * kC, *l = lg + lane * kC;
            float acc = g[0] * l[0];
#pragma unroll
            for (int c = 1; c < kC - 1; ++c) acc = __builtin_fmaf(g[c], l[c], acc);   // ascending c, one rounding per term
            a.grad_bin[n0 + lane] = acc - g[kC - 1];
        }
    }
}

// The checks both entry points share, under the name `fn` of the one that was called; `blocks` = workgroups of four waves.
static int check_geosem(const char *fn, long long N, int C, long long *blocks)
{
    GF_CHECK_ARG_AS(fn, C == kC, "only 18 channels are supported (17 semantic classes and the empty one)");
    GF_CHECK_ARG_AS(fn, N >= 0, "bad size");
    *blocks = (N + 255) / 256;
    GF_CHECK_ARG_AS(fn, *blocks < (1ll << 31), "problem too large");
    return GF_OK;
}

}  // namespace gf

extern "C" int gf_head_geosem_forward(long long N, int C, const float *logits, const float *bin_logits, float *out,
                                      long long *labels, void *stream_)
{
    using namespace gf;
    long long blocks = 0;
    if (int rc = check_geosem(__func__, N, C, &blocks)) return rc;
    if (N == 0) return GF_OK;
    GF_CHECK_ARG(logits && bin_logits && out, "null pointer");
    GeosemArgs a{};
    a.logits = logits; a.bin_logits = bin_logits; a.out = out; a.labels = labels; a.N = N;
    hipLaunchKernelGGL(gf_head_geosem_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_head_geosem_backward(long long N, int C, const float *logits, const float *bin_logits, const float *grad_out,
                                       float *grad_logits, float *grad_bin, void *stream_)
{
    using namespace gf;
    long long blocks = 0;
    if (int rc = check_geosem(__func__, N, C, &blocks)) return rc;
    if (N == 0) return GF_OK;
    GF_CHECK_ARG(logits && bin_logits && grad_out && grad_logits && grad_bin, "null pointer");
    GeosemArgs a{};
    a.logits = logits; a.bin_logits = bin_logits; a.grad_out = grad_out; a.out = grad_logits; a.grad_bin = grad_bin; a.N = N;
    hipLaunchKernelGGL(gf_head_geosem_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
