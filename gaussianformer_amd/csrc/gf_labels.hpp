// gf_labels.hpp -- the head's per-row label rule (model/head/gaussian_head.py:164-185), one copy for the kernels that form labels
// from the [N,18] logits: gf_head_labels (head_labels.hip) writes them, the metric's counting pass (miou.hip) only counts them.
#pragma once
#include "gf_common.hpp"

namespace gf {

constexpr int kLabelRowsLds = 64 * kC;   // floats of LDS a wave needs for its 64 rows

// Stages the wave's `rows` (<= 64) rows, which start at `blk`, in its own piece of LDS `mine` (16-byte aligned): coalesced 16-byte
// pieces where `vec_ok` (the logits' base is 16-byte aligned; 64 rows are 4608 bytes, so every wave's first row then is), and hands
// the piece over to the wave's lanes.  All 64 lanes call it.
__device__ __forceinline__ void stage_label_rows(const float *blk, int rows, bool vec_ok, int lane, float *mine)
{
    const int nflt = rows * kC;
    if (vec_ok && rows == 64) {
        // the usual case: the wave's five 16-byte pieces per lane (4.5 on average) requested together, then written to LDS --
        // as a load-store loop every piece was a round trip of its own
        float4 v[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = *reinterpret_cast<const float4 *>(blk + min(4 * lane + 256 * k, 64 * kC - 4));
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (4 * lane + 256 * k < 64 * kC) *reinterpret_cast<float4 *>(mine + 4 * lane + 256 * k) = v[k];
    } else {
        for (int e0 = 4 * lane; e0 < nflt; e0 += 256) {
            if (vec_ok && e0 + 3 < nflt) {
                *reinterpret_cast<float4 *>(mine + e0) = *reinterpret_cast<const float4 *>(blk + e0);
            } else {
                for (int j = 0; j < 4 && e0 + j < nflt; ++j) mine[e0 + j] = blk[e0 + j];
            }
        }
    }
    wave_lds_handover();
}

// The label of one staged row: `bin` is the row's bin_logit (prob modes), `mode` a GF_LABELS_* value.
__device__ __forceinline__ int row_label(const float *row, float bin, int mode, float threshold, int empty_label)
{
    float best = 0.f;
    int arg = 0;
#pragma unroll
    for (int c = 0; c < kC; ++c) {
        float v = row[c];
        if (mode == 2) v = c < kC - 1 ? v * bin : 1 - bin;  // geosem (:166-168)
        if (c == 0 || v > best) {  // first maximal value wins, like torch.argmax
            best = v;
            arg = c;
        }
    }
    if (mode == 1 && !(bin > threshold)) arg = empty_label;  // :179-183
    return arg;
}

}  // namespace gf
