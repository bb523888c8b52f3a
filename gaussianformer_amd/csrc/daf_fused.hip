// daf_fused.hip -- the deformable aggregation of an INFERENCE frame in one launch (round 6; VERDICT r5 #5, SURVEY.md section 8f N2:
// "the weights could be consumed on the fly"): what DeformableFeatureAggregation.forward does between the weights_fc GEMM and
// output_proj (model/encoder/gaussian_encoder/deformable_module.py:174-233,242) --
//     project_points (:268-285)  ->  mask, all_miss, softmax over (pts, cams, L) per group (:199-214)  ->  DAF.apply
//     (ops/src/deformable_aggregation_cuda.cu:125-187)  ->  features.sum(dim=2) (:242)
// -- without the [A * pts, cams, L, G] weights tensor (88 MB at 25 600 anchors, 498 MB at 144 000: written by gf_daf_prepare,
// read back by gf_daf_forward), without the [A * pts, C] sampled features (118 / 664 MB, written, read back and summed over the
// key points by torch) and, where the attention logits are a sum of an anchor part and a camera part (use_camera_embed:
// weights_fc is linear, so W (f + e + c_cam) + b = [W (f + e) + b] + W c_cam, :253-262), without the [A, cams, L * pts * G] logits
// either (88 MB): the kernel adds the two parts as it reads them.
//
// One wave per anchor, four anchors per workgroup:
//   1. lanes = (key point, camera) pairs: projection, depth clamp, image_wh, visibility; the visible pairs are compacted into a
//      list (ballot + mbcnt) -- one pair in five is visible at the nuScenes rig, and everything below walks the list only;
//   2. lanes = (visible pair, level, group): logits from LDS copies of the anchor's and the cameras' parts, maximum and sum of
//      exp2((x - m) log2 e) per group over the wave (gf_daf_prepare's v_exp_f32 path: the same values);
//   3. four lane groups of sixteen (eight channels per lane, as gf_daf_fwd4_kernel<8>) take the visible pairs round-robin: four
//      levels x four bilinear taps each, all loaded from clamped pixels (no load under a condition), weight = exp2((x - m) log2 e)
//      / sum of the lane's channel group, formed again from the LDS logits (one v_exp_f32 per pair and level: nothing is kept per
//      entry); the four partial rows are added across the lane groups and ONE 512-byte row leaves per anchor.
// Results: the same products as the three-step path, summed in a different order (pairs are dealt to four lane groups and the key
// points are not summed last): equal to ~1e-6 of the row's magnitude, tests/test_daf_fused.py holds them to 1e-5.
#include "gf_daf.hpp"

#ifndef GF_FU_UNROLL
#define GF_FU_UNROLL 1   // levels of a visible pair whose row pieces are in flight together (measured, round 6: 2 -> 126 registers, four waves
                         // per SIMD, 147 us at 25 600 anchors; 1 with the allocation held to six waves -> 78 registers, 130 us; 4 -> 217 us)
#endif
#ifndef GF_FU_MINB
#define GF_FU_MINB 6     // workgroups (of four waves) per CU the register allocation aims for (7: eight spilled registers, 139 us; 8: 167 us)
#endif
#ifndef GF_FU_CPL
#define GF_FU_CPL 8      // channels per lane
#endif

namespace gf {

constexpr int kFuMaxPairs = 256;   // pts * cams per anchor (as gf_daf_prepare)
constexpr int kFuMaxLG = 64;       // L * G entries per pair

__host__ __device__ inline int fu_even(int n) { return n + (n & 1); }

struct DafFusedArgs {
    const float *key_points;   // [B, A, pts, 3]
    const float *proj;         // [B, cams, 4, 4]
    const float *image_wh;     // [B, cams, 2] or null
    const float *raw;          // [B, A, cams, L, pts, G], or null when the two parts below are given
    const float *raw_anchor;   // [B, A, L, pts, G] or null
    const float *raw_cam;      // [B, cams, L, pts, G] or null
    const float *feat;         // [B, cams * num_feat rows, C]: the formatted pyramid (feature_maps_format)
    const int *spatial_shape;  // [L, 2]
    const int *scale_start;    // [L]
    float *out;                // [B, A, C]
    int B, A, pts, cams, L, G, C, num_feat;
    const unsigned char *wmask;   // [B, A, cams, L, pts, G] attention-dropout keep-mask (read by the MASK instantiations only)
};

// one workgroup = 4 waves = 4 consecutive anchors.  MASK: entries the keep-mask drops leave their group's maximum and sum and
// weigh 0; a group with no visible, kept entry gives zero channels (all_miss, deformable_module.py:199-214).  The MASK = false
// instantiation is the code of gf_daf_fused_forward.
template <int CPL, bool MASK = false>   // channels per lane (8: C = 128 in sixteen lanes)
__global__ __launch_bounds__(256, GF_FU_MINB) void gf_daf_fused_kernel(DafFusedArgs a)
{
    extern __shared__ float s_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int npair = a.pts * a.cams, LG = a.L * a.G, LPG = a.L * a.pts * a.G;
    // dynamic LDS: [cams][LPG] camera logits (shared, padded to an even count) | per wave: [LPG] anchor logits, [npair] uv (float2),
    // [npair] list of visible pairs
    float *s_cam = s_dyn;
    const int per_wave = LPG + (LPG & 1) + 3 * npair + (npair & 1);   // (even: the uv pairs are read as float2)
    float *s_mine = s_dyn + (a.raw ? 0 : fu_even(a.cams * LPG)) + wave * per_wave;
    float *s_anc = s_mine;
    float2 *s_uv = reinterpret_cast<float2 *>(s_mine + LPG + (LPG & 1));
    int *s_list = reinterpret_cast<int *>(s_mine + LPG + (LPG & 1) + 2 * npair);
    const long long anchor = (long long)blockIdx.x * 4 + wave;   // b * A + a
    const long long nanchor = (long long)a.B * a.A;
    const int b = (int)(min(anchor, nanchor - 1) / a.A);
    if (!a.raw) {
        // the cameras' logits of this batch element (a workgroup's four anchors share one b unless it straddles two: then per wave
        // below -- rare, so simply: every wave copies its own b's table when the workgroup straddles)
        const int b0 = (int)(((long long)blockIdx.x * 4) / a.A), b3 = (int)(min((long long)blockIdx.x * 4 + 3, nanchor - 1) / a.A);
        if (b0 == b3) {
            for (int i = threadIdx.x; i < a.cams * LPG; i += 256) s_cam[i] = a.raw_cam[(size_t)b0 * a.cams * LPG + i];
            __syncthreads();
        } else {
            __syncthreads();
            s_cam = nullptr;   // (straddling workgroup: read the camera part from memory)
        }
    }
    if (anchor >= nanchor) return;
    const int CV = a.C / CPL;              // lanes per row
    const int sg = lane / CV, cv = lane - sg * CV, nsg = 64 / CV;
    const int c0 = cv * CPL;
    const int grp = c0 / (a.C / a.G);
    // ---- 1. projection (project_points, deformable_module.py:268-285) and the list of visible pairs
    if (!a.raw)
        for (int i = lane; i < LPG; i += 64) s_anc[i] = a.raw_anchor[anchor * LPG + i];
    const int nvis = visible_pairs<false>(a.key_points, anchor, a.proj, a.image_wh, (size_t)b * a.cams, a.pts, a.cams, lane, s_uv, s_list,
                                          nullptr, nullptr);
    wave_lds_handover();
    float acc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) acc[j] = 0.f;
    if (nvis > 0) {
        // ---- 2. softmax over the visible (pair, level) entries per group; entry e = (v * L + l) * G + g, so g = lane % G
        const int E = nvis * LG;
        const FusedLogits<MASK> lg{a.raw, s_anc, s_cam, a.raw_cam + (size_t)b * a.cams * LPG, a.wmask, (size_t)anchor * a.cams * LPG,
                                   a.pts, a.G, LPG};
        // (entries of a lane: e = lane + 64 k.  Where L G divides 64 -- the usual 4 x 4 -- the lane keeps its (level, group) and walks
        // the pairs in steps of 64 / (L G): no division per entry)
        const bool stepped = (64 % LG) == 0;
        const int dv = lane / LG, r0 = lane - dv * LG, l0 = r0 / a.G, g0 = r0 - l0 * a.G, vstep = stepped ? 64 / LG : 0;
        auto logit = [&](int e, int k) -> float {
            if (stepped) {
                const int pc = s_list[dv + k * vstep];
                return lg.kept(pc, l0, g0) ? lg.at(pc, l0, g0) : -INFINITY;
            }
            const int v = e / LG, r = e - v * LG, l = r / a.G;
            return lg.kept(s_list[v], l, r - l * a.G) ? lg.at(s_list[v], l, r - l * a.G) : -INFINITY;
        };
        float m = -INFINITY;
        for (int e = lane, k = 0; e < E; e += 64, ++k) m = fmaxf(m, logit(e, k));
        m = wave_xor_reduce_strided(m, a.G, Max());
        float s = 0.f;
        for (int e = lane, k = 0; e < E; e += 64, ++k) {
            if (MASK) {
                const float x = logit(e, k);   // (a dropped entry is -inf: its group's maximum may be -inf too)
                s += x == -INFINITY ? 0.f : fast_exp(x - m);
            } else {
                s += fast_exp(logit(e, k) - m);
            }
        }
        s = wave_xor_reduce_strided(s, a.G, Sum());
        // (lane % G == g holds group g's maximum and sum; a sampling lane needs those of ITS channel group: lane grp < G has them)
        const float inv_mine = s > 0.f ? 1.f / s : 0.f;
        const float inv = __shfl(inv_mine, grp, 64), mg = __shfl(m, grp, 64);
        // ---- 3. sampling: lane group sg takes the visible pairs sg, sg + nsg, ...
        for (int v = sg; v < nvis; v += nsg) {
            const int pc = s_list[v], cam = pc & 255;
            const float2 uv = s_uv[(pc >> 8) * a.cams + cam];
            const float *fcam = a.feat + ((size_t)b * a.cams + cam) * a.num_feat * a.C + c0;
#pragma unroll GF_FU_UNROLL
            for (int l = 0; l < a.L; ++l) {
                const int h = a.spatial_shape[2 * l], w = a.spatial_shape[2 * l + 1];
                const float h_im = uv.y * h - 0.5f, w_im = uv.x * w - 0.5f;   // deformable_aggregation_cuda.cu:174-175
                // bilinear_sampling, :13-53: four taps from clamped pixels, out-of-image ones contribute exactly 0
                const Taps t = make_taps(h_im, w_im, h, w);
                float v1[CPL], v2[CPL], v3[CPL], v4[CPL];
                load_corners<CPL>(fcam + (size_t)a.scale_start[l] * a.C, a.C, t, h, w, v1, v2, v3, v4);
                const float wt = lg.kept(pc, l, grp) ? fast_exp(lg.at(pc, l, grp) - mg) * inv : 0.f;
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    const float x1 = t.ok1 ? v1[j] : 0.f, x2 = t.ok2 ? v2[j] : 0.f, x3 = t.ok3 ? v3[j] : 0.f, x4 = t.ok4 ? v4[j] : 0.f;
                    acc[j] += (t.w1 * x1 + t.w2 * x2 + t.w3 * x3 + t.w4 * x4) * wt;
                }
            }
        }
    }
    // ---- the lane groups' partial rows -> one row per anchor (wave_xor_reduce_strided's order, all channels in ONE loop over d)
    for (int d = CV; d < 64; d <<= 1)
#pragma unroll
        for (int j = 0; j < CPL; ++j) acc[j] += __shfl_xor(acc[j], d, 64);
    if (sg == 0) {
        float *o = a.out + anchor * a.C + c0;
#pragma unroll
        for (int j = 0; j < CPL; j += 4)
            *reinterpret_cast<float4 *>(o + j) = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
    }
}


// ---------------------------------------------------------------------------------------------------------------------------------
// Backward of the block (training).  For anchor a and group g, with the kept entries e = (key point, camera, level) -- the camera
// sees the pair and the keep-mask keeps the entry --, w_e = exp(x_e - m) / sum and S_e[c] the bilinear sample:
//     gw_e          = sum_{c in g} grad_out[a, c] S_e[c]
//     d logit_e     = w_e (gw_e - sum_e' w_e' gw_e')                  (0 for entries that are not kept and for all-miss groups)
//     d mc_ms_feat += coef_tap w_e grad_out[a, c]                     (deformable_aggregation_cuda.cu:80-110)
//     d (u, v)      = sum_c w_e grad_out[a, c] (W dS/dw_im, H dS/dh_im)  (:92-121), mapped to the key point through the
//                     projection as gf_daf_prepare_backward does it
// One wave per anchor, as the forward: the projection, the visible list and the softmax are formed again from the logits (nothing
// is saved but the inputs), then the lane groups take the visible pairs round-robin and gather the forward's taps.  gw goes to LDS
// per (visible pair, level, group) -- pts * cams * L * G floats per wave at most, which is why a workgroup holds fewer waves where
// that does not fit four times --, the (u, v) gradient per pair to LDS, and the feature gradient leaves as float atomics (no
// [A * pts, C] expanded gradient, no [A * pts, cams, L, G] weights tensor).  The camera part of split logits is a sum over all the
// anchors of a batch element into cams * L * pts * G addresses: each workgroup (per_wg anchors of ONE batch element) adds its
// anchors' parts in LDS and writes one partial row; gf_daf_fused_cam_reduce_kernel sums the rows.
struct DafFusedBwdArgs {
    DafFusedArgs f;
    const float *grad_out;       // [B, A, C]
    float *grad_feat;            // [B, cams * num_feat, C], accumulated, or null
    float *grad_kp;              // [B, A, pts, 3] or null
    float *grad_raw;             // [B, A, cams, L, pts, G] or null (full logits)
    float *grad_raw_anchor;      // [B, A, L, pts, G] or null (split logits)
    float *part_cam;             // [B * nchunk, cams * L * pts * G] per-workgroup sums of d raw_cam, or null
    int per_wg, nchunk;          // anchors per workgroup, workgroups per batch element
};

// floats of LDS per wave: uv, d uv (float2 each), anchor logits, visible list, pair -> list slot, key-point partials, gw
__host__ __device__ inline int fu_bwd_per_wave(int npair, int LG, int LPG) { return fu_even(4 * npair + LPG + 2 * npair + 3 * npair + npair * LG); }

template <int CPL>
__global__ __launch_bounds__(256) void gf_daf_fused_bwd_kernel(DafFusedBwdArgs args)
{
    const DafFusedArgs &a = args.f;
    extern __shared__ float s_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int npair = a.pts * a.cams, LG = a.L * a.G, LPG = a.L * a.pts * a.G, J = a.cams * LPG;
    const int b = blockIdx.x / args.nchunk, chunk = blockIdx.x - b * args.nchunk;
    const bool split = a.raw == nullptr;
    const bool need_gw = args.grad_raw || args.grad_raw_anchor || args.part_cam;
    float *s_cam = s_dyn, *s_gcam = s_dyn + (split ? J : 0);
    float *s_mine = s_dyn + fu_even((split ? J : 0) + (args.part_cam ? J : 0)) + wave * fu_bwd_per_wave(npair, LG, LPG);
    float2 *s_uv = reinterpret_cast<float2 *>(s_mine), *s_guv = s_uv + npair;
    float *s_anc = s_mine + 4 * npair;
    int *s_list = reinterpret_cast<int *>(s_anc + LPG), *s_pidx = s_list + npair;
    float *s_part = reinterpret_cast<float *>(s_pidx + npair), *s_gw = s_part + 3 * npair;
    if (split)
        for (int i = threadIdx.x; i < J; i += blockDim.x) s_cam[i] = a.raw_cam[(size_t)b * J + i];
    if (args.part_cam)
        for (int i = threadIdx.x; i < J; i += blockDim.x) s_gcam[i] = 0.f;
    __syncthreads();
    const int CV = a.C / CPL;
    const int sg = lane / CV, cv = lane - sg * CV, nsg = 64 / CV;
    const int c0 = cv * CPL, grp = c0 / (a.C / a.G), lanes_per_group = (a.C / a.G) / CPL;
    const int a_end = min(a.A, (chunk + 1) * args.per_wg);
    for (int ia = chunk * args.per_wg + wave; ia < a_end; ia += nw) {
        const long long anchor = (long long)b * a.A + ia;
        // ---- 1. projection and the list of visible pairs (as the forward)
        if (split)
            for (int i = lane; i < LPG; i += 64) s_anc[i] = a.raw_anchor[anchor * LPG + i];
        const int nvis = visible_pairs<true>(a.key_points, anchor, a.proj, a.image_wh, (size_t)b * a.cams, a.pts, a.cams, lane, s_uv, s_list,
                                             s_guv, s_pidx);
        wave_lds_handover();
        // (FusedLogits here: 46 -> 47 spilled SGPRs, so this kernel keeps its own view of the logits; profiles/daf_block_pieces.txt)
        auto logit_at = [&](int pc, int l, int g) -> float {
            const int pt = pc >> 8, cam = pc & 255;
            const int o = (l * a.pts + pt) * a.G + g;
            if (!split) return a.raw[(anchor * a.cams + cam) * LPG + o];
            return s_anc[o] + s_cam[cam * LPG + o];
        };
        auto kept = [&](int pc, int l, int g) -> bool {
            return !a.wmask || a.wmask[(anchor * a.cams + (pc & 255)) * LPG + (l * a.pts + (pc >> 8)) * a.G + g] != 0;
        };
        // ---- 2. the softmax's maximum and sum per group (entry e = (v * L + l) * G + g; lane % G == g)
        const int E = nvis * LG;
        auto entry = [&](int e, int &pc, int &l) {
            const int v = e / LG, r = e - v * LG;
            pc = s_list[v];
            l = r / a.G;
        };
        const int gl = lane % a.G;
        float m = -INFINITY;
        for (int e = lane; e < E; e += 64) {
            int pc, l;
            entry(e, pc, l);
            if (kept(pc, l, gl)) m = fmaxf(m, logit_at(pc, l, gl));
        }
        m = wave_xor_reduce_strided(m, a.G, Max());
        float s = 0.f;
        for (int e = lane; e < E; e += 64) {
            int pc, l;
            entry(e, pc, l);
            if (kept(pc, l, gl)) s += fast_exp(logit_at(pc, l, gl) - m);
        }
        s = wave_xor_reduce_strided(s, a.G, Sum());
        const float inv_mine = s > 0.f ? 1.f / s : 0.f;
        const float inv = __shfl(inv_mine, grp, 64), mg = __shfl(m, grp, 64);
        // ---- 3. the forward's taps again: gw, d (u, v), d mc_ms_feat
        float go[CPL];
#pragma unroll
        for (int j = 0; j < CPL; j += 4)
            *reinterpret_cast<float4 *>(go + j) = *reinterpret_cast<const float4 *>(args.grad_out + anchor * a.C + c0 + j);
        for (int v = sg; v < nvis; v += nsg) {
            const int pc = s_list[v], pt = pc >> 8, cam = pc & 255;
            const float2 uv = s_uv[pt * a.cams + cam];
            const size_t row0 = ((size_t)b * a.cams + cam) * a.num_feat;
            const float *fcam = a.feat + row0 * a.C + c0;
            float gu = 0.f, gv = 0.f;
            for (int l = 0; l < a.L; ++l) {
                const int h = a.spatial_shape[2 * l], w = a.spatial_shape[2 * l + 1];
                const float h_im = uv.y * h - 0.5f, w_im = uv.x * w - 0.5f;
                const Taps t = make_taps(h_im, w_im, h, w);
                const Corners c = clamp_corners(t, h, w);   // (load_corners below: 2 223 instructions for 2 222)
                const size_t p1 = (size_t)c.r1 * a.C, p2 = (size_t)c.r2 * a.C, p3 = (size_t)c.r3 * a.C, p4 = (size_t)c.r4 * a.C;
                const float *base = fcam + (size_t)a.scale_start[l] * a.C;
                float v1[CPL], v2[CPL], v3[CPL], v4[CPL];
#pragma unroll
                for (int j = 0; j < CPL; j += 4) {
                    *reinterpret_cast<float4 *>(v1 + j) = *reinterpret_cast<const float4 *>(base + p1 + j);
                    *reinterpret_cast<float4 *>(v2 + j) = *reinterpret_cast<const float4 *>(base + p2 + j);
                    *reinterpret_cast<float4 *>(v3 + j) = *reinterpret_cast<const float4 *>(base + p3 + j);
                    *reinterpret_cast<float4 *>(v4 + j) = *reinterpret_cast<const float4 *>(base + p4 + j);
                }
                const float wt = kept(pc, l, grp) ? fast_exp(logit_at(pc, l, grp) - mg) * inv : 0.f;
                float sv = 0.f, sw = 0.f, sh = 0.f;
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    const float x1 = t.ok1 ? v1[j] : 0.f, x2 = t.ok2 ? v2[j] : 0.f, x3 = t.ok3 ? v3[j] : 0.f, x4 = t.ok4 ? v4[j] : 0.f;
                    sv += go[j] * (t.w1 * x1 + t.w2 * x2 + t.w3 * x3 + t.w4 * x4);
                    sw += go[j] * (t.hh * (x2 - x1) + t.lh * (x4 - x3));   // grad_w_weight, :84-110
                    sh += go[j] * (t.hw * (x3 - x1) + t.lw * (x4 - x2));   // grad_h_weight
                }
                if (need_gw) {
                    // (xor 1 .. ASCENDING, here and for gu, gv below: group_sum adds in descending order -- other last bits)
                    for (int d = 1; d < lanes_per_group; d <<= 1) sv += __shfl_xor(sv, d, 64);
                    if (cv % lanes_per_group == 0) s_gw[v * LG + l * a.G + grp] = sv;
                }
                gu += (float)w * wt * sw;
                gv += (float)h * wt * sh;
                if (args.grad_feat && wt != 0.f) {
                    float *gbase = args.grad_feat + (row0 + a.scale_start[l]) * a.C + c0;
                    const bool ok[4] = {t.ok1, t.ok2, t.ok3, t.ok4};
                    const size_t po[4] = {p1, p2, p3, p4};
                    const float cw[4] = {t.w1 * wt, t.w2 * wt, t.w3 * wt, t.w4 * wt};
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (ok[k])
#pragma unroll
                            for (int j = 0; j < CPL; ++j) unsafeAtomicAdd(gbase + po[k] + j, cw[k] * go[j]);
                }
            }
            if (args.grad_kp) {
                for (int d = 1; d < CV; d <<= 1) {
                    gu += __shfl_xor(gu, d, 64);
                    gv += __shfl_xor(gv, d, 64);
                }
                if (cv == 0) s_guv[pt * a.cams + cam] = make_float2(gu, gv);
            }
        }
        wave_lds_handover();
        // ---- 4. softmax backward: d logit_e = w_e (gw_e - sum_e' w_e' gw_e'), written in the logits' layouts
        if (need_gw) {
            float dot = 0.f;
            for (int e = lane; e < E; e += 64) {
                int pc, l;
                entry(e, pc, l);
                if (kept(pc, l, gl)) dot += fast_exp(logit_at(pc, l, gl) - m) * inv_mine * s_gw[e];
            }
            dot = wave_xor_reduce_strided(dot, a.G, Sum());
            auto dlogit = [&](int pt, int cam, int l) -> float {   // group gl
                const int v = s_pidx[pt * a.cams + cam], pc = (pt << 8) | cam;
                if (v < 0 || !kept(pc, l, gl)) return 0.f;
                return fast_exp(logit_at(pc, l, gl) - m) * inv_mine * (s_gw[v * LG + l * a.G + gl] - dot);
            };
            if (args.grad_raw)   // [cams][L][pts][G], every entry written
                for (int i = lane; i < J; i += 64) {
                    int r = i / a.G;
                    const int pt = r % a.pts;
                    r /= a.pts;
                    const int l = r % a.L, cam = r / a.L;
                    args.grad_raw[anchor * J + i] = dlogit(pt, cam, l);
                }
            if (split && (args.grad_raw_anchor || args.part_cam))   // [L][pts][G]: the anchor part sums the cameras
                for (int i = lane; i < LPG; i += 64) {
                    const int r = i / a.G, pt = r % a.pts, l = r / a.pts;
                    float sum = 0.f;
                    for (int cam = 0; cam < a.cams; ++cam) {
                        const float x = dlogit(pt, cam, l);
                        sum += x;
                        if (args.part_cam && x != 0.f) atomicAdd(s_gcam + cam * LPG + i, x);
                    }
                    if (args.grad_raw_anchor) args.grad_raw_anchor[anchor * LPG + i] = sum;
                }
        }
        // ---- 5. projection backward (gf_daf_prepare_backward's arithmetic), u = x / max(z, 1e-5) / w_img.  (Its text, not a helper
        // shared with gf_daf_prepare_bwd_kernel: 7 instructions and a 47th spilled SGPR here, other FMA contractions there.)
        if (args.grad_kp) {
            for (int q = lane; q < npair; q += 64) {
                const int pt = q / a.cams, cam = q - pt * a.cams;
                const float *kp = a.key_points + (anchor * a.pts + pt) * 3;
                const float *M = a.proj + ((size_t)b * a.cams + cam) * 16;
                const Proj p = project(M, kp[0], kp[1], kp[2]);
                const float zc = fmaxf(p.z, 1e-5f), iz = 1.f / zc;
                const float2 g2 = s_guv[q];
                float gu = g2.x, gv = g2.y;
                if (a.image_wh) {
                    gu /= a.image_wh[((size_t)b * a.cams + cam) * 2];
                    gv /= a.image_wh[((size_t)b * a.cams + cam) * 2 + 1];
                }
                const float cz = p.z > 1e-5f ? -(gu * p.x + gv * p.y) * iz * iz : 0.f;
                const float cx = gu * iz, cy = gv * iz;
                s_part[3 * q] = cx * M[0] + cy * M[4] + cz * M[8];
                s_part[3 * q + 1] = cx * M[1] + cy * M[5] + cz * M[9];
                s_part[3 * q + 2] = cx * M[2] + cy * M[6] + cz * M[10];
            }
            wave_lds_handover();
            for (int pt = lane; pt < a.pts; pt += 64) {
                float gx = 0.f, gy = 0.f, gz = 0.f;
                for (int cam = 0; cam < a.cams; ++cam) {
                    const float *c = s_part + 3 * (pt * a.cams + cam);
                    gx += c[0]; gy += c[1]; gz += c[2];
                }
                float *o = args.grad_kp + (anchor * a.pts + pt) * 3;
                o[0] = gx; o[1] = gy; o[2] = gz;
            }
        }
        wave_lds_handover();   // the wave's LDS is reused by its next anchor
    }
    if (args.part_cam) {
        __syncthreads();
        for (int i = threadIdx.x; i < J; i += blockDim.x) args.part_cam[(size_t)blockIdx.x * J + i] = s_gcam[i];
    }
}

// d raw_cam[b, i] = sum over the batch element's workgroup rows.  64 entries x 4 row subsets per workgroup, gridDim.z slices of the
// rows; the slices meet with one float atomic each (out is zeroed first).
__global__ __launch_bounds__(256) void gf_daf_fused_cam_reduce_kernel(const float *part, float *out, int J, int nchunk)
{
    __shared__ float s_red[4][64];
    const int t = threadIdx.x & 63, sub = threadIdx.x >> 6, b = blockIdx.y;
    const int i = blockIdx.x * 64 + t;
    float s = 0.f;
    if (i < J)
        for (int c = blockIdx.z * 4 + sub; c < nchunk; c += 4 * gridDim.z) s += part[((size_t)b * nchunk + c) * J + i];
    s_red[sub][t] = s;
    __syncthreads();
    if (sub == 0 && i < J) unsafeAtomicAdd(out + (size_t)b * J + i, s_red[0][t] + s_red[1][t] + s_red[2][t] + s_red[3][t]);
}

// the launch geometry of the backward: waves per workgroup (4, or fewer where four waves' LDS does not fit), anchors per workgroup
struct FuBwdGeom {
    int nw, per_wg, nchunk;
    size_t lds;
};
static FuBwdGeom fu_bwd_geom(int A, int pts, int cams, int L, int G, bool split, bool cam_part)
{
    const int npair = pts * cams, LG = L * G, LPG = L * pts * G, J = cams * LPG;
    FuBwdGeom g;
    const size_t shared = (size_t)fu_even((split ? J : 0) + (cam_part ? J : 0)), per = (size_t)fu_bwd_per_wave(npair, LG, LPG);
    g.nw = 4;
    while (g.nw > 1 && sizeof(float) * (shared + g.nw * per) > 160 * 1024) g.nw >>= 1;
    g.lds = sizeof(float) * (shared + g.nw * per);
    g.per_wg = 4 * g.nw;   // (each wave takes four anchors: a quarter of the partial rows of one anchor per wave)
    g.nchunk = (A + g.per_wg - 1) / g.per_wg;
    return g;
}

static int fu_check(int B, int A, int pts, int cams, int L, int G, int C, int num_feat)
{
    GF_CHECK_ARG(B >= 0 && A >= 0 && pts > 0 && cams > 0 && L > 0 && G > 0 && C > 0 && num_feat > 0, "bad size");
    GF_CHECK_ARG((G & (G - 1)) == 0 && G <= 64, "G must be a power of two <= 64");
    GF_CHECK_ARG(pts * cams <= kFuMaxPairs, "pts * cams too large");
    GF_CHECK_ARG(L * G <= kFuMaxLG, "L * G too large");
    GF_CHECK_ARG(C % 8 == 0 && C % G == 0 && (C / G) % 8 == 0 && 64 % (C / 8) == 0 && C / 8 >= G,
                 "channels: C a multiple of 8 G with C / 8 lanes dividing a wave");
    return GF_OK;
}

static int fu_forward(int B, int A, int pts, int cams, int L, int G, int C, int num_feat, const float *key_points,
                      const float *projection_mat, const float *image_wh, const float *raw_weights, const float *raw_anchor,
                      const float *raw_cam, const unsigned char *weight_mask, const float *mc_ms_feat, const int *spatial_shape,
                      const int *scale_start_index, float *out, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = fu_check(B, A, pts, cams, L, G, C, num_feat)) return rc;
    if ((long long)B * A == 0) return GF_OK;
    GF_CHECK_ARG(key_points && projection_mat && mc_ms_feat && spatial_shape && scale_start_index && out, "null pointer");
    GF_CHECK_ARG((raw_weights != nullptr) != (raw_anchor != nullptr && raw_cam != nullptr) && ((raw_anchor != nullptr) == (raw_cam != nullptr)),
                 "give raw_weights, or raw_anchor and raw_cam");
    GF_CHECK_ARG((((uintptr_t)mc_ms_feat | (uintptr_t)out) & 15) == 0, "features and output must be 16-byte aligned");
    DafFusedArgs a;
    a.key_points = key_points; a.proj = projection_mat; a.image_wh = image_wh; a.raw = raw_weights; a.raw_anchor = raw_anchor;
    a.raw_cam = raw_cam; a.feat = mc_ms_feat; a.spatial_shape = spatial_shape; a.scale_start = scale_start_index; a.out = out;
    a.B = B; a.A = A; a.pts = pts; a.cams = cams; a.L = L; a.G = G; a.C = C; a.num_feat = num_feat; a.wmask = weight_mask;
    const int npair = pts * cams, LPG = L * pts * G;
    const size_t lds = sizeof(float) * ((raw_weights ? 0 : (size_t)fu_even(cams * LPG)) + 4 * ((size_t)LPG + (LPG & 1) + 3 * npair + (npair & 1)));
    GF_CHECK_ARG(lds <= 160 * 1024, "shape needs more LDS than a CU has");
    const long long nanchor = (long long)B * A;
    const void *kernel = weight_mask ? reinterpret_cast<const void *>(gf_daf_fused_kernel<GF_FU_CPL, true>)
                                     : reinterpret_cast<const void *>(gf_daf_fused_kernel<GF_FU_CPL, false>);
    if (lds > 64 * 1024 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();   // (not left for the next launch check to find)
        set_error("%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu) failed", __func__, lds);
        return GF_ELAUNCH;
    }
    if (weight_mask)
        hipLaunchKernelGGL((gf_daf_fused_kernel<GF_FU_CPL, true>), dim3((unsigned)((nanchor + 3) / 4)), dim3(256), lds, stream, a);
    else
        hipLaunchKernelGGL((gf_daf_fused_kernel<GF_FU_CPL, false>), dim3((unsigned)((nanchor + 3) / 4)), dim3(256), lds, stream, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

}  // namespace gf

extern "C" int gf_daf_fused_forward(int B, int A, int pts, int cams, int L, int G, int C, int num_feat, const float *key_points,
                                    const float *projection_mat, const float *image_wh, const float *raw_weights,
                                    const float *raw_anchor, const float *raw_cam, const float *mc_ms_feat, const int *spatial_shape,
                                    const int *scale_start_index, float *out, void *stream_)
{
    return gf::fu_forward(B, A, pts, cams, L, G, C, num_feat, key_points, projection_mat, image_wh, raw_weights, raw_anchor, raw_cam,
                          nullptr, mc_ms_feat, spatial_shape, scale_start_index, out, stream_);
}

extern "C" int gf_daf_fused_forward_masked(int B, int A, int pts, int cams, int L, int G, int C, int num_feat, const float *key_points,
                                           const float *projection_mat, const float *image_wh, const float *raw_weights,
                                           const float *raw_anchor, const float *raw_cam, const unsigned char *weight_mask,
                                           const float *mc_ms_feat, const int *spatial_shape, const int *scale_start_index, float *out,
                                           void *stream_)
{
    return gf::fu_forward(B, A, pts, cams, L, G, C, num_feat, key_points, projection_mat, image_wh, raw_weights, raw_anchor, raw_cam,
                          weight_mask, mc_ms_feat, spatial_shape, scale_start_index, out, stream_);
}

extern "C" size_t gf_daf_fused_backward_workspace_bytes(int B, int A, int pts, int cams, int L, int G)
{
    using namespace gf;
    if (B < 0 || A < 0 || pts <= 0 || cams <= 0 || L <= 0 || G <= 0 || pts * cams > kFuMaxPairs || L * G > kFuMaxLG) return 0;
    const FuBwdGeom g = fu_bwd_geom(A, pts, cams, L, G, true, true);
    return sizeof(float) * (size_t)B * g.nchunk * cams * L * pts * G;
}

extern "C" int gf_daf_fused_backward(int B, int A, int pts, int cams, int L, int G, int C, int num_feat, const float *key_points,
                                     const float *projection_mat, const float *image_wh, const float *raw_weights,
                                     const float *raw_anchor, const float *raw_cam, const unsigned char *weight_mask,
                                     const float *mc_ms_feat, const int *spatial_shape, const int *scale_start_index,
                                     const float *grad_out, float *grad_mc_ms_feat, float *grad_key_points, float *grad_raw_weights,
                                     float *grad_raw_anchor, float *grad_raw_cam, void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace gf;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = fu_check(B, A, pts, cams, L, G, C, num_feat)) return rc;
    GF_CHECK_ARG((raw_weights != nullptr) != (raw_anchor != nullptr && raw_cam != nullptr) && ((raw_anchor != nullptr) == (raw_cam != nullptr)),
                 "give raw_weights, or raw_anchor and raw_cam");
    const bool split = raw_weights == nullptr;
    GF_CHECK_ARG(!grad_raw_weights || !split, "grad_raw_weights needs raw_weights");
    GF_CHECK_ARG(!(grad_raw_anchor || grad_raw_cam) || split, "grad_raw_anchor / grad_raw_cam need raw_anchor and raw_cam");
    if ((long long)B * A == 0) return GF_OK;
    GF_CHECK_ARG(key_points && projection_mat && mc_ms_feat && spatial_shape && scale_start_index && grad_out, "null pointer");
    GF_CHECK_ARG((((uintptr_t)mc_ms_feat | (uintptr_t)grad_out) & 15) == 0, "features and grad_out must be 16-byte aligned");
    const FuBwdGeom g = fu_bwd_geom(A, pts, cams, L, G, split, grad_raw_cam != nullptr);
    GF_CHECK_ARG(g.lds <= 160 * 1024, "shape needs more LDS than a CU has");
    const size_t J = (size_t)cams * L * pts * G;
    GF_CHECK_ARG(!grad_raw_cam || (workspace && workspace_bytes >= sizeof(float) * (size_t)B * g.nchunk * J),
                 "workspace too small: see gf_daf_fused_backward_workspace_bytes");
    GF_CHECK_ARG((long long)B * g.nchunk < (1ll << 31), "problem too large");
    if (!(grad_mc_ms_feat || grad_key_points || grad_raw_weights || grad_raw_anchor || grad_raw_cam)) return GF_OK;
    DafFusedBwdArgs a{};
    DafFusedArgs &f = a.f;
    f.key_points = key_points; f.proj = projection_mat; f.image_wh = image_wh; f.raw = raw_weights; f.raw_anchor = raw_anchor;
    f.raw_cam = raw_cam; f.feat = mc_ms_feat; f.spatial_shape = spatial_shape; f.scale_start = scale_start_index; f.out = nullptr;
    f.B = B; f.A = A; f.pts = pts; f.cams = cams; f.L = L; f.G = G; f.C = C; f.num_feat = num_feat; f.wmask = weight_mask;
    a.grad_out = grad_out; a.grad_feat = grad_mc_ms_feat; a.grad_kp = grad_key_points; a.grad_raw = grad_raw_weights;
    a.grad_raw_anchor = grad_raw_anchor; a.part_cam = grad_raw_cam ? static_cast<float *>(workspace) : nullptr;
    a.per_wg = g.per_wg; a.nchunk = g.nchunk;
    if (g.lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(gf_daf_fused_bwd_kernel<GF_FU_CPL>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)g.lds) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu) failed", __func__, g.lds);
        return GF_ELAUNCH;
    }
    hipLaunchKernelGGL(gf_daf_fused_bwd_kernel<GF_FU_CPL>, dim3((unsigned)(B * g.nchunk)), dim3(64 * g.nw), g.lds, stream, a);
    GF_CHECK_LAUNCH();
    if (grad_raw_cam) {
        if (hipMemsetAsync(grad_raw_cam, 0, sizeof(float) * B * J, stream) != hipSuccess) {
            set_error("%s: hipMemsetAsync failed", __func__);
            return GF_ELAUNCH;
        }
        const int slices = std::min(32, (g.nchunk + 3) / 4);
        hipLaunchKernelGGL(gf_daf_fused_cam_reduce_kernel, dim3((unsigned)((J + 63) / 64), (unsigned)B, (unsigned)slices), dim3(256), 0,
                           stream, a.part_cam, grad_raw_cam, (int)J, g.nchunk);
        GF_CHECK_LAUNCH();
    }
    return GF_OK;
}
