// gf_daf.hpp -- the pieces the deformable-aggregation sources (daf.hip, daf_prepare.hip, daf_fused.hip) share: the bilinear cell of
// a tap, the projection of a key point into a camera with its visibility gate, the list of an anchor's visible pairs, the fused
// forward's view of the logits.  Each says which reference lines it restates, which lanes must be active and its order of operations.
#pragma once
#include "gf_common.hpp"

namespace gf {

// ---- VEC consecutive channels of a lane as one load / store (per lane, no other lane involved) --------------------------------
template <int VEC>
struct VecT;
struct alignas(16) Float8 { float4 lo, hi; };
template <>
struct VecT<8> { using type = Float8; };
template <>
struct VecT<4> { using type = float4; };
template <>
struct VecT<2> { using type = float2; };
template <>
struct VecT<1> { using type = float; };

template <int VEC>
__device__ __forceinline__ void vload(const float *p, float (&v)[VEC])
{
    using T = typename VecT<VEC>::type;
    const T t = *reinterpret_cast<const T *>(p);
    const float *f = reinterpret_cast<const float *>(&t);
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = f[j];
}

template <int VEC>
__device__ __forceinline__ void vstore(float *p, const float (&v)[VEC])
{
    using T = typename VecT<VEC>::type;
    T t;
    float *f = reinterpret_cast<float *>(&t);
#pragma unroll
    for (int j = 0; j < VEC; ++j) f[j] = v[j];
    *reinterpret_cast<T *>(p) = t;
}

// ---- the bilinear cell (per lane) ------------------------------------------------------------------------------------------------
// The bilinear cell of a tap position (bilinear_sampling, deformable_aggregation_cuda.cu:13-29,51): its low pixel, the
// fractions and the four coefficients; of corner k (0 .. 3: k >> 1 the row step, k & 1 the column step) coefficient and pixel.
struct Cell {
    int h_low, w_low;
    float w1, w2, w3, w4, lh, lw, hh, hw;
    __device__ __forceinline__ float coef(int k) const { return k == 0 ? w1 : k == 1 ? w2 : k == 2 ? w3 : w4; }
    __device__ __forceinline__ int py(int k) const { return h_low + (k >> 1); }
    __device__ __forceinline__ int px(int k) const { return w_low + (k & 1); }
};
__device__ __forceinline__ Cell make_cell(float h_im, float w_im)
{
    Cell t;
    t.h_low = (int)floorf(h_im);
    t.w_low = (int)floorf(w_im);
    t.lh = h_im - t.h_low;
    t.lw = w_im - t.w_low;
    t.hh = 1 - t.lh;
    t.hw = 1 - t.lw;
    t.w1 = t.hh * t.hw; t.w2 = t.hh * t.lw; t.w3 = t.lh * t.hw; t.w4 = t.lh * t.lw;
    return t;
}

// ... and which of the corners lie in the image
struct Taps : Cell {
    bool ok1, ok2, ok3, ok4;
};
__device__ __forceinline__ Taps make_taps(float h_im, float w_im, int height, int width)
{
    Taps t;
    static_cast<Cell &>(t) = make_cell(h_im, w_im);
    const int h_high = t.h_low + 1, w_high = t.w_low + 1;
    t.ok1 = t.h_low >= 0 && t.w_low >= 0;
    t.ok2 = t.h_low >= 0 && w_high <= width - 1;
    t.ok3 = h_high <= height - 1 && t.w_low >= 0;
    t.ok4 = h_high <= height - 1 && w_high <= width - 1;
    return t;
}

// pixel rows (h * width + w) of the four taps with out-of-image coordinates clamped to the nearest
// valid pixel; such taps carry a zero coefficient (ok1..ok4 false), their value is never used
struct Corners {
    int r1, r2, r3, r4;
};
__device__ __forceinline__ Corners clamp_corners(const Taps &t, int height, int width)
{
    const int h0 = max(t.h_low, 0), h1 = min(t.h_low + 1, height - 1);
    const int w0 = max(t.w_low, 0), w1 = min(t.w_low + 1, width - 1);
    return {h0 * width + w0, h0 * width + w1, h1 * width + w0, h1 * width + w1};
}

// The four corner values of a level (base = its first pixel row, this lane's channels).  All four taps are loaded
// unconditionally from clamped (always valid) pixels and the out-of-image ones are replaced by zero BY THE CALLER: a load under
// `if (ok)` is followed by its own s_waitcnt inside the branch, which made the sixteen taps of a camera a serial chain.  (The
// zeroing stays with the callers' arithmetic: moved in here, the selects come before the forward's sums in another order and
// the compiler contracts a different product of val = w1 x1 + .. + w4 x4 into the FMAs -- other last bits, and not the same
// ones in the three forward kernels.)
template <int VEC>
__device__ __forceinline__ void load_corners(const float *base, int C, const Taps &t, int height, int width,
                                             float (&v1)[VEC], float (&v2)[VEC], float (&v3)[VEC], float (&v4)[VEC])
{
    const Corners c = clamp_corners(t, height, width);
    vload<VEC>(base + (size_t)c.r1 * C, v1);
    vload<VEC>(base + (size_t)c.r2 * C, v2);
    vload<VEC>(base + (size_t)c.r3 * C, v3);
    vload<VEC>(base + (size_t)c.r4 * C, v4);
}

// ---- projection (per lane) -------------------------------------------------------------------------------------------------------
// The first three rows of M (4 x 4, row-major) applied to (X, Y, Z, 1); each row summed left to right, the translation last
// (project_points, deformable_module.py:268-277: the matmul).
struct Proj { float x, y, z; };
__device__ __forceinline__ Proj project(const float *M, float X, float Y, float Z)
{
    Proj p;
    p.x = M[0] * X + M[1] * Y + M[2] * Z + M[3];
    p.y = M[4] * X + M[5] * Y + M[6] * Z + M[7];
    p.z = M[8] * X + M[9] * Y + M[10] * Z + M[11];
    return p;
}

// One (key point, camera) pair (project_points, :268-285, and the visibility mask of :199-203): p = M (X, Y, Z, 1),
// zc = max(p.z, 1e-5) (torch.clamp(points_2d[..., 2:3], min=1e-5)), u = p.x / zc, then / the image's width where image_wh is
// given (v alike with the height) -- two divisions in that order, never one by a product; visible = p.z > 1e-5 and 0 < u, v < 1.
// kp = the key point's three floats, bc = b * cams + cam: the camera's matrix is proj + 16 bc, its image size image_wh + 2 bc.
// (The BACKWARD of this chain stays written out in gf_daf_prepare_bwd_kernel and in step 5 of gf_daf_fused_bwd_kernel: as one
// helper it had other products contracted into the FMAs of the first and other resources in the second)
struct PairProj { float u, v; bool vis; };
__device__ __forceinline__ PairProj project_pair(const float *kp, const float *proj, const float *image_wh, size_t bc)
{
    const Proj p = project(proj + bc * 16, kp[0], kp[1], kp[2]);
    const float zc = fmaxf(p.z, 1e-5f);
    PairProj r;
    r.u = p.x / zc;
    r.v = p.y / zc;
    if (image_wh) {
        r.u /= image_wh[bc * 2];
        r.v /= image_wh[bc * 2 + 1];
    }
    r.vis = (p.z > 1e-5f) && (r.u > 0) && (r.u < 1) && (r.v > 0) && (r.v < 1);
    return r;
}

// ---- the fused kernels' visible pairs (all 64 lanes of the wave active: ballot) -----------------------------------------------
// Projects the anchor's pts * cams pairs (pair q = pt * cams + cam, lanes = pairs, 64 per pass), leaves (u, v) of EVERY pair in
// s_uv[q] and compacts the visible ones, in pair order, into s_list as (pt << 8) | cam (pts * cams <= 256); returns their
// number.  BWD: also clears the pair's d (u, v) in s_guv[q] and notes its place in s_list, or -1, in s_pidx[q] (the forward
// passes null for both).  key_points [B, A, pts, 3], anchor = b * A + a, bc0 = b * cams.  The caller's wave_lds_handover() comes
// before any lane reads what this wrote.
template <bool BWD>
__device__ __forceinline__ int visible_pairs(const float *key_points, long long anchor, const float *proj, const float *image_wh, size_t bc0,
                                             int pts, int cams, int lane, float2 *s_uv, int *s_list, float2 *s_guv, int *s_pidx)
{
    const int npair = pts * cams;
    int nvis = 0;
    for (int q0 = 0; q0 < npair; q0 += 64) {
        const int q = q0 + lane;
        bool vis = false;
        if (q < npair) {
            const int pt = q / cams, cam = q - pt * cams;
            const PairProj r = project_pair(key_points + (anchor * pts + pt) * 3, proj, image_wh, bc0 + cam);
            vis = r.vis;
            s_uv[q] = make_float2(r.u, r.v);
            if (BWD) s_guv[q] = make_float2(0.f, 0.f);
        }
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(vis);
        const int pos = nvis + mbcnt(bal);
        if (BWD && q < npair) s_pidx[q] = vis ? pos : -1;
        if (vis) s_list[pos] = ((q / cams) << 8) | (q % cams);
        nvis += __builtin_popcountll(bal);
    }
    return nvis;
}

// ---- the fused forward's attention logits of one anchor (per lane) -------------------------------------------------------------
// Entry (pc = (pt << 8) | cam, level l, group g) lies at o = (l * pts + pt) * G + g of its camera's LPG = L * pts * G floats: the
// weights_fc layout [cams][L][pts][G] (deformable_module.py:243-262).  Full logits: raw [B, A, cams, LPG], block = the anchor's
// offset in it (a 32-bit index on top: cams * LPG <= 2^14).  Split logits (raw null): anchor part + camera part, added in that
// order as they are read; anc[LPG] is the wave's LDS copy, the camera part the workgroup's LDS table cam_lds[cams][LPG] or, where
// that is null (a workgroup that straddles two batch elements), cam_mem, the batch element's block in memory.  MASK: wmask (layout
// and block of raw) drops the entries whose byte is 0; without it wmask is not looked at.  (gf_daf_fused_bwd_kernel keeps its own
// two lambdas: with this struct it spilled a 47th SGPR)
template <bool MASK>
struct FusedLogits {
    const float *raw, *anc, *cam_lds, *cam_mem;
    const unsigned char *wmask;
    size_t block;
    int pts, G, LPG;
    __device__ __forceinline__ int offset(int pc, int l, int g) const { return (l * pts + (pc >> 8)) * G + g; }
    __device__ __forceinline__ float at(int pc, int l, int g) const
    {
        const int cam = pc & 255, o = offset(pc, l, g);
        if (raw) return raw[block + (cam * LPG + o)];
        return anc[o] + (cam_lds ? cam_lds[cam * LPG + o] : cam_mem[cam * LPG + o]);
    }
    __device__ __forceinline__ bool kept(int pc, int l, int g) const { return !MASK || wmask[block + ((pc & 255) * LPG + offset(pc, l, g))] != 0; }
};

}  // namespace gf
