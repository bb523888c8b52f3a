// splat_mfma.hpp -- what the two persistent matrix-core forward kernels of splat_fwd.hip (gf_splat_render_mfma_kernel, one tile per
// workgroup, and gf_splat_render_mfma_wave_kernel, one double brick per wave) do alike per group of 32 Gaussians: the exponent +
// accumulate of a block pair -- and the tile kernel's record request (the wave kernel fetches each record once, four pieces per
// half-lane, and keeps that request and its slot layout to itself).  gfx950 only, device only, plain functions; each says which
// lanes must be active, what LDS it touches and which waits and fences it leaves to the caller.  The kernels are held to bit-identity with each other
// (test_mfma_wave_and_tile_kernels_agree_bit_for_bit, test_list_builder_regimes_agree_across_kernels_and_with_the_oracle), so forms
// that differ stay in the kernels: the tile kernel forms `tb` with selects, zeroes a dead lane's opacity and theta, takes theta's
// three f16 terms from split3 and splits S' with fmaf behind the fp32 transpose (it runs at 252 VGPRs: its operand phase is left
// alone); the wave kernel uses packed 16-bit operations for `tb`, leaves a dead lane's opacity and theta as its record gives them
// (its `tb` row alone makes the weights +0), forms theta's terms two per conversion (v_cvt_pk_f16_f32, v_fma_mix_f32) and splits S'
// BEFORE the transpose, which is a transposing 16-bit LDS read of two [Gaussian][channel] f16 images.  The matrix-core backward
// (splat_bwd_mfma.hip) takes the H8 union from here and nothing else: its group arithmetic has other operand roles and its
// requests are compiler-visible __builtin_amdgcn_global_load_lds on purpose.  The unit decode, the two list builders, the box test
// with its queue push and the theta operands are the same text in the wave kernel and the backward and are NOT here: each was moved
// into a function and each changed the compiled wave kernel (profiles/splat_mfma_pieces.txt).
#pragma once
#include "gf_common.hpp"

namespace gf {

union H8 {   // an MFMA A / B fragment, by vector, packed pair, element or dword
    h8 v;
    fp16x2 p[4];
    _Float16 e[8];
    uint32_t u[4];
};

// ---- record request ------------------------------------------------------------------------------------------------------------
// The tile kernel's record request: six 16-byte pieces per lane of the record at `rec` into the six 1 KB planes of the wave's slot
// `dst` by LDS-DMA -- mean / opacity, covariance, covariance + box, and the three semantics pieces at byte offsets o3, o4, o5 of the
// record (the channels its half-lane stages).  All 64 lanes active.  Issued from inline asm: nothing
// waits here, the caller's `s_waitcnt vmcnt` does, and the slot must be free (a wave fence behind its last reads) before the call.
// (The backward fetches other pieces and a seventh, and issues them as compiler-visible builtins on purpose: it stays there.)
__device__ __forceinline__ void request_record_pieces(const char *rec, char *dst, int o3, int o4, int o5)
{
    lds_dma16((gptr)(rec), (lptr)(dst));
    lds_dma16((gptr)(rec + 16), (lptr)(dst + 1024));
    lds_dma16((gptr)(rec + 32), (lptr)(dst + 2048));
    lds_dma16((gptr)(rec + o3), (lptr)(dst + 3072));
    lds_dma16((gptr)(rec + o4), (lptr)(dst + 4096));
    lds_dma16((gptr)(rec + o5), (lptr)(dst + 5120));
}

// ---- forward: exponent + accumulate of a pair of 32-voxel blocks ---------------------------------------------------------------
// w = exp2(d) of the 16 exponents a lane holds, split into f16 hi + lo: B operands of the accumulation (wh[kh], wl[kh]: K half kh).
// All 64 lanes active (the values feed MFMAs); registers only; no waits or fences.
__device__ __forceinline__ void exp_split_weights(const f32x16 &d, H8 (&wh)[2], H8 (&wl)[2])
{
#pragma unroll
    for (int q = 0; q < 16; q += 2) {
        const float w0 = __builtin_amdgcn_exp2f(d[q]), w1 = __builtin_amdgcn_exp2f(d[q + 1]);
        const fp16x2 hi = __builtin_amdgcn_cvt_pkrtz(w0, w1);
        float q0, q1;  // exact residuals w - hi, the f16 halves read in place (v_fma_mix_f32)
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(q0) : "v"(hi), "v"(w0));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(q1) : "v"(hi), "v"(w1));
        wh[q >> 3].p[(q & 7) >> 1] = hi;
        wl[q >> 3].p[(q & 7) >> 1] = __builtin_amdgcn_cvt_pkrtz(q0, q1);
    }
}
// Two blocks at a time: exponents of the pair (eight MFMAs, two independent chains alternate: theta's three terms against phi, the
// box term tb against the one-hot coordinates), exp + split of each (VALU), accumulation of the pair (twelve MFMAs; per K half
// the matrix products S'_lo W_hi, S'_hi W_lo, S'_hi W_hi, in that order) -- which drains in the matrix pipe under the next pair's
// VALU work, the last one under the next group's operand preparation.  All 64 lanes active; registers only; no waits or fences.
// Priorities (s_setprio) and the inline-asm operand pins stay with the callers, around the call.
__device__ __forceinline__ void exp_accumulate_pair(const H8 &t1, const H8 &t2, const H8 &t3, const H8 &tb, h8 phi0, h8 phi1, h8 hot0,
                                                    h8 hot1, const H8 (&sh)[2], const H8 (&sl)[2], f32x16 &acc0, f32x16 &acc1)
{
    f32x16 d0, d1;
#pragma unroll
    for (int q = 0; q < 16; ++q) { d0[q] = 0.f; d1[q] = 0.f; }
    d0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(t3.v, phi0, d0, 0, 0, 0);
    d1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(t3.v, phi1, d1, 0, 0, 0);
    d0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(t2.v, phi0, d0, 0, 0, 0);
    d1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(t2.v, phi1, d1, 0, 0, 0);
    d0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(t1.v, phi0, d0, 0, 0, 0);
    d1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(t1.v, phi1, d1, 0, 0, 0);
    d0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(tb.v, hot0, d0, 0, 0, 0);
    d1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(tb.v, hot1, d1, 0, 0, 0);
    H8 wh[2][2], wl[2][2];
    exp_split_weights(d0, wh[0], wl[0]);
    exp_split_weights(d1, wh[1], wl[1]);
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(sl[kh].v, wh[0][kh].v, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(sl[kh].v, wh[1][kh].v, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(sh[kh].v, wl[0][kh].v, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(sh[kh].v, wl[1][kh].v, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(sh[kh].v, wh[0][kh].v, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(sh[kh].v, wh[1][kh].v, acc1, 0, 0, 0);
    }
}

}  // namespace gf
