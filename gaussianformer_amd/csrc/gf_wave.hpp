// gf_wave.hpp -- lane, wave (wave64) and workgroup primitives shared by every kernel of libgf_hip.so (gfx950 only).
// Each helper says which lanes must be active, where its result is valid and, for floating point, the order of summation:
// that order is part of the bits of a result, so forms that differ in it stay apart under names that say how.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gf {

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }

// number of set bits of `mask` below this lane
__device__ __forceinline__ int mbcnt(unsigned long long mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                          __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// This wave's LDS writes before the call are visible to its own lanes after it: a workgroup-scope fence (the writes are
// complete, and the compiler moves no LDS access across it) and a wave barrier (a scheduling point for the wave's lanes, no
// instruction).  Where one wave owns a piece of LDS it stands in for __syncthreads(); it does NOT order other waves.
__device__ __forceinline__ void wave_lds_handover()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// ---- DPP running sums: all 64 lanes active (bound_ctrl gives an inactive or out-of-row source 0) ----------------------------
// v + v of the lane that CTRL selects, in the rows of ROW_MASK
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_add(float v)
{
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, true));
}

// Sums over aligned groups of N lanes, valid in the LAST lane of each group; order: prefix by row_shr 1, 2, 4[, 8], the two rows
// of a half joined by row_bcast 15.  (Deformable aggregation, nuScenes layout: 8 lanes per channel group, 32 per point.)
__device__ __forceinline__ float sum4_last(float v)  // valid in lanes with (lane & 3) == 3
{
    v = dpp_add<0x111>(v);  // row_shr:1
    return dpp_add<0x112>(v);  // row_shr:2
}
__device__ __forceinline__ float sum8_last(float v)  // valid in lanes with (lane & 7) == 7
{
    return dpp_add<0x114>(sum4_last(v));  // row_shr:4
}
__device__ __forceinline__ float sum16_last(float v)  // valid in lanes with (lane & 15) == 15 (a DPP row)
{
    return dpp_add<0x118>(sum8_last(v));  // row_shr:8
}
__device__ __forceinline__ float sum32_last(float v)  // valid in lanes 31 and 63
{
    return dpp_add<0x142, 0xa>(sum16_last(v));  // row_bcast:15 into rows 1 and 3
}

// Sum over the wave, the same bits in every lane (lane 63's total through v_readlane).  Order: prefix by row_shr 1, 2, 4, 8,
// rows joined by row_bcast 15, 31.
__device__ __forceinline__ float wave_sum(float v)
{
    v = dpp_add<0x143, 0xc>(sum32_last(v));  // row_bcast:31 into rows 2 and 3
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// Inclusive prefix sum over the wave, valid in every lane: six DPP adds (row_shr 1, 2, 4, 8, row_bcast 15, 31).  The splat
// kernels' scan (forward, both backwards); unsigned callers cast.
__device__ __forceinline__ int wave_incl_scan_dpp(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, true);
    return v;
}

// Reduction of a 32-bit value over the wave, uniform: DPP inside each row of 16 (quad_perm, row_half_mirror, row_mirror), then
// op(op(row 0, row 1), op(row 2, row 3)).  All 64 lanes active.  Floats go through as bits with MaxF / MinF.  (FPS.)
template <class Op>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t v, Op op)
{
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));  // row_mirror
    const uint32_t r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const uint32_t r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    return op(op(r0, r1), op(r2, r3));
}
struct MaxU { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
struct MinU { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; } };
struct MaxF { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return __float_as_uint(fmaxf(__uint_as_float(a), __uint_as_float(b))); } };
struct MinF { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return __float_as_uint(fminf(__uint_as_float(a), __uint_as_float(b))); } };

// ---- shuffle forms (ds_bpermute): the lanes read from must be active ---------------------------------------------------------
struct Sum { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct Max { __device__ float operator()(float a, float b) const { return fmaxf(a, b); } };

// Butterfly over the wave, xor 32 .. 1, unrolled: every lane ends with the same bits (each step combines the same two values in
// either order).  (Lifter: softmax maximum and sums with Max / Sum, the fp64 loss partial.)
template <typename T, typename Op>
__device__ __forceinline__ T wave_xor_reduce(T v, Op op)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}
// The same sum over aligned groups of `width` lanes (a run-time power of two <= 64), xor width / 2 .. 1; valid in every lane of
// the group.  A loop: an unroll request on a run-time trip count cannot be met and warns, so it stays a function of its own.
// (Deformable aggregation's backward away from the DPP layouts: lanes per channel group / per point.)
__device__ __forceinline__ float group_sum(float v, int width)
{
    for (int d = width >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// Butterfly over the lanes that share lane % G (G a power of two), xor G .. 32 ASCENDING; the same bits in each of them.
// (Deformable aggregation's weights: softmax over the lanes of one channel group.)
template <typename Op>
__device__ __forceinline__ float wave_xor_reduce_strided(float v, int G, Op op)
{
    for (int d = G; d < 64; d <<= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}

// (value, index) with the larger value; equal values -> the lower index.  Butterfly, xor 32 .. 1: every lane ends with the pair.
__device__ __forceinline__ void wave_argmax(float &v, int &i)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(i, d, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// fp64 sum over the wave, valid in LANE 0 only: tree by __shfl_down 32 .. 1 (occupancy loss; not the butterfly's order)
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// Inclusive prefix sum over the wave, valid in every lane: steps d = 1, 2, 4 .. 32, each adding the running sum of the lane d
// below (__shfl_up) -- a fixed order, so the lifter's float cdf is reproducible.  Occupancy loss (int) and lifter (int, float)
// use this form; it is other instructions than wave_incl_scan_dpp and stays apart from it.
template <typename T>
__device__ __forceinline__ T wave_incl_scan_shfl(T v)
{
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// ---- workgroup forms: every thread of the workgroup calls (they hold __syncthreads) -------------------------------------------
// exclusive scan over a workgroup of WAVES waves (wave_incl_scan_shfl inside each); `lds` holds WAVES ints; `total` gets the sum
template <int WAVES>
__device__ __forceinline__ int block_excl_scan(int v, int *lds, int &total)
{
    const int w = threadIdx.x >> 6, incl = wave_incl_scan_shfl(v);
    if (lane_id() == 63) lds[w] = incl;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        const int t = lds[i];
        off += i < w ? t : 0;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return off + incl - v;
}

// sum of 256 doubles, one per thread of a 256-thread workgroup, returned to every thread: LDS tree, halves folded 128 .. 1
// (lds[t] += lds[t + s]) -- a fixed order, which the occupancy loss's bitwise reproducibility rests on.  `lds` holds 256 doubles;
// __syncthreads before it is written again (every thread reads lds[0] on the way out)
__device__ __forceinline__ double block_sum256(double v, double *lds)
{
    lds[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    return lds[0];
}

// ---- LDS-DMA: memory -> LDS without passing registers (M0 = the wave's LDS base; lane i lands at base + i * size) ------------
// Issued from inline asm.  hipcc's waitcnt pass treats a global_load_lds it can see as a pending write to ALL of LDS and puts a
// full `s_waitcnt vmcnt(0)` in front of the next LDS access -- in the wave-autonomous kernel that drained the record request of
// group k + 1 before group k's S' rows were read, and the prefetched bitmask row before the epilogue's staging writes: the very
// round trips those requests were issued early to hide (found in the ISA, round 5).  Issued from asm the request is invisible
// to that pass, and every wait for it is an explicit `s_waitcnt vmcnt(N)` in the source.  The compiler's own vmcnt waits stay
// safe: they count outstanding operations, which only makes them wait longer when these requests are in flight.
// `g` is per lane, `l` wave-uniform; the splat kernels pass address-space pointers (gptr, lptr), deformable aggregation generic ones.
template <typename G, typename L>
__device__ __forceinline__ void lds_dma16(G g, L l)
{
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"((uint32_t)(uintptr_t)l) : "memory", "m0");
}
template <typename G, typename L>
__device__ __forceinline__ void lds_dma4(G g, L l)
{
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(g), "s"((uint32_t)(uintptr_t)l) : "memory", "m0");
}

}  // namespace gf
