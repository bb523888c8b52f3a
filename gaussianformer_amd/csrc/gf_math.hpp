// gf_math.hpp -- operand types and small numeric helpers shared by the kernels of libgf_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gf {

// ---- vector types: packed VALU pairs and MFMA fragments -------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));     // v_pk_*_f32 operand
typedef float f32x16 __attribute__((ext_vector_type(16)));   // C / D fragment of a 32x32 MFMA
typedef _Float16 h8 __attribute__((ext_vector_type(8)));     // A / B fragment of v_mfma_f32_32x32x16_f16 (splat kernels)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));  // ... the same type under the sparse convolution's name
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));   // A / B fragment of v_mfma_f32_32x32x16_bf16
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));   // result of v_cvt_pkrtz_f16_f32

// ---- address spaces ----------------------------------------------------------------------------------------------------------
using gptr = const __attribute__((address_space(1))) void *;   // global memory, read: the source of an LDS-DMA
using lptr = __attribute__((address_space(3))) void *;         // LDS: its destination
// read-only floats through the constant address space: a wave-uniform fetch becomes a scalar (SMEM) load straight into SGPRs,
// no VGPRs spent on it (the splat kernels' records, Gaussian parameters and lattice)
using cfloat_t = const float __attribute__((address_space(4))) *;
// non-temporal 16-byte store of four floats at a 4-byte aligned global address: (nt4 *)((gfloat *)base + i); the global address
// space keeps the stores global_store (not flat)
typedef __attribute__((address_space(1))) float gfloat;
typedef float nt4v __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((address_space(1))) nt4v nt4;
// write-through 16-byte store (`sc1`) of four floats at a wave-uniform base + a 32-bit per-lane byte offset + the constant IMM: the
// line leaves the XCD's L2 with the store instead of staying there, dirty, until the kernel's end drains it (plain and nt stores
// keep it).  Issued from inline asm, so hipcc does not count it: the asm `s_waitcnt vmcnt(N)` around such stores
// count them by hand (`s_nop 1`: the data registers may be rewritten before a 16-byte store has read them).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) char gchar;
template <int IMM>
__device__ __forceinline__ void store16_wt(gchar *sbase, uint32_t voff, f32x4 v)
{
    asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 sc1\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(sbase), "i"(IMM) : "memory");
}

// three f16 terms of an fp64 value (33 bits): the value as a (hi, lo) pair of floats, then exact fp32 residuals
__device__ __forceinline__ void split3(double t, _Float16 &a, _Float16 &b, _Float16 &c)
{
    float hi = (float)t;
    asm volatile("" : "+v"(hi));  // keeps (half)(float)double from becoming a software double -> half conversion
    const float lo = (float)(t - (double)hi);
    a = (_Float16)hi;
    float r = (hi - (float)a) + lo;
    asm volatile("" : "+v"(r));
    b = (_Float16)r;
    c = (_Float16)(r - (float)b);
}

// exp(x) as v_exp_f32 on x log2(e): relative error <= 1e-6 for |x| < 16
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

// ---- safe_sigmoid (model/utils/safe_ops.py:7-9): clamp to +-9.21, then 1 / (1 + exp(-x)) with ocml's expf (key points, refine)
constexpr float kSigmoidClamp = 9.21f;
__device__ __forceinline__ float safe_sigmoid(float x)
{
    x = fminf(fmaxf(x, -kSigmoidClamp), kSigmoidClamp);
    return 1.f / (1.f + expf(-x));
}
// d safe_sigmoid / dx given its value s (torch.clamp passes the gradient on [min, max], bounds included)
__device__ __forceinline__ float safe_sigmoid_grad(float x, float s)
{
    return (x >= -kSigmoidClamp && x <= kSigmoidClamp) ? s * (1.f - s) : 0.f;
}

// ---- unit quaternion (w, x, y, z) = F.normalize(q, dim=-1) = q / max(||q||, 1e-12) (model/utils/utils.py:23) ------------------
struct UnitQuat {
    float w, x, y, z, inv_norm, norm;   // norm = ||q|| before the clamp
};
__device__ __forceinline__ UnitQuat unit_quat(float q0, float q1, float q2, float q3)
{
    const float n = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    UnitQuat r;
    r.norm = n;
    r.inv_norm = 1.f / fmaxf(n, 1e-12f);
    r.w = q0 * r.inv_norm; r.x = q1 * r.inv_norm; r.y = q2 * r.inv_norm; r.z = q3 * r.inv_norm;
    return r;
}
// the two loaders: four scalar loads at any alignment (key points: a slice of an anchor row) ...
__device__ __forceinline__ UnitQuat unit_quat(const float *q) { return unit_quat(q[0], q[1], q[2], q[3]); }
// ... and one 16-byte load of a 16-byte aligned quaternion (Gaussian prepare: rows of a [P, 4] tensor)
__device__ __forceinline__ UnitQuat unit_quat_aligned16(const float *q)
{
    const float4 v = *reinterpret_cast<const float4 *>(q);
    return unit_quat(v.x, v.y, v.z, v.w);
}
// get_rotation_matrix (model/utils/utils.py:24-69): mat1 @ mat2^T without the first row and column
__device__ __forceinline__ void rotation_of(const UnitQuat &q, float (&R)[3][3])
{
    const float w = q.w, x = q.x, y = q.y, z = q.z;
    R[0][0] = w * w + x * x - y * y - z * z; R[0][1] = 2.f * (x * y - w * z); R[0][2] = 2.f * (x * z + w * y);
    R[1][0] = 2.f * (x * y + w * z); R[1][1] = w * w - x * x + y * y - z * z; R[1][2] = 2.f * (y * z - w * x);
    R[2][0] = 2.f * (x * z - w * y); R[2][1] = 2.f * (y * z + w * x); R[2][2] = w * w - x * x - y * y + z * z;
}

}  // namespace gf
