// The encoder's Gaussian refinement step: what SparseGaussian3DRefinementModule.forward (version 1,
// model/encoder/gaussian_encoder/refine_module.py:72-123) and SparseGaussian3DRefinementModuleV2.forward (version 2,
// refine_module_v2.py:62-107) compute after their MLP, in one launch forward and one backward.
//
// The reference strings 30-40 slices, stacks, cats, clamps, sigmoids and logs over an [n, D] tensor; autograd doubles that.
// Here one wave takes 64 consecutive rows.  A row is 4 D bytes (112 at D = 28), so a lane reading its own row from memory
// would touch 64 cache lines per instruction; instead the 64 rows -- contiguous in memory -- cross between memory and an
// LDS tile as one run of dwords (a wave instruction moves 256 contiguous bytes), and each lane reads its row from the tile.
// The tile's row pitch is odd, so the 64 lanes of a column read hit 64 different banks.  (An LDS-DMA load lands lane-linear
// and cannot write a padded pitch, so the tile is filled through registers.)  Every output leaves the same way: the lane
// writes its row into a tile, the wave stores the tile as one run.
//
// Arithmetic: fp32, unfused (contract(off)) and in the reference's operation order, with ocml's expf / logf / log1pf -- the
// inverse sigmoid of version 2 amplifies a rounding of its argument by up to 1e4 near its clamp, so this op stays within the
// error of torch's own fp32 evaluation rather than a v_exp_f32's 1e-6.  The backward recomputes the forward's values from
// (output, anchor) with the same code, so it needs no forward result.  That code -- a row's forward values, the forward tail on
// them, the tile moves -- is gf_refine.hpp's, shared with refine_mlp.hip (the MLP and this tail in one launch).
//
// HBM traffic per row, forward: 4 (2 D + Da + 10 + opa + S [+ 6]) bytes.
#include "gf_refine.hpp"

namespace gf {

// torch.clamp's gradient mask: bounds included
__device__ __forceinline__ bool passes(float x, float lo, float hi) { return x >= lo && x <= hi; }

template <int VERSION, bool BACKWARD>
__global__ __launch_bounds__(64) void gf_refine_kernel(RefineArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ float lds[];
    const int po = a.po, pa = a.pa, pn = a.pn;
    float *t_o = lds;                  // output rows; forward: becomes anchor_out, backward: grad_output
    float *t_a = t_o + 64 * po;        // anchor columns < C; backward: becomes grad_anchor
    float *t_n = t_a + 64 * pa;        // the narrow outputs, or their gradients
    float *t_g = t_n + 64 * pn;        // backward: grad of anchor_out
    const int base = blockIdx.x * 64, rows = min(64, a.n - base), lane = lane_id();
    const int opa = (a.flags & GF_REFINE_OPACITY) ? 1 : 0, sem0 = 10 + opa;
    const bool sig = !(a.flags & GF_REFINE_XYZ_IDENTITY), restrict_xyz = (a.flags & GF_REFINE_RESTRICT_XYZ) != 0;
    const bool softmax = (a.flags & GF_REFINE_SEM_SOFTMAX) != 0, softplus = (a.flags & GF_REFINE_SEM_SOFTPLUS) != 0;

    const size_t b = base;
    tile_load(a.output, b, a.D, t_o, po, 0, a.D, rows);
    tile_load(a.anchor, b, a.Da, t_a, pa, 0, a.C, rows);
    if (BACKWARD) {
        tile_load(a.g_anchor_out, b, a.D, t_g, po, 0, a.D, rows);
        tile_load(a.g_means, b, 3, t_n, pn, kNMeans, 3, rows);
        tile_load(a.g_scales, b, 3, t_n, pn, kNScales, 3, rows);
        tile_load(a.g_rotations, b, 4, t_n, pn, kNRot, 4, rows);
        tile_load(a.g_opacities, b, opa, t_n, pn, kNOpa, opa, rows);
        tile_load(a.g_semantics, b, a.S, t_n, pn, kNSem, a.S, rows);
        if (VERSION == 2) {
            tile_load(a.g_original, b, 3, t_n, pn, kNOrig, 3, rows);
            tile_load(a.g_delta, b, 3, t_n, pn, kNDelta, 3, rows);
        }
    }
    __syncthreads();

    if (lane < rows) {
        float *ro = t_o + lane * po, *ra = t_a + lane * pa, *rn = t_n + lane * pn;
        if (!BACKWARD) {
            refine_row_forward<VERSION>(a, ro, ra, rn);
        } else {
            // ---- the forward's values, recomputed by the forward's code
            RefineRow v;
            refine_row_values<VERSION>(a, ro, ra, v);
            const float (&o)[10] = v.o, (&av)[10] = v.av, (&x)[10] = v.x, (&s0)[3] = v.s0, (&xyz)[3] = v.xyz, (&c0)[3] = v.c0;
            const float (&u)[3] = v.u, (&t)[3] = v.t, (&act)[3] = v.act, (&ssc)[3] = v.ssc, (&qv)[4] = v.qv;
            const float norm = v.norm, sopa = v.sopa;
            // ---- gradients, in autograd's order: the heads of the prediction first, then anchor_out's own gradient joins
            float gx[10];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float dact = sig ? safe_sigmoid_grad(xyz[i], act[i])
                                       : (VERSION == 2 && !passes(xyz[i], kUnitLo, kUnitHi) ? 0.f : 1.f);
                gx[i] = t_g[lane * po + i] + rn[kNMeans + i] * a.span[i] * dact;
                gx[3 + i] = t_g[lane * po + 3 + i] + rn[kNScales + i] * a.scale_span * safe_sigmoid_grad(x[3 + i], ssc[i]);
            }
            float gq[4], dot = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                gq[j] = t_g[lane * po + 6 + j] + rn[kNRot + j];
                dot += gq[j] * qv[j];
            }
            // x / max(||x||, eps): below eps the divisor is a constant
#pragma unroll
            for (int j = 0; j < 4; ++j) gx[6 + j] = (norm >= kNormEps ? gq[j] - qv[j] * dot : gq[j]) * v.inv_norm;
            // columns from 10 on: the tile's own row takes the gradient (and the anchor's tile where it was added)
            if (opa) {
                const float g = t_g[lane * po + 10] + rn[kNOpa] * safe_sigmoid_grad(ro[10], sopa);
                ro[10] = g;
                if (10 < a.C) ra[10] = g;
            }
            if (softmax) {
                float m = -INFINITY, sum = 0.f, gy = 0.f;
                for (int j = 0; j < a.S; ++j) m = fmaxf(m, ro[sem0 + j]);
                for (int j = 0; j < a.S; ++j) {
                    const float e = expf(ro[sem0 + j] - m);
                    ro[sem0 + j] = e;
                    sum += e;
                }
                for (int j = 0; j < a.S; ++j) {
                    ro[sem0 + j] = ro[sem0 + j] / sum;
                    gy += rn[kNSem + j] * ro[sem0 + j];
                }
                for (int j = 0; j < a.S; ++j) {
                    const float g = t_g[lane * po + sem0 + j] + ro[sem0 + j] * (rn[kNSem + j] - gy);
                    ro[sem0 + j] = g;
                    if (sem0 + j < a.C) ra[sem0 + j] = g;
                }
            } else {
                for (int j = 0; j < a.S; ++j) {
                    const float sv = ro[sem0 + j];
                    float g = rn[kNSem + j];
                    if (softplus && !(sv > 20.f)) {
                        const float z = expf(sv);
                        g = g * z / (z + 1.f);
                    }
                    g += t_g[lane * po + sem0 + j];
                    ro[sem0 + j] = g;
                    if (sem0 + j < a.C) ra[sem0 + j] = g;
                }
            }
            if (VERSION == 1) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (!sig && !passes(x[i], kUnitLo, kUnitHi)) gx[i] = 0.f;
                }
#pragma unroll
                for (int k = 0; k < 10; ++k) {
                    if (k < a.C) ra[k] = gx[k];
                    ro[k] = (k < 3 && restrict_xyz) ? gx[k] * a.unit[k] * 2.f * safe_sigmoid_grad(o[k], s0[k]) : gx[k];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    float gu;   // through reverse_cartesian: the clamp, then log(t / (1 - t))
                    if (sig) gu = passes(u[i], kLogitLo, kLogitHi) ? gx[i] / (t[i] * (1.f - t[i])) : 0.f;
                    else gu = passes(u[i], kUnitLo, kUnitHi) ? gx[i] : 0.f;
                    const float gm = gu / a.span[i];
                    const float g_delta = gm + rn[kNDelta + i], g_orig = gm + rn[kNOrig + i];
                    ro[i] = g_delta * a.unit[i] * 2.f * safe_sigmoid_grad(o[i], s0[i]);
                    ra[i] = g_orig * a.span[i] * (sig ? safe_sigmoid_grad(av[i], c0[i]) : (passes(av[i], kUnitLo, kUnitHi) ? 1.f : 0.f));
                }
#pragma unroll
                for (int k = 3; k < 10; ++k) ro[k] = gx[k];
            }
        }
    }
    __syncthreads();

    if (!BACKWARD) {
        refine_store_forward<VERSION>(a, b, t_o, t_n, rows);
    } else {
        tile_store(a.grad_output, b, t_o, po, 0, a.D, a.D, rows);
        tile_store(a.grad_anchor, b, t_a, pa, 0, a.Da, a.C, rows);
    }
}

static size_t lds_bytes(const RefineArgs &a, bool backward) { return (size_t)64 * 4 * (a.po * (backward ? 2 : 1) + a.pa + a.pn); }

int refine_launch_backward(const char *who, const RefineArgs &a, int version, hipStream_t stream)
{
    const dim3 grid((a.n + 63) / 64), block(64);
    if (version == 1) hipLaunchKernelGGL((gf_refine_kernel<1, true>), grid, block, lds_bytes(a, true), stream, a);
    else hipLaunchKernelGGL((gf_refine_kernel<2, true>), grid, block, lds_bytes(a, true), stream, a);
    GF_CHECK_LAUNCH_AS(who);
    return GF_OK;
}

}  // namespace gf

extern "C" int gf_refine_forward(int n, int D, int Da, int version, int flags, int R, int S, const double *consts, const float *output,
                                 const float *anchor, float *anchor_out, float *means, float *scales, float *rotations,
                                 float *opacities, float *semantics, float *original_means, float *delta_means, void *stream_)
{
    using namespace gf;
    RefineArgs a{};
    if (int rc = refine_fill_args(a, __func__, n, D, Da, version, flags, R, S, consts)) return rc;
    if (n == 0) return GF_OK;
    GF_CHECK_ARG(output && (anchor || a.C == 0) &&
                     refine_forward_outputs_present(version, flags, S, anchor_out, means, scales, rotations, opacities, semantics, original_means, delta_means),
                 "null pointer");
    a.output = output; a.anchor = anchor; a.anchor_out = anchor_out; a.means = means; a.scales = scales; a.rotations = rotations;
    a.opacities = opacities; a.semantics = semantics; a.original_means = original_means; a.delta_means = delta_means;
    const dim3 grid((n + 63) / 64), block(64);
    if (version == 1) hipLaunchKernelGGL((gf_refine_kernel<1, false>), grid, block, lds_bytes(a, false), (hipStream_t)stream_, a);
    else hipLaunchKernelGGL((gf_refine_kernel<2, false>), grid, block, lds_bytes(a, false), (hipStream_t)stream_, a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_refine_backward(int n, int D, int Da, int version, int flags, int R, int S, const double *consts, const float *output,
                                  const float *anchor, const float *grad_anchor_out, const float *grad_means, const float *grad_scales,
                                  const float *grad_rotations, const float *grad_opacities, const float *grad_semantics,
                                  const float *grad_original_means, const float *grad_delta_means, float *grad_output,
                                  float *grad_anchor, void *stream_)
{
    using namespace gf;
    RefineArgs a{};
    if (int rc = refine_fill_args(a, __func__, n, D, Da, version, flags, R, S, consts)) return rc;
    if (n == 0) return GF_OK;
    GF_CHECK_ARG(output && (anchor || a.C == 0) && grad_output && (grad_anchor || Da == 0), "null pointer");
    a.output = output; a.anchor = anchor;
    a.g_anchor_out = grad_anchor_out; a.g_means = grad_means; a.g_scales = grad_scales; a.g_rotations = grad_rotations;
    a.g_opacities = grad_opacities; a.g_semantics = grad_semantics; a.g_original = grad_original_means; a.g_delta = grad_delta_means;
    a.grad_output = grad_output; a.grad_anchor = grad_anchor;
    return refine_launch_backward(__func__, a, version, (hipStream_t)stream_);
}
