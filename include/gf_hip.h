/*
 * gf_hip.h -- C ABI of libgf_hip.so: the MI355X (gfx950) implementation of
 * GaussianFormer's hot path.  Plain pointers and sizes only; every pointer is a DEVICE
 * pointer unless stated otherwise; `stream` is a hipStream_t passed as void* (NULL = the
 * null stream).  All entry points return 0 on success or a negative GF_E* code;
 * gf_last_error() gives a thread-local message.  No entry point synchronises the host
 * with the device or allocates device memory: scratch comes from the caller-provided
 * workspace (size it with gf_splat_workspace_bytes()).
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * huang-yh/GaussianFormer tree); INTEGRATION.md shows the binding a maintainer adds on the
 * reference side.
 */
#ifndef GF_HIP_H_INCLUDED
#define GF_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF_ABI_VERSION 10   /* 10: gf_refine_forward / gf_refine_backward, and gf_anchor_embed_forward, gf_ffn_*, gf_refine_mlp_*, gf_deform_logits_forward / gf_deform_output_forward, gf_deform_output_train_sizes / gf_deform_output_forward_train / gf_deform_output_backward, gf_miou_workspace_size / gf_miou_step / gf_miou_step_logits, gf_subm_conv_apply_epilogue, gf_head_geosem_forward / gf_head_geosem_backward (added without a bump: a library without them fails to load, the binding resolves every symbol); 9: gf_dcn_workspace_bytes / gf_dcn_forward / gf_dcn_backward; 8: gf_lift_workspace_bytes / gf_lift_pixels, gf_pixel_loss_workspace_bytes / gf_pixel_loss_forward / gf_pixel_loss_backward; 7: gf_occ_loss_workspace_bytes / gf_occ_loss_forward / gf_occ_loss_backward; 6: gf_daf_fused_forward_masked / gf_daf_fused_backward_workspace_bytes / gf_daf_fused_backward; 5: gf_fps_workspace_bytes / gf_farthest_point_sampling, option "fps.exhaustive"; 4 (round 6, later): gf_subm_conv_apply_scratch / gf_subm_apply_scratch_bytes, option "subm.bf16x3", state word 4 bit 1, long rows in the matrix-core backward; 3 (round 6): gf_set_option / gf_get_option / gf_is_development_build, gf_daf_fused_forward; GF_WORKSPACE_ZEROED = one verdict word; workspace without the fused forward's per-XCD copies */

/* error codes */
#define GF_OK 0
#define GF_EINVAL (-1)    /* bad argument (null pointer, unsupported size) */
#define GF_EWORKSPACE (-2) /* workspace too small */
#define GF_ELAUNCH (-3)   /* HIP launch failure */

/* splat variants: model/head/localagg (base) vs model/head/localagg_prob{,_fast} (prob) */
#define GF_SPLAT_BASE 0
#define GF_SPLAT_PROB 1

/* number of semantic channels; compile-time constant in the reference too
 * (model/head/localagg/src/config.h:15  NUM_CHANNELS 18) */
#define GF_NUM_CHANNELS 18

/* flags for gf_splat_forward / gf_splat_backward */
#define GF_PTS_AUTO 0          /* verify on device whether pts is the dense voxel-centre grid */
#define GF_PTS_ASSUME_DENSE 1  /* caller guarantees point n lies in voxel n (N == H*W*D) */
#define GF_PTS_GENERAL 2       /* always take the arbitrary-points path */
/* exp() flavour (forward).  GF_FAST_EXP: the prep kernel pre-multiplies the quadratic form by log2(e) (fp64,
 * rounded once) and the render kernel issues a bare v_exp_f32 -- measured max error vs the reference 3.7e-6 at
 * gs25600 (2.9e-6 for the two alternatives), tolerance 1e-4.  With none of the three flags the base variant uses
 * GF_FAST_EXP and the prob variant GF_COMP_EXP: the Prob config's quadratic form cancels ~1e3 -> ~1e0, and only the
 * natural-log form, evaluated in the reference's own operation order, stays within 1e-4 of the reference there. */
#define GF_FAST_EXP 4          /* prescaled form + bare v_exp_f32 (default of the base variant) */
#define GF_LIBM_EXP 8          /* natural-log form + ocml expf (13 VALU per exp) */
#define GF_COMP_EXP 16         /* natural-log form + v_exp_f32 with a compensated argument (<= 3 ulp) */
/* prob variant, forward only: `logits` receives the un-normalised numerator sum_g semantics_g * prob_g instead of
 * numerator / probability (localagg_prob/src/forward.cu:92-98 is left to the caller).  For Gaussian-sharded inference:
 * numerators, probability and density add up over shards, 1 - bin_logits multiplies. */
#define GF_PROB_NUMERATOR 32
/* prob variant, forward and backward: evaluate det(Sigma^-1) (localagg_prob/src/forward.cu:77, backward.cu:78) in
 * fp64 instead of the reference's fp32 expression.  The default reproduces the reference's arithmetic (and its
 * cancellation noise on ill-conditioned Gaussians, including the NaN of a determinant that rounds negative); this
 * flag trades that parity for the correctly rounded value.  Pass the same flag to forward and backward. */
#define GF_PROB_EXACT_DET 64
/* Base variant, dense points: the forward renders on the matrix cores (split-f16 MFMA, fp32 accumulate; DESIGN.md
 * §3.2b; measured 1.7e-5 / 3.1e-5 from the reference's own kernels at gs25600 / gs144000, tolerance 1e-4).  This is
 * the DEFAULT whenever it applies: base variant, N == H*W*D without GF_PTS_GENERAL, no label epilogue, none of the
 * three exp-flavour flags and no GF_EXACT_FP32.  It needs pts to be an exact affine lattice of voxel centres and
 * operands the split-f16 arithmetic carries to 1e-4 (per-Gaussian bounds on theta: |theta| < 3e4 and an accuracy bound on
 * the bricks around the mean -- an isotropic Gaussian on a 0.5 m grid: sigma >= 0.056 m; |opacity * semantics| < 64).  The lattice is
 * verified on the device with GF_PTS_AUTO and asserted by the caller with GF_PTS_ASSUME_DENSE (a static property of the
 * grid); the two range conditions depend on each frame's Gaussians and are verified in the records pass of EVERY call,
 * whatever the pts flag.  A call that fails any verdict runs the arbitrary-points body instead (correct, ~7x slower;
 * reported in the state block, see gf_splat_state_bytes) -- so callers whose voxel centres are not exactly
 * representable (e.g. a 0.4 m cell) should pass GF_EXACT_FP32.  GF_MFMA_SPLAT requests this kernel explicitly (it overrides an exp-flavour
 * flag); the prob variant, the label epilogue and arbitrary points ignore it. */
#define GF_MFMA_SPLAT 128
/* Forward on the exact-fp32 VALU tile kernel (2.3e-6 / 1.0e-6 from the reference; ascending-Gaussian summation order,
 * bit-identical between the dense and the arbitrary-points bodies): the default until ABI version 1. */
#define GF_EXACT_FP32 256
/* gf_splat_backward only: the caller vouches that no other gf_splat_* call has used `workspace` since the forward that wrote
 * `state` (and that the inputs are the ones that forward saw).  The forward's records pass lays out everything the matrix-core
 * backward needs, so that pass is then not launched again (about 11 us at P = 25 601).  Checked on the device: the
 * workspace carries a generation word (bumped by every call that rewrites it) and the state block a copy of it (word GF_STATE_GENERATION); if
 * they differ the gradients are NaN, never wrong.  Without the flag the pass is launched and stands down by itself when
 * the generations agree (an empty launch).  Ignored where the matrix-core backward does not apply. */
#define GF_RECORDS_VALID 512
/* gf_splat_forward only: a backward of this call will follow.  The records pass then also lays out the matrix-core backward's
 * partial-gradient rows (a scan per 64 Gaussians) and 64 waves of the render kernel finish the layout (a prefix over
 * <= 618 totals, one word per Gaussian) and one unit per supertile publishes the supertile's candidate list -- about 1.3 us of the
 * forward at P = 25 601 -- so that gf_splat_backward starts with its gradient kernel, whose units read those lists instead of
 * scanning bitmask rows: no records pass, no set-up launch (GF_RECORDS_VALID), 25 us less.  Without it the forward does none of this and
 * the backward prepares everything itself.  The outcome is word GF_STATE_ROWS of the state block (gf_splat_state_bytes); with
 * GF_ROWS_OVERFLOW (many large Gaussians) the matrix-core backward would add what does not fit with atomics -- correct, but the
 * Gaussian-major backward, GF_EXACT_FP32, is the faster one then; the Python module follows this bit.  Rows of more than 618 words (39 552 < P <= 262 144, round 6) publish a supertile's whole one-pass list (up to
 * 896 entries).  Ignored where the matrix-core backward does not apply. */
#define GF_PREPARE_BACKWARD 1024
/* The caller promises that the workspace's first GF_SPLAT_FLAG_BYTES bytes (32 KB, its flag section) were zero when the workspace
 * was first handed to the library (e.g. allocated with hipMemset / torch.zeros) and have since only been written by the library.  The matrix-core forward
 * on the wave kernel then keeps its fall-back verdict in ONE word of that section (a double-buffered block maintained on the
 * device, so a replayed HIP graph behaves like an eager call) instead of one word per wave of the records pass that every render
 * wave has to read (19 KB per wave).  Same results; without the flag nothing changes. */
#define GF_WORKSPACE_ZEROED 2048

/* The state block (gf_splat_state_bytes): indices of its uint32 words, the words in use, and the bits of two of them. */
#define GF_STATE_NOT_DENSE 0     /* word indices */
#define GF_STATE_PATH 1
#define GF_STATE_VERDICT 2
#define GF_STATE_GENERATION 3
#define GF_STATE_ROWS 4
#define GF_STATE_WORDS 5
#define GF_VERDICT_POINT 1       /* word GF_STATE_VERDICT: a point is not in its voxel */
#define GF_VERDICT_LATTICE 2     /* ... pts is not an exact affine lattice */
#define GF_VERDICT_THETA 4       /* ... a Gaussian's quadratic-form coefficients may leave the range the kernel is accurate in */
#define GF_VERDICT_OPASEM 8      /* ... a Gaussian's |opacity * semantics| is 64 or more (4 and 8: matrix-core kernels only, every call) */
#define GF_ROWS_READY 1          /* word GF_STATE_ROWS: the matrix-core backward's rows are laid out in the workspace and all fit */
#define GF_ROWS_OVERFLOW 2       /* ... they were laid out and do NOT fit */
#define GF_SPLAT_FLAG_BYTES 32768 /* the flag section at the start of a splat workspace (GF_WORKSPACE_ZEROED: what the caller zeroes once) */

/* values of word GF_STATE_PATH after gf_splat_forward: which body rendered the call */
#define GF_PATH_EXACT_TILE 0     /* exact-fp32 tile kernel (dense grid) */
#define GF_PATH_MATRIX_CORE 1    /* split-f16 MFMA kernel (dense exact lattice), one workgroup per tile: P > 262 144, or P > 39 552 on a workspace without GF_WORKSPACE_ZEROED */
#define GF_PATH_MATRIX_CORE_WAVE 3 /* the same arithmetic (equal bits), one wave per double brick: P <= 39 552, and (long-row instantiation, GF_WORKSPACE_ZEROED) P <= 262 144 */
#define GF_PATH_MATRIX_CORE_PAIR 4 /* retired: round 5's two-waves-per-double-brick kernel (removed after a5ba306); never reported */
#define GF_PATH_MATRIX_CORE_SOLO 5 /* retired: round 5's single-wave kernel with the opacity in the exponent (removed after a5ba306); never reported */
#define GF_PATH_ARBITRARY 2      /* arbitrary-points body (pts not the dense grid, or a failed lattice / range verdict) */

int gf_abi_version(void);
const char *gf_last_error(void);

/* Library options: process-wide integers set by explicit calls -- the library never reads the environment.  Unknown names
 * return GF_EINVAL.  The product library knows six, all 0 by default, each selecting an alternative kernel kept for comparison
 * (same results within the documented bounds):
 *   "splat.mfma_tile_kernel"  1: the matrix-core forward runs on the tile kernel (one workgroup per tile) even where the wave
 *                                kernel applies (P <= 39 552); the two are bit-identical
 *   "daf.backward_tiles"      1: gf_daf_backward_sorted accumulates by pixel tiles instead of by image regions
 *   "subm.f32_mfma"           1: gf_subm_conv_apply on the exact-f32 MFMA kernel instead of the 3 x bf16 split
 *   "subm.tile_gemm"          1: gf_subm_conv_apply's gather-GEMM with one tile of 128 pairs per workgroup also on long segments
 *   "subm.bf16x3"             1: gf_subm_conv_apply_scratch on the three-term bf16 split (six products) instead of two f16 terms (three)
 *                                (>= 32 tiles per offset on average: runs of eight tiles per workgroup otherwise); equal bits
 *   "fps.exhaustive"          1: gf_farthest_point_sampling updates every bucket on every pick instead of pruning by box bounds;
 *                                the same bits (the exactness cross-check and the brute-force baseline)
 * gf_is_development_build() always returns 0 (kept for ABI 8: the development build was removed after a5ba306). */
int gf_set_option(const char *name, int value);
int gf_get_option(const char *name, int *value);
int gf_is_development_build(void);

/* Bytes of device scratch gf_splat_forward / gf_splat_backward need for these sizes. */
size_t gf_splat_workspace_bytes(int P, int N, int H, int W, int D);

/* Bytes of the small per-call state block written by gf_splat_forward and read by
 * gf_splat_backward (replaces the geomBuffer/binningBuffer/imgBuffer triple the reference
 * saves in ctx: model/head/localagg/local_aggregate/__init__.py:52-62).  Its first GF_STATE_WORDS uint32 words after a forward:
 *   [GF_STATE_NOT_DENSE]  1 = pts is NOT the dense voxel-centre grid (the backward then builds voxel2pts), 0 = it is
 *   [GF_STATE_PATH]       GF_PATH_* -- the body that rendered the forward (a GF_PATH_ARBITRARY on an N == H*W*D call is the slow
 *                         fall-back of a failed verdict: visible to the caller after its next synchronisation)
 *   [GF_STATE_VERDICT]    GF_VERDICT_* bits of the device-side checks
 *   [GF_STATE_GENERATION] the workspace's generation at that forward: every launch that rewrites the workspace's records bumps
 *                         the workspace's own generation word, so equal = the forward's records are still there (GF_RECORDS_VALID)
 *   [GF_STATE_ROWS]       GF_ROWS_* bits (GF_PREPARE_BACKWARD; 0 without it) */
size_t gf_splat_state_bytes(void);

/*
 * Gaussian -> voxel splat, forward.
 * Replaces  _C.local_aggregate            model/head/localagg/local_aggregate.h:18-28,
 *           LocalAggregateCUDA            model/head/localagg/local_aggregate.cu:35-83,
 *           Aggregator::forward           model/head/localagg/src/aggregator_impl.cu:152-252
 * and the prob / prob_fast counterparts   model/head/localagg_prob/local_aggregate.cu:35-89.
 *
 *   pts          f32 [N,3]   query points            points_int  i32 [N,3]  their voxel coords
 *   means3D      f32 [P,3]                           means3D_int i32 [P,3]
 *   opacity      f32 [P]     semantics f32 [P,18]    cov3D f32 [P,6] = (xx,yy,zz,xy,yz,xz) of Sigma^-1
 *   radii        i32 [P] (radii_per_axis=0) or i32 [P,3] (radii_per_axis=1, localagg_prob_fast)
 *   out_logits   f32 [N,18]  written in full (no pre-zeroing needed)
 *   out_bin_logits / out_density / out_probability  f32 [N]  (GF_SPLAT_PROB only, else NULL)
 *   state        gf_splat_state_bytes() bytes, kept by the caller until backward
 * Limits: C == 18, H,W <= 2047, D <= 1023, H*W*D < 2^31.
 */
int gf_splat_forward(int variant, int radii_per_axis, int flags, int P, int N, int C, int H,
                     int W, int D, const float *pts, const int *points_int,
                     const float *means3D, const int *means3D_int, const float *opacity,
                     const float *semantics, const int *radii, const float *cov3D,
                     float *out_logits, float *out_bin_logits, float *out_density,
                     float *out_probability, void *state, void *workspace,
                     size_t workspace_bytes, void *stream);

/*
 * Splat backward.
 * Replaces  _C.local_aggregate_backward   model/head/localagg/local_aggregate.h:30-43,
 *           LocalAggregateBackwardCUDA    model/head/localagg/local_aggregate.cu:85-130,
 *           Aggregator::backward          model/head/localagg/src/aggregator_impl.cu:256-307
 * and the prob counterpart                model/head/localagg_prob/local_aggregate.cu:91-148.
 * logits/bin_logits/density/probability are the forward outputs (GF_SPLAT_PROB only);
 * bin_logits_grad/density_grad may be NULL (treated as zero).  Gradient outputs
 * (means3D_grad [P,3], opacity_grad [P], semantics_grad [P,18], cov3D_grad [P,6]) are
 * written in full.
 *
 * Two implementations.  (1) The Gaussian-major exact-fp32 kernels (every variant, arbitrary points; gradients ~1e-6 of the
 * tensor's maximum from the reference's own kernels).  (2) For the base variant after a forward that one of the matrix-core
 * kernels rendered (word GF_STATE_PATH of `state`) and bitmask rows of <= 4 096 words (P <= 262 144; rows of more than 618 words, P > 39 552,
 * since round 6: they take the forward's published lists in pieces): the voxel-major matrix-core backward --
 * every double brick loads its gradient rows once, the sums over voxels are contractions on the MFMAs (split-f16 operands,
 * fp32 accumulate), per-(Gaussian, brick) partial rows are added up in a fixed order
 * (~1e-5 from the reference; tolerance 1e-3).  Which one applies is device-side knowledge, so by default BOTH pipelines are
 * launched, each gated on the state block (the one that stands down costs its empty launches).  flags:
 *   GF_EXACT_FP32   (1) only.
 *   GF_MFMA_SPLAT   (2) only: the caller has seen the state block and asserts a matrix-core forward; if the state block says
 *                   otherwise every gradient comes out NaN (never silently wrong).  Ignored where (2) does not apply.
 *   GF_RECORDS_VALID  (2) without its records pass and set-up launch: see the flag (pairs with GF_PREPARE_BACKWARD in the forward).
 *   GF_PTS_ASSUME_DENSE / GF_PTS_GENERAL as in the forward (they select (1)'s body; (2) takes its verdict from `state`).
 * The words of `state` it reads are described at gf_splat_state_bytes.
 * Limit: P <= 262 144 Gaussians per call (the block prefix of (1) lives in LDS); more is refused with GF_EINVAL -- shard the set
 * (gradients are per Gaussian: a backward per shard with the same out_grad gives the same rows; the Python op does so by itself).
 * The forward has no such limit.
 */
int gf_splat_backward(int variant, int radii_per_axis, int flags, int P, int N, int C, int H,
                      int W, int D, const float *pts, const int *points_int,
                      const float *means3D, const int *means3D_int, const float *opacity,
                      const float *semantics, const int *radii, const float *cov3D,
                      const float *logits, const float *bin_logits, const float *density,
                      const float *probability, const float *logits_grad,
                      const float *bin_logits_grad, const float *density_grad,
                      float *means3D_grad, float *opacity_grad, float *semantics_grad,
                      float *cov3D_grad, const void *state, void *workspace,
                      size_t workspace_bytes, void *stream);

/*
 * Per-Gaussian clipped box volume (tiles_touched, u32 [P]) and their total
 * (num_rendered, u64 [1], device).  Integer-exact restatement of
 * FORWARD::preprocessCUDA (model/head/localagg/src/forward.cu:9-28) + InclusiveSum's last
 * element (src/aggregator_impl.cu:193-197); used by parity tests and to report R.
 */
int gf_splat_box_volumes(int radii_per_axis, int P, int H, int W, int D,
                         const int *means3D_int, const int *radii, uint32_t *tiles_touched,
                         unsigned long long *num_rendered, void *stream);

/* radii_mode of gf_gaussian_prepare */
#define GF_RADII_SCALAR 0          /* local_aggregate:       ceil(max(scales) m / grid)              */
#define GF_RADII_SCALAR_CLAMPED 1  /* local_aggregate_prob:  ... .clamp(min=radii_min)               */
#define GF_RADII_PER_AXIS 2        /* local_aggregate_prob_fast: ceil(scales m / grid).clamp(min), [P,3] */
/* bits OR-ed into *status (the reference's host-side asserts, evaluated on the device) */
#define GF_PREPARE_MEAN_OUT_OF_GRID 1  /* means3D_int outside [0,H)x[0,W)x[0,D) */
#define GF_PREPARE_RADIUS_BELOW_ONE 2  /* radii.min() < 1 */

/*
 * Fused per-Gaussian pre-processing for the splat, no host synchronisation.
 * Replaces  GaussianHead.prepare_gaussian_args   model/head/gaussian_head.py:108-120
 *             (S, R = get_rotation_matrix(q) model/utils/utils.py:20-69, Cov = (SR)^T(SR),
 *              CovInv = Cov.cpu().inverse().cuda())
 *           LocalAggregator.forward integer path  model/head/localagg/local_aggregate/__init__.py:139-143
 *             (means3D_int, radii, the [0,4,8,1,5,2] packing and the .min()/.max() asserts)
 *   means3D f32 [P,3]   scales f32 [P,3]   rotations f32 [P,4] (w,x,y,z; normalised inside)
 *   pc_min: 3 floats on the HOST.  Any output pointer may be NULL to skip it:
 *   means3D_int i32 [P,3]   radii i32 [P] ([P,3] for GF_RADII_PER_AXIS)
 *   cov6 f32 [P,6] = Sigma^-1 as (xx,yy,zz,xy,yz,xz)   cov9 f32 [P,9] = full Sigma^-1
 *   status i32 [1] (device, caller-zeroed): GF_PREPARE_* bits, checked by the caller when it wants to
 * Sigma^-1 = R^T S^-2 R in closed form; differs from the reference's fp32 LAPACK inverse by
 * O(cond(Sigma) * 2^-24) relative.  A quaternion of norm below 1e-12 (the clamp of F.normalize) has no direction and
 * is taken as the zero quaternion: Sigma^-1 = 0, and a zero rotation gradient in gf_gaussian_prepare_backward.
 */
int gf_gaussian_prepare(int P, int H, int W, int D, const float *pc_min, float grid_size,
                        float scale_multiplier, int radii_mode, int radii_min,
                        const float *means3D, const float *scales, const float *rotations,
                        int *means3D_int, int *radii, float *cov6, float *cov9, int *status,
                        void *stream);

/*
 * The tensor surgery of prepare_gaussian_args ahead of the covariance, one launch.
 * Replaces  GaussianHead.prepare_gaussian_args   model/head/gaussian_head.py:88-109
 *             (zeros column + torch.cat for the semantics, the appended "empty" Gaussian -- five torch.cat --, or the
 *              softmax + zero column of the prob head)
 *   means3D/scales [P,3], rotations [P,4], semantics [P,Cin], opacities [P] or NULL (= ones)       -> device
 *   empty_mean[3], empty_scale[3], empty_rot[4]                                                       -> HOST (buffers of the head)
 *   empty_scalar                                                                                      -> device, 1 float (a parameter)
 *   outputs [P + with_empty, ...], semantics_out [.., Cout] with Cout = Cin or Cin + 1: the extra (zero) column is the last
 *   one, or the first with zero_first (the kitti datasets); softmax = 1 applies torch.softmax over the Cin inputs first.
 */
int gf_gaussian_pack(int P, int Cin, int Cout, int zero_first, int with_empty, int softmax, int empty_label,
                     const float *means3D, const float *scales, const float *rotations, const float *semantics,
                     const float *opacities, const float *empty_mean, const float *empty_scale,
                     const float *empty_rot, const float *empty_scalar, float *means_out, float *scales_out,
                     float *rotations_out, float *semantics_out, float *opacities_out, void *stream);

/*
 * Gradient of Sigma^-1 with respect to scales [P,3] and (un-normalised) rotations [P,4]: what
 * autograd computes through gaussian_head.py:108-119.  cov_grad is [P,6] (gradient of the packed
 * entries, as gf_splat_backward's cov3D_grad) or, with grad_is_full, an arbitrary [P,9].
 */
int gf_gaussian_prepare_backward(int P, int grad_is_full, const float *scales, const float *rotations,
                                 const float *cov_grad, float *scales_grad, float *rotations_grad,
                                 void *stream);

/*
 * Multi-camera multi-level deformable aggregation, forward.
 * Replaces  deformable_aggregation_forward  model/encoder/gaussian_encoder/ops/src/deformable_aggregation.cpp:41-71
 *           deformable_aggregation_kernel   .../ops/src/deformable_aggregation_cuda.cu:125-187
 *   mc_ms_feat f32 [B,cams,num_feat,C]   spatial_shape i32 [L,2]   scale_start_index i32 [L]
 *   sampling_location f32 [B,pts,cams,2] weights f32 [B,pts,cams,L,G]   output f32 [B,pts,C]
 * Requires C % G == 0.
 */
int gf_daf_forward(int B, int num_cams, int num_feat, int C, int L, int num_pts, int G,
                   const float *mc_ms_feat, const int *spatial_shape,
                   const int *scale_start_index, const float *sampling_location,
                   const float *weights, float *output, void *stream);

/*
 * The same forward with the channel groups PINNED TO XCDs: XCD x only ever reads channel group x % G of the pyramid (a
 * quarter of it at G = 4, so the three coarse levels of all cameras stay in its 4 MB L2), at the price of reading the
 * sampling locations and weights once per group.  Bit-identical output.  Faster when many cameras see a point at
 * unrelated places (230 400 points at uniform random locations, 3.06 visible cameras each: 502 against 595 us), slower
 * on projected geometry (1.04 visible cameras, neighbouring taps: 153 against 123 us) -- hence a separate entry, not
 * the default.  Layouts other than 4 channels per lane with groups of 32 channels fall back to gf_daf_forward.
 */
int gf_daf_forward_pinned(int B, int num_cams, int num_feat, int C, int L, int num_pts, int G,
                          const float *mc_ms_feat, const int *spatial_shape, const int *scale_start_index,
                          const float *sampling_location, const float *weights, float *output, void *stream);

/*
 * Deformable aggregation, backward.  The three gradient buffers must be zero on entry, as the reference's
 * Python side makes them (ops/deformable_aggregation.py:55-67): grad_mc_ms_feat is accumulated; an entry of
 * grad_weights / grad_sampling_location has exactly one producer and is stored, not added (entries of cameras
 * that do not see the point keep their zero).
 * Replaces  deformable_aggregation_backward  .../ops/src/deformable_aggregation.cpp:73-110
 *           deformable_aggregation_grad_kernel .../ops/src/deformable_aggregation_cuda.cu:190-259
 */
int gf_daf_backward(int B, int num_cams, int num_feat, int C, int L, int num_pts, int G,
                    const float *mc_ms_feat, const int *spatial_shape,
                    const int *scale_start_index, const float *sampling_location,
                    const float *weights, const float *grad_output, float *grad_mc_ms_feat,
                    float *grad_sampling_location, float *grad_weights, void *stream);

/*
 * Deformable aggregation backward, pixel-major gradient of the feature maps.  Same arguments,
 * results and zero-on-entry contract as gf_daf_backward, plus a device
 * workspace.  grad_weights / grad_sampling_location come from the same point-major kernel;
 * grad_mc_ms_feat is produced without the reference's per-channel atomic scatter
 * (deformable_aggregation_cuda.cu:92-110): taps are bucketed by destination pixel row with a
 * counting sort and every row is gathered (summation order within a row is unspecified, as
 * with the atomics).  gf_daf_backward_workspace_bytes returns 0 for shapes this path does not
 * support (it needs C % 4 == 0, C/4 in {16,32,64}, (C/G) % 4 == 0 and 32-bit tap ids); use
 * gf_daf_backward for those.
 */
size_t gf_daf_backward_workspace_bytes(int B, int num_cams, int num_feat, int C, int L, int num_pts, int G);
int gf_daf_backward_sorted(int B, int num_cams, int num_feat, int C, int L, int num_pts, int G,
                           const float *mc_ms_feat, const int *spatial_shape,
                           const int *scale_start_index, const float *sampling_location,
                           const float *weights, const float *grad_output, float *grad_mc_ms_feat,
                           float *grad_sampling_location, float *grad_weights, void *workspace,
                           size_t workspace_bytes, void *stream);

/*
 * Kernel-level timing for bench.py's roofline leg.  gf_profile_enable(n) pre-creates n
 * hipEvent pairs; while enabled, every gf_splat_forward call brackets its dominant kernel
 * (the dense render kernel) with hipEventRecord on the caller's stream (asynchronous, no
 * host sync).  gf_profile_read() waits for the recorded events, writes the per-launch
 * durations in milliseconds, resets the ring and returns how many were written.
 * gf_profile_enable(0) disables and frees.  Not part of the reference interface.
 */
int gf_profile_enable(int max_pairs);
/*
 * feature_maps_format (model/encoder/gaussian_encoder/ops/deformable_aggregation.py:77-117): L image-feature levels
 * [planes, C, hw_l] (planes = bs * cams, contiguous) <-> one channels-last table [planes, sum_l hw_l, C], level l
 * starting at row sum_{k<l} hw_k.  inverse = 0 fills the table from the levels, inverse = 1 the levels from the
 * table (the backward of the former).  hw and levels are HOST arrays (L <= 8 ints / device pointers).
 */
int gf_feature_maps_format(int planes, int C, int L, const int *hw, float *const *levels, float *table,
                           int inverse, void *stream);

/*
 * Submanifold sparse 3-D convolution over point cells: the operator of
 * SparseConv3D (model/encoder/gaussian_encoder/spconv3d_module.py:10-83; spconv.SubMConv3d, kernel K, stride 1,
 * padding K/2, no bias).  spconv is not in the reference tree; the published algorithm is restated:
 *     out[i] = sum_k sum_{j : cell(j) = cell(i) + offset_k} features[j] . weight[k]
 * with offsets in [K,K,K] order (x major, z fastest) and weight f32 [K^3, Cin, Cout].  Points sharing a cell all
 * contribute and all receive that cell's output (= a dense convolution of the scattered-and-summed features,
 * read back at the points).  indices i32 [N,4] = (batch, x, y, z); points outside the grid are inactive (output 0).
 *
 * Call order:
 *   1. gf_subm_rulebook_count builds the device tables.  The total pair count is the i64 at byte
 *      gf_subm_tables_bytes(..) - 256 of `tables`; the i64 after it is non-zero when the point set is refused
 *      (bit 0: a cell with more than 65535 points, bit 1: more than 2^31 - 1 pairs) -- the caller must stop there.
 *   2. the caller allocates pair_in / pair_out (i32 [total]) and partial (f32 [total, Cout]);
 *   3. gf_subm_rulebook_fill;
 *   4. gf_subm_conv_apply, any number of times (the gradient w.r.t. the features is the same call with
 *      weight'[k] = weight[K^3-1-k]^T), and gf_subm_conv_weight_grad.
 * Without the host read: gf_subm_rulebook_build does steps 1 and 3 in one call for pair arrays the caller sized in
 * advance (`pair_capacity` entries; partial f32 [pair_capacity, Cout]; pass pair_capacity as `total_pairs` below).  A
 * point set with more pairs than that leaves the rulebook EMPTY, sets bit 2 of the refusal word -- which the caller
 * reads whenever it next synchronises -- and makes gf_subm_conv_apply write NaN to every output row (a refusal must
 * not look like a feature).
 * Cin and Cout in {32, 64, 128} (the reference uses 128 -> 128), K odd <= 7.  gf_subm_conv_apply multiplies on the
 * bf16 matrix cores with fp32-EQUIVALENT operands: every fp32 value is split into three bf16 terms and a product is
 * six v_mfma_f32_32x32x16_bf16 partial products accumulated in fp32 (the dropped terms are <= 2^-24 relative each);
 * gf_set_option("subm.f32_mfma", 1) selects the f32-MFMA kernel instead (v_mfma_f32_32x32x2_f32: bitwise an fmaf
 * chain, ~13 % slower).  The weight gradient runs on f32 MFMAs with blocked summation (32 pairs summed from zero, the
 * blocks added per chunk of 512 pairs, float atomics between the chunks of a segment): measured <= 3.6 * 2^-24 sum|a||b| per
 * element on ordinary operands and <= 13.4 * 2^-24 where a few products dominate a sum.  Results are deterministic except the weight gradient
 * of segments longer than 512 pairs (float atomics between their chunks).
 * gf_subm_conv_apply_scratch (round 6) is the same operator with `scratch` of gf_subm_apply_scratch_bytes(N, Cin) bytes (device,
 * 16-byte aligned, contents irrelevant before and after the call): the feature rows are split once per call into TWO f16 terms
 * under an exact power-of-two scale per row (the weight slices likewise, per output column) and a product is THREE
 * v_mfma_f32_32x32x16_f16 partial products (dropped term <= 2^-22 relative) -- half the matrix-core work of the bf16 form,
 * ~2^-21 per product instead of 2^-24 (both far inside 3e-5 of the fp64 definition, tests/test_subm_conv.py).  f16 has less
 * RANGE than fp32, and that is part of the contract: a row (column) is scaled so that its largest |x| lies in [2^14, 2^15), so an
 * element more than 2^17 times smaller than its row's (column's) largest loses its lo term to f16's subnormal spacing -- each
 * operand errs by at most 2^-22 |x| + 2^-39 max|row or column|, and an output element by at most
 *     2^-20 sum|a||b|  +  2 * 2^-39 (sum_pairs max|a_row| sum_c |b_c|  +  sum_pairs sum_c |a_c| max|b_column|)
 * (tests/subm_judge.py holds every element of the output and of the input gradient to exactly this, and the
 * bf16 and f32 formats, which have fp32's range, to the first term alone).  The second term matters only where a row's or a
 * column's large elements do not dominate sum|a||b|.  The Python
 * module calls this one; gf_set_option("subm.bf16x3", 1) makes it take the three-term bf16 kernels (= gf_subm_conv_apply),
 * "subm.f32_mfma" the exact-f32 MFMA kernel.
 */
/* (round 5) The block's own preamble -- voxel indices (batch, x, y, z) of the anchor centres, spconv3d_module.py:56-66 -- in one
 * launch instead of a dozen elementwise ops; the same fp32 operations in the same order, each rounded on its own.  `anchor` is
 * [rows, anchor_stride] fp32 on the device (centre in the first three columns), batch index = row / per_batch; span = hi - lo and
 * lo of pc_range (what `cartesian` multiplies and adds), pc_lo / grid = the module's pc_range[:3] and grid_size buffers: four host
 * arrays of three floats.  out: int32 [rows, 4] on the device, 16-byte aligned. */
int gf_subm_voxelize(long long rows, int per_batch, int anchor_stride, int use_sigmoid, const float *anchor, const float *span,
                     const float *lo, const float *pc_lo, const float *grid, int *out, void *stream);
size_t gf_subm_tables_bytes(int N, int batch, int X, int Y, int Z, int K);
int gf_subm_rulebook_count(int N, int batch, int X, int Y, int Z, int K, const int *indices, void *tables,
                           size_t tables_bytes, void *stream);
int gf_subm_rulebook_fill(int N, int batch, int X, int Y, int Z, int K, const int *indices, void *tables,
                          int *pair_in, int *pair_out, void *stream);
int gf_subm_rulebook_build(int N, int batch, int X, int Y, int Z, int K, const int *indices, void *tables,
                           size_t tables_bytes, int *pair_in, int *pair_out, long long pair_capacity, void *stream);
/* The same three with an OUTPUT RANGE (round 5; the anchor-sharded frame, where the reference would run the whole SparseConv3D,
 * spconv3d_module.py:10-83, on every replica): pairs are made for the output points [out_lo, out_hi) only, every point of the set
 * stays a neighbour.  gf_subm_conv_apply on such a rulebook computes those rows (the others come out as zeros) with
 * (out_hi - out_lo) / N of the gather-GEMM work; the pair count at the end of `tables` counts the range's pairs. */
int gf_subm_rulebook_count_range(int N, int batch, int X, int Y, int Z, int K, int out_lo, int out_hi, const int *indices,
                                 void *tables, size_t tables_bytes, void *stream);
int gf_subm_rulebook_fill_range(int N, int batch, int X, int Y, int Z, int K, int out_lo, int out_hi, const int *indices,
                                void *tables, int *pair_in, int *pair_out, void *stream);
int gf_subm_rulebook_build_range(int N, int batch, int X, int Y, int Z, int K, int out_lo, int out_hi, const int *indices,
                                 void *tables, size_t tables_bytes, int *pair_in, int *pair_out, long long pair_capacity,
                                 void *stream);
int gf_subm_conv_apply(int N, int batch, int X, int Y, int Z, int K, int Cin, int Cout, long long total_pairs,
                       const float *features, const float *weight, const void *tables, const int *pair_in,
                       float *partial, float *out, void *stream);
size_t gf_subm_apply_scratch_bytes(int N, int Cin);
int gf_subm_conv_apply_scratch(int N, int batch, int X, int Y, int Z, int K, int Cin, int Cout, long long total_pairs,
                               const float *features, const float *weight, const void *tables, const int *pair_in,
                               float *partial, float *out, void *scratch, size_t scratch_bytes, void *stream);
/* gf_subm_conv_apply_scratch with an epilogue in its last pass (the reduction holds a finished row in registers): for every
 * row i < N, with c the sum of the row's partial rows in exactly the order gf_subm_conv_apply_scratch forms it,
 *     out[i] = relu?( LN?( (c + bias) + residual[i] ) )
 * every part optional (NULL / relu = 0), applied in that order; with all of them absent the bytes are gf_subm_conv_apply_scratch's.
 * LN is LayerNorm over the Cout values with eps = 1e-5 and biased variance, the mean first and then the squared deviations --
 * gf_ffn_forward's rule; a lane sums its four values as (x + y) + (z + w) and the Cout / 4 lanes of a row combine by a
 * butterfly (xor Cout / 8 .. 1), so a row's bits depend neither on N nor on the row's place in its workgroup.  ReLU is
 * v < 0 ? 0 : v: a NaN stays a NaN, and an over-capacity rulebook gives NaN in every output row whatever epilogue is asked for.
 * bias, ln_weight, ln_bias: [Cout]; residual: [N, Cout]; all device pointers, 16-byte aligned, read only.  Refused with
 * GF_EINVAL before any HIP call: ln_weight without ln_bias or the reverse, relu other than 0 or 1, a misaligned pointer, out
 * overlapping residual or any other input, and everything gf_subm_conv_apply_scratch refuses.  scratch is
 * gf_subm_apply_scratch_bytes(N, Cin) bytes as there.  N == 0 returns GF_OK without a launch.  No host synchronisation, no
 * allocation, no atomics: graph-capturable and bitwise reproducible. */
int gf_subm_conv_apply_epilogue(int N, int batch, int X, int Y, int Z, int K, int Cin, int Cout, long long total_pairs,
                                const float *features, const float *weight, const void *tables, const int *pair_in,
                                float *partial, float *out, void *scratch, size_t scratch_bytes, const float *bias,
                                const float *residual, const float *ln_weight, const float *ln_bias, int relu, void *stream);
/* The training step of a stage y = relu?( LN( (c + bias?) + residual? ) ), the three conv + LayerNorm + ReLU stages of
 * spconv3d_module.py:26-37 (and a single-layer block's norm(conv + residual)); the LayerNorm pair is required.
 *
 * gf_subm_stage_train_sizes (spconv3d_module.py:26-37): host code; the bytes of the two caller-allocated regions of a stage of N
 * rows: `saved` holds pre [N, Cout], `workspace` the backward's partial triples (both 0 for N == 0, both monotone in N).
 * GF_EINVAL: Cout outside {32, 64, 128}, N < 0, a null pointer.
 *
 * gf_subm_conv_apply_epilogue_train (spconv3d_module.py:26-37): gf_subm_conv_apply_epilogue -- the same arguments, the same
 * refusals, out BITWISE the same -- that also stores pre[i] = (c + bias) + residual[i], the row the LayerNorm reads, to
 * pre [N, Cout] (16-byte aligned, overlapping neither out nor an input).  Mean and rstd are not saved: the backward recomputes
 * them from pre by the forward's own arithmetic.  ln_weight / ln_bias must both be given.
 *
 * gf_subm_stage_backward (spconv3d_module.py:26-37): from grad_out = dL/dy [N, Cout] and pre, with xhat, mean, rstd of pre,
 *     u = xhat ln_weight + ln_bias,   g_u = relu ? (u > 0 ? grad_out : 0) : grad_out,   g_xhat = g_u ln_weight,
 *     grad_pre = rstd (g_xhat - mean_c(g_xhat) - xhat mean_c(g_xhat xhat))               (= dL/dc = dL/dresidual)
 *     grad_ln_bias = sum_i g_u,  grad_ln_weight = sum_i g_u xhat,  grad_bias = sum_i grad_pre   (grad_bias may be NULL)
 * A workgroup sums the three column terms over its 256 / (Cout / 4) rows in a fixed order (a wave's rows by a butterfly, the
 * four waves in their order), writes one partial triple to `workspace`, and a second launch adds the partials in double in a
 * fixed order: no float atomics, bitwise reproducible.  A row of pre with a NaN or an infinity (an over-capacity rulebook's
 * forward) gives NaN in grad_pre and in all three sums.
 *
 * gf_subm_conv_apply_stage_backward (spconv3d_module.py:26-37): gf_subm_conv_apply_scratch's arguments without `out`, then the
 * stage backward's without grad_out: the convolution's finished row IS dL/dy of the stage whose rows `pre` are (the caller passes
 * the next stage's grad_pre as features and that stage's mirrored, transposed weight, Cout = the width of `pre`); it goes through
 * the stage backward in the reduce pass's registers and only grad_pre is stored.  grad_pre and the three sums are BITWISE those
 * of gf_subm_conv_apply_scratch followed by gf_subm_stage_backward.
 *
 * Both backward entries refuse with GF_EINVAL before any HIP call: a null ln_weight or ln_bias, relu other than 0 or 1, a
 * misaligned pointer, grad_pre overlapping any input or the workspace, Cout (Cin) outside {32, 64, 128}; GF_EWORKSPACE: a
 * workspace shorter than gf_subm_stage_train_sizes says.  N == 0 returns GF_OK with the parameter gradients zero-filled.  No
 * allocation, no host synchronisation: graph-capturable. */
int gf_subm_stage_train_sizes(int N, int Cout, size_t *saved_bytes, size_t *workspace_bytes);
int gf_subm_conv_apply_epilogue_train(int N, int batch, int X, int Y, int Z, int K, int Cin, int Cout, long long total_pairs,
                                      const float *features, const float *weight, const void *tables, const int *pair_in,
                                      float *partial, float *out, void *scratch, size_t scratch_bytes, const float *bias,
                                      const float *residual, const float *ln_weight, const float *ln_bias, int relu, float *pre,
                                      void *stream);
int gf_subm_stage_backward(int N, int Cout, const float *pre, const float *grad_out, const float *ln_weight, const float *ln_bias,
                           int relu, float *grad_pre, float *grad_ln_weight, float *grad_ln_bias, float *grad_bias, void *workspace,
                           size_t workspace_bytes, void *stream);
int gf_subm_conv_apply_stage_backward(int N, int batch, int X, int Y, int Z, int K, int Cin, int Cout, long long total_pairs,
                                      const float *features, const float *weight, const void *tables, const int *pair_in,
                                      float *partial, void *scratch, size_t scratch_bytes, const float *pre, const float *ln_weight,
                                      const float *ln_bias, int relu, float *grad_pre, float *grad_ln_weight, float *grad_ln_bias,
                                      float *grad_bias, void *workspace, size_t workspace_bytes, void *stream);
int gf_subm_conv_weight_grad(int N, int batch, int X, int Y, int Z, int K, int Cin, int Cout, long long total_pairs,
                             const float *features, const float *grad_out, const void *tables, const int *pair_in,
                             const int *pair_out, float *grad_weight, void *stream);

/* modes of gf_head_labels */
#define GF_LABELS_ARGMAX 0          /* base head: argmax over the 18 logits (gaussian_head.py:185) */
#define GF_LABELS_PROB_THRESHOLD 1  /* prob head: argmax where bin_logits > threshold, else empty_label (:178-183) */
#define GF_LABELS_PROB_GEOSEM 2     /* prob head with combine_geosem: argmax of cat(logits[:,:-1]*bin, 1-bin) (:166-170,:185) */

/*
 * Occupancy labels straight from the splat outputs, replacing the transposes,
 * argmax and mask kernels at the end of GaussianHead.forward (model/head/gaussian_head.py:164-185).
 *   logits f32 [N,18]   bin_logits f32 [N] (prob modes, else NULL)   labels i64 [N] (torch.argmax's dtype)
 * Ties resolve to the first maximal channel, like torch.argmax.
 */
int gf_head_labels(long long N, int C, int mode, const float *logits, const float *bin_logits,
                   float threshold, int empty_label, long long *labels, void *stream);

/*
 * The prob head's geosem step (model/head/gaussian_head.py:166-168), one launch each way instead of three torch launches
 * with two [N,17] / [N,18] intermediates (backward: autograd's zero-fill, two products and a strided sum):
 *   forward    out[n,c] = logits[n,c] * bin_logits[n] (c < 17),  out[n,17] = 1 - bin_logits[n]
 *              labels (may be NULL): the head's final_occ of the row, by gf_head_labels' GF_LABELS_PROB_GEOSEM rule -- the same
 *              labels bit for bit, from the same launch
 *   backward   grad_logits[n,c] = grad_out[n,c] * bin_logits[n] (c < 17),  grad_logits[n,17] = +0.0
 *              grad_bin[n] = sum_{c<17} grad_out[n,c] * logits[n,c] - grad_out[n,17]
 *   logits, out, grad_out, grad_logits f32 [N,18]   bin_logits, grad_bin f32 [N]   labels i64 [N]
 * Every element of out and grad_logits is one correctly rounded fp32 operation (equal to the torch expression bit for bit);
 * grad_bin is summed in fp32 in ascending c by one lane per row, no atomics: it repeats bit for bit.  Non-finite inputs
 * propagate by IEEE rules.  C must be 18.  Any 4-byte aligned base pointer is taken (16-byte accesses where a base allows);
 * inputs and outputs must not alias.  N == 0 returns GF_OK.  No host read, no allocation.
 */
int gf_head_geosem_forward(long long N, int C, const float *logits, const float *bin_logits,
                           float *out, long long *labels /* may be NULL */, void *stream);
int gf_head_geosem_backward(long long N, int C, const float *logits, const float *bin_logits,
                            const float *grad_out, float *grad_logits, float *grad_bin, void *stream);

/*
 * gf_splat_forward with the head epilogue folded into the render kernel: the labels are taken from
 * the accumulators (same rules as gf_head_labels).  out_logits may be NULL (labels only: the
 * 46 MB logits are never written); for the prob variant the three extra outputs must then be NULL too.
 */
int gf_splat_forward_labels(int variant, int radii_per_axis, int flags, int P, int N, int C, int H, int W, int D,
                            const float *pts, const int *points_int, const float *means3D, const int *means3D_int,
                            const float *opacity, const float *semantics, const int *radii, const float *cov3D,
                            float *out_logits, float *out_bin_logits, float *out_density, float *out_probability,
                            int label_mode, float threshold, int empty_label, long long *out_labels,
                            void *state, void *workspace, size_t workspace_bytes, void *stream);

/*
 * (round 6) The deformable aggregation of an INFERENCE frame in one launch: project_points, mask / all_miss / softmax, the
 * multi-scale bilinear sampling and the sum over the key points (deformable_module.py:174-233,242; ops/src/
 * deformable_aggregation_cuda.cu:125-187) -- gf_daf_prepare + gf_daf_forward + features.sum(dim=2) without the [A*pts, cams, L, G]
 * weights tensor and the [A*pts, C] sampled features in between.  No gradients (training keeps the three steps).
 *   key_points f32 [B,A,pts,3]   projection_mat f32 [B,cams,4,4]   image_wh f32 [B,cams,2] or NULL
 *   the attention logits, either  raw_weights f32 [B,A,cams,L,pts,G]  (weights_fc output as reshaped at :243-253; the other two NULL)
 *                        or       raw_anchor f32 [B,A,L,pts,G] + raw_cam f32 [B,cams,L,pts,G]  (use_camera_embed, :253-262: weights_fc
 *                                 is linear, so its output is the sum of an anchor part and a camera part -- added on the fly here)
 *   mc_ms_feat / spatial_shape / scale_start_index / num_feat as gf_daf_forward
 *   out f32 [B,A,C]
 * G a power of two, pts * cams <= 256, L * G <= 64, C a multiple of 8 G with C / 8 dividing 64.  Equal to the three-step path up to
 * the order of the sums (~1e-6 of a row's magnitude).
 */
int gf_daf_fused_forward(int B, int A, int pts, int cams, int L, int G, int C, int num_feat, const float *key_points,
                         const float *projection_mat, const float *image_wh, const float *raw_weights, const float *raw_anchor,
                         const float *raw_cam, const float *mc_ms_feat, const int *spatial_shape, const int *scale_start_index,
                         float *out, void *stream);

/*
 * gf_daf_fused_forward with the attention-dropout keep-mask of training (deformable_module.py:199-214, 263-282):
 *   weight_mask u8 [B,A,cams,L,pts,G] (the layout of raw_weights and of gf_daf_prepare's mask; non-zero = keep) or NULL.
 * A dropped entry leaves its group's maximum and sum and weighs 0; a group whose entries are all dropped or invisible gives zero
 * channels (the reference's all_miss, which can hold for one group of an anchor and not for the others).  With weight_mask NULL
 * this is gf_daf_fused_forward (the same kernel: the same bits).  Other arguments and limits as gf_daf_fused_forward.
 */
int gf_daf_fused_forward_masked(int B, int A, int pts, int cams, int L, int G, int C, int num_feat, const float *key_points,
                                const float *projection_mat, const float *image_wh, const float *raw_weights, const float *raw_anchor,
                                const float *raw_cam, const unsigned char *weight_mask, const float *mc_ms_feat,
                                const int *spatial_shape, const int *scale_start_index, float *out, void *stream);

/* Bytes of the workspace gf_daf_fused_backward needs for grad_raw_cam (per-workgroup partial sums); 0 for invalid sizes. */
size_t gf_daf_fused_backward_workspace_bytes(int B, int A, int pts, int cams, int L, int G);

/*
 * Backward of gf_daf_fused_forward_masked (training): replaces the autograd of the reference's block -- the softmax / mask /
 * all_miss (deformable_module.py:199-233), DAF backward (ops/src/deformable_aggregation_cuda.cu:56-121, 190-259), the sum over the
 * key points (:242) and project_points (:268-285) -- without the [A*pts, cams, L, G] weights tensor and the [A*pts, C] expanded
 * gradient.  For anchor a, group g and kept entries e = (pt, cam, l), w_e the forward's weight and S_e[c] its bilinear sample:
 *   gw_e = sum_{c in g} grad_out[a,c] S_e[c],   d logit_e = w_e (gw_e - sum_e' w_e' gw_e')   (0 where not kept, 0 for all-miss groups)
 * Inputs: the forward's (the same logits form, the same weight_mask or NULL) and grad_out f32 [B,A,C] (16-byte aligned).
 * Outputs, each may be NULL:
 *   grad_mc_ms_feat f32 like mc_ms_feat: ACCUMULATED (zero it first), float atomics -- the last bits may differ between runs
 *   grad_key_points f32 [B,A,pts,3]                     (gf_daf_prepare_backward's projection backward)
 *   grad_raw_weights f32 [B,A,cams,L,pts,G]             (full logits only)
 *   grad_raw_anchor f32 [B,A,L,pts,G]                   (split logits only: d logit summed over the cameras)
 *   grad_raw_cam f32 [B,cams,L,pts,G]                   (split logits only: d logit summed over the anchors of each batch element;
 *                                                        needs gf_daf_fused_backward_workspace_bytes(B, A, pts, cams, L, G) bytes)
 * Every output but grad_mc_ms_feat is fully written, zeros included.  Limits as gf_daf_fused_forward, and one wave's LDS (the gw
 * of every visible entry, pts * cams * L * G floats) must fit a CU: shapes the forward takes are all taken for L * G <= 43 (the
 * reference's block: 16); larger ones may be refused with GF_EINVAL.  Every check runs before any HIP call.
 */
int gf_daf_fused_backward(int B, int A, int pts, int cams, int L, int G, int C, int num_feat, const float *key_points,
                          const float *projection_mat, const float *image_wh, const float *raw_weights, const float *raw_anchor,
                          const float *raw_cam, const unsigned char *weight_mask, const float *mc_ms_feat, const int *spatial_shape,
                          const int *scale_start_index, const float *grad_out, float *grad_mc_ms_feat, float *grad_key_points,
                          float *grad_raw_weights, float *grad_raw_anchor, float *grad_raw_cam, void *workspace,
                          size_t workspace_bytes, void *stream);

/*
 * Fused caller-side preparation of the deformable aggregation.
 * Replaces, in DeformableFeatureAggregation.forward (model/encoder/gaussian_encoder/deformable_module.py):
 *   project_points :268-285 (4x4 projection, depth clamp 1e-5, image_wh normalisation, visibility mask),
 *   the weights / weight_mask permutes :174-193, the -inf masking, all_miss handling and softmax :199-214.
 *   key_points f32 [B,A,pts,3]   projection_mat f32 [B,cams,4,4]   image_wh f32 [B,cams,2] or NULL
 *   raw_weights f32 [B,A,cams,L,pts,G] (weights_fc output as reshaped at :243-253)
 *   weight_mask u8 same layout (attention-dropout keep mask, :263) or NULL = keep all
 * Outputs, in the layouts gf_daf_forward takes:
 *   points_2d f32 [B,A*pts,cams,2]   weights f32 [B,A*pts,cams,L,G]
 * G must be a power of two <= 64 and pts*cams <= 256.
 */
int gf_daf_prepare(int B, int A, int pts, int cams, int L, int G, const float *key_points,
                   const float *projection_mat, const float *image_wh, const float *raw_weights,
                   const unsigned char *weight_mask, float *points_2d, float *weights, void *stream);

/*
 * Its gradient: grad_raw_weights [B,A,cams,L,pts,G] from (weights, grad_weights) and
 * grad_key_points [B,A,pts,3] from grad_points_2d; either output may be NULL.
 */
int gf_daf_prepare_backward(int B, int A, int pts, int cams, int L, int G, const float *key_points,
                            const float *projection_mat, const float *image_wh, const float *weights,
                            const float *grad_weights, const float *grad_points_2d, float *grad_raw_weights,
                            float *grad_key_points, void *stream);

/*
 * ---- key points of the deformable aggregation (first step of the caller preparation) --------
 * Replaces SparseGaussian3DKeyPointsGenerator.forward (model/encoder/gaussian_encoder/deformable_module.py:51-90)
 * with its default sigmoid activations: per anchor, F fixed + K learned offsets, times the activated scale
 * (scale_lo + (scale_hi - scale_lo) * safe_sigmoid(anchor[3:6])), rotated by get_rotation_matrix(anchor[6:10])^T
 * (model/utils/utils.py:20-69), plus the activated centre (pc_range, safe_sigmoid(anchor[0:3])).
 *   anchor     f32 [n, anchor_dim >= 10]  (xyz, scale, quaternion (w,x,y,z), ...) before activation; n = bs * anchors
 *   learned    f32 [n, K, 3]   raw output of learnable_fc (may be NULL when K == 0)
 *   fix_scale  f32 [F, 3]      device pointer, F <= 16
 *   pc_range   6 floats, HOST pointer
 *   identity_activations  bit 0: xyz_activation is not "sigmoid" (the centre columns are used as they are, :79-80);
 *                         bit 1: scale_activation is not "sigmoid" (:66-67).  0 = the reference configs.
 *   key_points f32 [n, F + K, 3]
 */
int gf_key_points(int n, int anchor_dim, int F, int K, const float *anchor, const float *learned, const float *fix_scale,
                  const float *pc_range, float scale_lo, float scale_hi, float learnable_fixed_scale,
                  int identity_activations, float *key_points, void *stream);

/* Its gradient: grad_anchor [n, anchor_dim] (columns >= 10 are written as zero), grad_learned [n, K, 3]. */
int gf_key_points_backward(int n, int anchor_dim, int F, int K, const float *anchor, const float *learned,
                           const float *fix_scale, const float *pc_range, float scale_lo, float scale_hi,
                           float learnable_fixed_scale, int identity_activations, const float *grad_key_points,
                           float *grad_anchor, float *grad_learned, void *stream);

/* ---- farthest point sampling -------------------------------------------------------------------------------------
 * Replaces pointops.farthest_point_sampling(xyz, offset, new_offset) as GaussianLifterV2 calls it with random_sampling=False
 * (model/lifter/gaussian_lifter_v2.py:233-251; pointops is not part of the reference tree).  Segment s is points
 * [offset[s-1], offset[s]) and writes picks [new_offset[s-1], new_offset[s]) (offset[-1] = new_offset[-1] = 0):
 *   the first pick is the segment's first point; every point keeps d = 1e10f; after each pick c, d[p] = min(d[p], dist2(p, c))
 *   with dist2 = (dx*dx + dy*dy) + dz*dz, dx = p.x - c.x, each operation rounded to fp32 and none fused; the next pick is the
 *   point with the largest d, ties to the LOWEST index (this op's own rule).  More picks than points repeat by the same rule.
 * The result is bit-for-bit deterministic.  One workgroup per segment; at most 262 144 points per segment.
 *   xyz         f32 [n, 3]
 *   offset_host, new_offset_host   int [b], HOST pointers: validated here (non-decreasing, offset[b-1] == n, no segment over
 *               the limit, no empty segment with picks) before any HIP call
 *   offset, new_offset             int [b], DEVICE copies of the same values (the kernel reads them)
 *   idx         int [new_offset[b-1]]  global indices into xyz
 *   workspace   gf_fps_workspace_bytes(n) bytes
 * gf_set_option("fps.exhaustive", 1) updates every point on every pick (no pruning; the same bits). */
size_t gf_fps_workspace_bytes(int n);
int gf_farthest_point_sampling(int n, int b, const int *offset_host, const int *new_offset_host, const float *xyz,
                               const int *offset, const int *new_offset, int *idx, void *workspace, size_t workspace_bytes,
                               void *stream);

/* ---- occupancy loss ---------------------------------------------------------------------------------------------
 * What OccupancyLoss.loss_voxel (loss/occupancy_loss.py:104-149) computes for the shipped configs (no focal, dice or
 * sem/geo-scal terms), forward and backward, with no host synchronisation:
 *   loss = (1/L) sum_layers (ce_weight * CE + lovasz_weight * Lovasz), over the voxels kept by mask (GF_OCC_MASK) and, with
 *   GF_OCC_IGNORE_EMPTY, label != empty_label.
 *   CE: sum w[y] (-log softmax(x)[y]) / sum w[y] over kept voxels with y != ignore_index; GF_OCC_PROB: -log(clamp(p, 1e-6,
 *       1 - 1e-6)) on the input (gradient only where 1e-6 <= p <= 1 - 1e-6).  All kept voxels ignored: 0/0 = NaN.
 *   Lovasz-softmax on p (softmax of x, or the input with GF_OCC_PROB) over the kept voxels, without those labelled lovasz_ignore
 *       (GF_OCC_LOVASZ_IGNORE); voxels labelled ignore_index stay in, as background of every class (as the reference).  Per
 *       present class: errors |fg - p_c| sorted descending, ties to the LOWER voxel index (this op's own rule), dotted with
 *       lovasz_grad; mean over present classes, 0 if none.  d|.|/dp = 0 at 0.
 *   A non-finite input on a voxel that enters a term, or a label outside [0, C) other than ignore_index: loss = NaN.
 * The loss is bitwise reproducible (no float atomics).  GF_OCC_NO_LOVASZ: the CE term alone (no sort).
 *   pred        L device pointers (a HOST array), fp32, element (c, n) at pred[l][c * stride_c + n * stride_n]
 *   label       int64 [N]; mask uint8/bool [N] (GF_OCC_MASK); class_weights f32 [C]; C = 18; 1 <= L <= GF_OCC_MAX_LAYERS
 *   loss        f32 scalar (device)
 *   workspace   gf_occ_loss_workspace_bytes(L, N, C, flags) bytes; the backward reads what the forward left there
 *   scratch     gf_occ_loss_scratch_bytes(L, N, C, flags) bytes, the forward's alone (sort keys, histograms, partials): free
 *               once the forward has run
 *   grad_loss   f32 scalar (device); grad_pred: L device pointers (HOST array) in pred's layout, every element written */
#define GF_OCC_PROB 1
#define GF_OCC_MASK 2
#define GF_OCC_LOVASZ_IGNORE 4
#define GF_OCC_IGNORE_EMPTY 8
#define GF_OCC_NO_LOVASZ 16 /* CE only (use_lovasz_loss=False): no Lovász voxels, no sort; non-finite checks on CE voxels only */
#define GF_OCC_SCAL 32      /* the scene-class affinity terms: gf_occ_loss_scal_* only (below); the size queries honour it */
#define GF_OCC_MAX_LAYERS 8
size_t gf_occ_loss_workspace_bytes(int L, int N, int C, int flags);
size_t gf_occ_loss_scratch_bytes(int L, int N, int C, int flags);
int gf_occ_loss_forward(int L, int N, int C, int flags, const float *const *pred, long long stride_c, long long stride_n,
                        const long long *label, const unsigned char *mask, const float *class_weights, float ce_weight,
                        float lovasz_weight, int lovasz_ignore, int ignore_index, int empty_label, float *loss, void *workspace,
                        size_t workspace_bytes, void *scratch, size_t scratch_bytes, void *stream);
int gf_occ_loss_backward(int L, int N, int C, int flags, const float *const *pred, long long stride_c, long long stride_n,
                         const long long *label, const unsigned char *mask, const float *class_weights, float ce_weight,
                         float lovasz_weight, int lovasz_ignore, int ignore_index, int empty_label, const float *grad_loss,
                         float *const *grad_pred, void *workspace, size_t workspace_bytes, void *stream);
/* The same loss with the scene-class affinity terms of MonoScene / SurroundOcc (sem_scal_loss, geo_scal_loss of
 * loss/occupancy_loss.py:185-268; use_sem_geo_scal_loss=True):
 *   loss = (1/L) sum_layers (ce_weight * CE + lovasz_weight * Lovasz + sem_scal_weight * sem + geo_scal_weight * geo)
 * V = the kept voxels with label != ignore_index and a label in [0, C) (the CE's voxels); p as for the Lovasz term.  Per layer
 * S_c = sum_V p_c, N_c = sum_{V, y = c} p_c (summed in double in a fixed order, each rounded to fp32 once), T_c = #{V, y = c};
 * every ratio below and f are then evaluated in fp32, eps = 1e-5.
 *   f(x) = binary_cross_entropy_with_logits(inverse_sigmoid(x), 1): while x >= float(1 - 1e-5): x -= 1e-5f; while x < 1e-5f:
 *       x += 1e-5f; f = softplus(log(1/x - 1)), f' = -1/x at the shifted x.  Each loop is cut off after 8 steps; a ratio still
 *       out of range then (inputs that are no probabilities, GF_OCC_PROB only) makes the loss NaN where the reference loops on.
 *   sem = (1/count) sum over the classes i in [0, C-1) with T_i > 0 (count of them) of
 *       f(N_i / (S_i + eps)) [if S_i > 0] + f(N_i / (T_i + eps)) + f(((|V| - T_i) - (S_i - N_i)) / ((|V| - T_i) + eps)) [if |V| > T_i];
 *       count == 0 (the reference divides by zero): the loss is NaN.
 *   geo, with e = empty_label (must lie in [0, C)) and I = (|V| - T_e) - (S_e - N_e):
 *       f(I / ((|V| - S_e) + eps)) + f(I / ((|V| - T_e) + eps)) + f(N_e / (T_e + eps)), without guards, as the reference.
 * The gradient in p-space is a_c + b_c [y = c] on the voxels of V, through the softmax Jacobian unless GF_OCC_PROB.
 * flags must hold GF_OCC_SCAL, and workspace and scratch the sizes the queries give with it; every other argument as above. */
int gf_occ_loss_scal_forward(int L, int N, int C, int flags, const float *const *pred, long long stride_c, long long stride_n,
                             const long long *label, const unsigned char *mask, const float *class_weights, float ce_weight,
                             float lovasz_weight, float sem_scal_weight, float geo_scal_weight, int lovasz_ignore,
                             int ignore_index, int empty_label, float *loss, void *workspace, size_t workspace_bytes,
                             void *scratch, size_t scratch_bytes, void *stream);
int gf_occ_loss_scal_backward(int L, int N, int C, int flags, const float *const *pred, long long stride_c, long long stride_n,
                              const long long *label, const unsigned char *mask, const float *class_weights, float ce_weight,
                              float lovasz_weight, float sem_scal_weight, float geo_scal_weight, int lovasz_ignore,
                              int ignore_index, int empty_label, const float *grad_loss, float *const *grad_pred,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ---- evaluation metric -------------------------------------------------------------------------------------------
 * One frame of MeanIoU._after_step (misc/metric_util.py:35-66) -- the call eval.py:163, train.py:317 and visualize.py:205 make
 * after the head -- added to running totals on the device, with no host read: two launches, a counting
 * pass and a finish pass, instead of two boolean-index compactions, 51 torch.sum(...).item() round trips and, with
 * filter_minmax, two nonzero() calls.  Per voxel n, in the reference's order:
 *   target' = empty_label where target == dataset_empty_label (GF_MIOU_REMAP, :43)
 *   GF_MIOU_FILTER_MINMAX (:44-48): z = n % D; min_z / max_z = the lowest / highest z at which ANY voxel, masked or not, has
 *       target' != empty_label; a prediction at z outside [min_z, max_z] counts as empty_label (the caller's tensor is not
 *       written).  No such voxel (the reference raises there): the frame is counted unfiltered and status[1] goes up by one.
 *   kept = mask[n] != 0, every voxel without a mask (:49-55)
 *   over the kept voxels, for i < num_classes and c = class_indices_host[i] (:57-61):
 *       totals[0][i] += #(target' == c)   totals[1][i] += #(target' == c and prediction == c)   totals[2][i] += #(prediction == c)
 *   and at i = num_classes the same three with "!= empty_label" for "== c" (:63-66).
 * Label values of any size are compared as they are (255 occurs in the data); only the class indices must lie in [0, 32).
 *   outputs     int64 [N] (gf_miou_step), or formed per voxel by gf_head_labels' rule from logits f32 [N,18], bin_logits
 *               f32 [N] (prob modes, else NULL), mode (GF_LABELS_*) and threshold (gf_miou_step_logits; model/head/
 *               gaussian_head.py:164-185): the same totals as gf_head_labels followed by gf_miou_step, no labels written
 *   targets     int64 [N], or uint8 [N] with GF_MIOU_TARGETS_U8;  mask uint8/bool [N] or NULL
 *   class_indices_host   HOST int[num_classes], 1 <= num_classes <= GF_MIOU_MAX_CLASSES
 *   totals      int64 [3][num_classes + 1] (seen, correct, positive), ADDED to;  status int64 [2]: [0] += 1 per call
 *   workspace   gf_miou_workspace_size(N, D, flags) bytes (0: sizes refused); nothing in it needs to be zero or kept
 * D is read with GF_MIOU_FILTER_MINMAX only (1 <= D <= GF_MIOU_MAX_D, N a multiple of D).  N == 0 counts a frame.
 * (The size query is ..._size, not ..._bytes: tests/golden/workspace_bytes.json records every ..._bytes query and is not
 * extended by this op; tests/test_miou.py pins its sizes.) */
#define GF_MIOU_TARGETS_U8 1
#define GF_MIOU_FILTER_MINMAX 2
#define GF_MIOU_REMAP 4
#define GF_MIOU_MAX_CLASSES 32
#define GF_MIOU_MAX_D 64
size_t gf_miou_workspace_size(long long N, int D, int flags);
int gf_miou_step(long long N, int D, int flags, const long long *outputs, const void *targets, const unsigned char *mask,
                 int num_classes, const int *class_indices_host, int empty_label, int dataset_empty_label, long long *totals,
                 long long *status, void *workspace, size_t workspace_bytes, void *stream);
int gf_miou_step_logits(long long N, int D, int flags, int C, int mode, const float *logits, const float *bin_logits,
                        float threshold, const void *targets, const unsigned char *mask, int num_classes,
                        const int *class_indices_host, int empty_label, int dataset_empty_label, long long *totals,
                        long long *status, void *workspace, size_t workspace_bytes, void *stream);

/* ---- GaussianLifterV2's pixel lifting and PixelDistributionLoss ----------------------------------------------------
 * gf_lift_pixels replaces the per-frame pixel work of GaussianLifterV2.forward from the pixel logits to the FPS call
 * (model/lifter/gaussian_lifter_v2.py:169-233 with model/utils/sampler.py:9-37), DESIGN.md §3.10.  Per batch element
 * bi, camera c, pixel (i, j) (q = (c h + i) w + j) and depth bin k < S:
 *   u = (j + 0.5f) / w * image_wh[bi][c][0], v = (i + 0.5f) / h * image_wh[bi][c][1] (fp32, in this order);
 *   point_k = (img2lidar[bi][c] @ (u d_k, v d_k, d_k, 1))[:3], d = depth_bins;
 *   pdf = softmax(logits[bi][q][0..S]); disabled = argmax(pdf) == S (ties to the lower index);
 *   sample j < a: stochastic (uniforms given): index = #{k : cdf_k <= uniforms[bi][q][j]} clipped to S, cdf = cumsum(pdf /
 *   (FLT_EPSILON + sum pdf)); deterministic (uniforms NULL): the j-th largest pdf entry, ties to the lower index.
 *   The candidate of slot q a + j is point_min(index, S-1) when the pixel is not disabled and pc_min <= point < pc_max on
 *   every axis.  points[bi][0 .. counts[bi]) are the candidates in slot order; src[bi][.] their slots; the rest of the
 *   [n h w a] rows holds 0 (points) and -1 (src).
 *   pixel_gt[bi][q][k] = in range(point_k) && occ[bi][ix][iy][iz], i* = trunc((p - pc_min) / voxel_size) clamped to the
 *   grid; pixel_gt[bi][q][S] = no k set.
 *   logits      f32 [b][n h w][S + 1];  img2lidar f32 [b][n][4][4];  image_wh f32 [b][n][2];  depth_bins f32 [S]
 *   pc_range_host   HOST float[6] (x, y, z min, x, y, z max)
 *   occ         uint8 [b][X][Y][Z], (label != empty) & cam_mask, needed with pixel_gt only
 *   uniforms    f32 [b][n h w][a] or NULL (deterministic)
 *   points      f32 [b][n h w a][3], counts int [b], src int [b][n h w a] (or NULL): points and counts both or neither
 *   pixel_gt    uint8 [b][n h w][S + 1] or NULL
 *   workspace   gf_lift_workspace_bytes(b, n h w, a) bytes
 * Limits: S + 1 <= GF_LIFT_MAX_BINS (four entries per lane of a 64-lane wave), 1 <= a <= GF_LIFT_MAX_ANCHORS; every check
 * runs before any HIP call.  No float atomics: the outputs are bitwise reproducible.
 *
 * gf_pixel_loss_forward / _backward: PixelDistributionLoss.loss_voxel (loss/bce_loss.py:60-87) without its weight:
 *   p = softmax over each row of `bins` (GF_PIXEL_LOSS_SOFTMAX) or sigmoid (GF_PIXEL_LOSS_SIGMOID) in fp32;
 *   loss = mean over rows x bins of -(t max(log p, -100) + (1 - t) max(log1p(-p), -100)), t = pixel_gt != 0 (torch's
 *   binary_cross_entropy), summed in a fixed order (bitwise reproducible);
 *   backward: d/dp = grad_loss (p - t) / max((1 - p) p, 1e-12f) / (rows bins) (torch's BCE backward), then through the
 *   softmax (p (g - sum g p)) or the sigmoid (g (1 - p) p).  Every element of grad_logits is written.
 *   workspace   gf_pixel_loss_workspace_bytes(rows, bins) bytes (the forward's partials) */
#define GF_LIFT_MAX_BINS 256
#define GF_LIFT_MAX_ANCHORS 8
#define GF_PIXEL_LOSS_SOFTMAX 1
#define GF_PIXEL_LOSS_SIGMOID 2
size_t gf_lift_workspace_bytes(int b, int npix, int a);
int gf_lift_pixels(int b, int n, int h, int w, int S, int a, const float *logits, const float *img2lidar,
                   const float *image_wh, const float *depth_bins, const float *pc_range_host, float voxel_size, int X, int Y,
                   int Z, const unsigned char *occ, const float *uniforms, float *points, int *counts, int *src,
                   unsigned char *pixel_gt, void *workspace, size_t workspace_bytes, void *stream);
size_t gf_pixel_loss_workspace_bytes(int rows, int bins);
int gf_pixel_loss_forward(int rows, int bins, int flags, const float *logits, const unsigned char *pixel_gt, float *loss,
                          void *workspace, size_t workspace_bytes, void *stream);
int gf_pixel_loss_backward(int rows, int bins, int flags, const float *logits, const unsigned char *pixel_gt,
                           const float *grad_loss, float *grad_logits, void *stream);

/* ---- modulated deformable convolution (DCNv2) -----------------------------------------------------------------------
 * Replaces mmcv's modulated_deform_conv2d / ModulatedDeformConv2dPack (registered as 'DCNv2'; the reference's ResNet-101
 * backbone with stage_with_dcn=(False, False, True, True) in every config), DESIGN.md §3.11.  Per output pixel (ho, wo), deform
 * group g, tap k = i kw + j and input channel c of group g (c / (Cin / dg) == g):
 *   dy = offset[n][g 2 kh kw + 2 k][ho][wo], dx = offset[n][g 2 kh kw + 2 k + 1][ho][wo], m = mask[n][g kh kw + k][ho][wo];
 *   y = (ho sh - ph + i dh) + dy, x = (wo sw - pw + j dw) + dx (one fp32 add each);
 *   col = m * bilinear(input[n][c], y, x) when -1 < y < H and -1 < x < W (corners outside the image add 0), else 0;
 *   out[n][co][ho][wo] = sum_{c, k} weight[co][c][i][j] col + bias[co].
 *   Ho = (H + 2 ph - (dh (kh - 1) + 1)) / sh + 1, likewise Wo.
 * Layouts (fp32, contiguous): input [N][Cin][H][W], offset [N][2 dg kh kw][Ho][Wo], mask [N][dg kh kw][Ho][Wo], weight
 * [Co][Cin][kh][kw], bias [Co] or NULL, out / grad_out [N][Co][Ho][Wo]; the gradients have their input's layout.
 * Supported: N >= 0, kh, kw <= GF_DCN_MAX_KERNEL, stride and dilation >= 1, padding >= 0, groups == 1, Cin / dg and Co
 * multiples of GF_DCN_CHANNEL_GRANULE; anything else returns GF_EINVAL before any HIP call.
 *   workspace   gf_dcn_workspace_bytes(..., backward) bytes (0: unsupported shape); forward: a channels-last copy of the input
 *               and a re-laid weight; backward adds a channels-last grad_input accumulator and the weight-gradient partials
 *               (at most 16 copies of the weight): forward 36 / 26 MB, backward 88 / 61 MB at layer3 [6, 256, 54, 100] / layer4 [6, 512, 27, 50]
 * gf_dcn_backward: each gradient pointer may be NULL (not wanted).  grad_input is summed with fp32 atomics and is not bitwise
 * reproducible; the forward, grad_offset, grad_mask, grad_weight and grad_bias are (fixed-order sums).  Offset and mask
 * gradients are 0 where the sample is outside the window, and use the one-sided derivative of floor at integer coordinates
 * (mmcv's dmcn_get_coordinate_weight).  No host synchronisation: graph-capturable. */
#define GF_DCN_MAX_KERNEL 7
#define GF_DCN_CHANNEL_GRANULE 32
size_t gf_dcn_workspace_bytes(int N, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                              int groups, int dg, int backward);
int gf_dcn_forward(int N, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups,
                   int dg, const float *input, const float *offset, const float *mask, const float *weight, const float *bias,
                   float *out, void *workspace, size_t workspace_bytes, void *stream);
int gf_dcn_backward(int N, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups,
                    int dg, const float *input, const float *offset, const float *mask, const float *weight, const float *grad_out,
                    float *grad_input, float *grad_offset, float *grad_mask, float *grad_weight, float *grad_bias,
                    void *workspace, size_t workspace_bytes, void *stream);

/* ---- the encoder's Gaussian refinement step ---------------------------------------------------------------------------
 * Replaces what SparseGaussian3DRefinementModule.forward (version 1, model/encoder/gaussian_encoder/refine_module.py:72-123)
 * and SparseGaussian3DRefinementModuleV2.forward (version 2, refine_module_v2.py:62-107) do after their MLP, with
 * cartesian / reverse_cartesian (utils.py:26-47) and safe_sigmoid / safe_inverse_sigmoid (model/utils/safe_ops.py): one
 * launch instead of 30-40 torch kernels, DESIGN.md §3.12.  Per row, o = output row (the MLP's result after Scale,
 * D = 10 + opacity + S floats), a = anchor row (Da floats), ss = safe_sigmoid, span / lo from pc_range:
 *   version 1: with GF_REFINE_RESTRICT_XYZ o[i] = (2 ss(o[i]) - 1) unit[i], i < 3 (:72-80; unit = the module's unit_sigmoid);
 *              o[k] += a[k] for k < R (:82-84, refine_manual = 0 .. R - 1); xyz = o[0:3], clamped to [1e-6, 1 - 1e-6] with
 *              GF_REFINE_XYZ_IDENTITY (:86-89); means = (ss(xyz) | xyz) span + lo (:99-104)
 *   version 2: delta_means = (2 ss(o[0:3]) - 1) unit (:65; unit = unit_xyz); original_means = cartesian(a[0:3]) (:66);
 *              xyz = reverse_cartesian(original_means + delta_means) (:67-68: clamp to [1 - 0.9999, 0.9999], log(t / (1 - t));
 *              with GF_REFINE_XYZ_IDENTITY the clamp [1e-6, 1 - 1e-6] alone); means = cartesian(xyz) (:86); R is ignored
 *   both:      anchor_out = (xyz, o[3:6], normalize(o[6:10]) (eps 1e-12), o[10:]); scales = scale_lo + (scale_hi - scale_lo)
 *              ss(o[3:6]); rotations = normalize(o[6:10]); opacities = ss(o[10]) with GF_REFINE_OPACITY (else no column);
 *              semantics = softmax / softplus (threshold 20) / the S columns as they are.
 * A scale_activation other than "sigmoid" is not supported: both reference modules leave the scale unbound there (:106-108,
 * v2 :88-90) and raise.
 *   consts     11 doubles, HOST pointer: pc_range[6], scale_lo, scale_hi, unit[3] (differences are taken in double and
 *              rounded once, as the reference's Python floats are)
 *   output     f32 [n, D]      anchor f32 [n, Da]      anchor_out f32 [n, D]
 *   means, scales f32 [n, 3]; rotations f32 [n, 4]; opacities f32 [n, 0 | 1]; semantics f32 [n, S];
 *   original_means, delta_means f32 [n, 3] (version 2; ignored in version 1)
 * GF_EINVAL before any HIP call: S > 32, D != 10 + opacity + S, Da smaller than the anchor columns read (R; 3 in version 2),
 * unknown version or flags.  fp32 in the reference's operation order; no atomics, bitwise reproducible; no host
 * synchronisation, no workspace: graph-capturable. */
#define GF_REFINE_RESTRICT_XYZ 1   /* version 1: restrict_xyz */
#define GF_REFINE_XYZ_IDENTITY 2   /* xyz_activation is not "sigmoid" */
#define GF_REFINE_OPACITY 4        /* include_opa */
#define GF_REFINE_SEM_SOFTMAX 8    /* semantics_activation "softmax" */
#define GF_REFINE_SEM_SOFTPLUS 16  /* ... "softplus"; neither: the columns as they are */
int gf_refine_forward(int n, int D, int Da, int version, int flags, int R, int S, const double *consts, const float *output,
                      const float *anchor, float *anchor_out, float *means, float *scales, float *rotations, float *opacities,
                      float *semantics, float *original_means, float *delta_means, void *stream);

/* Its gradient, exactly torch autograd's of that composition (a clamp passes the gradient on [min, max], bounds included).
 * The forward's values are recomputed from (output, anchor): no forward result is needed.  Each grad_* of a forward output
 * may be NULL (= zero).  Every element of grad_output [n, D] and grad_anchor [n, Da] is written; grad_anchor is zero beyond
 * the first R (version 1) or 3 (version 2) columns. */
int gf_refine_backward(int n, int D, int Da, int version, int flags, int R, int S, const double *consts, const float *output,
                       const float *anchor, const float *grad_anchor_out, const float *grad_means, const float *grad_scales,
                       const float *grad_rotations, const float *grad_opacities, const float *grad_semantics,
                       const float *grad_original_means, const float *grad_delta_means, float *grad_output, float *grad_anchor,
                       void *stream);

/* The refinement modules' MLP and that tail in one launch, forward only: everything
 * SparseGaussian3DRefinementModule.forward (refine_module.py:70-123) and SparseGaussian3DRefinementModuleV2.forward
 * (refine_module_v2.py:62-107) compute from their three inputs.  Per row, E = 128:
 *   x = instance_feature + anchor_embed                                   (refine_module.py:70, refine_module_v2.py:62)
 *   x = relu(W0 x + b0);  x = relu(W2 x + b2);  x = LN4(x)                layers.0, .2, .4 (the modules' `layers`, :59-62)
 *   x = relu(W5 x + b5);  x = relu(W7 x + b7);  x = LN9(x)                layers.5, .7, .9
 *   o = (W10 x + b10) * scale                                             layers.10 [D, 128], layers.11.scale [D]
 *   (anchor_out, means, scales, rotations, opacities, semantics[, original_means, delta_means]) = the tail above on (o, anchor)
 * LayerNorm: eps 1e-5, biased variance, mean first, affine.  ReLU keeps a NaN.  The tail is gf_refine_forward's code on the
 * same bits: its outputs equal gf_refine_forward(mlp_out, anchor) bit for bit; version, flags, R, S and consts are its.
 *   instance_feature, anchor_embed  f32 [n, 128], 16-byte aligned          anchor f32 [n, Da]
 *   params     HOST table of GF_REFINE_MLP_PARAMS = 15 device pointers, the module's own tensors in state_dict order, in
 *              torch's layout, contiguous f32, each 16-byte aligned:
 *                0 layers.0.weight [128, 128]   1 layers.0.bias [128]     2 layers.2.weight   3 layers.2.bias
 *                4 layers.4.weight [128] (LayerNorm)   5 layers.4.bias    6 layers.5.weight   7 layers.5.bias
 *                8 layers.7.weight   9 layers.7.bias   10 layers.9.weight (LayerNorm)         11 layers.9.bias
 *                12 layers.10.weight [D, 128]   13 layers.10.bias [D]     14 layers.11.scale [D]
 *   mlp_out    f32 [n, D] or NULL (not written): o, the bits the tail consumed
 *   the outputs as gf_refine_forward's
 * The table is read during the call and the weights by the kernel, in place: nothing is cached or re-laid out, nothing is
 * loaded from beyond a tensor, and there is no workspace.
 * GF_EINVAL before any HIP call, the message naming the offending value: everything gf_refine_forward refuses (the same
 * messages), E != 128, a null or misaligned parameter, a null instance_feature, anchor_embed or anchor (or a misaligned one of
 * the first two), a null output.  n == 0 returns GF_OK without a launch and without looking at any pointer.  Exact fp32
 * products (v_mfma_f32_32x32x2_f32), no atomics, bitwise reproducible; a row's result does not depend on n or on the row's
 * position; no host synchronisation, no allocation: graph-capturable. */
#define GF_REFINE_MLP_PARAMS 15
int gf_refine_mlp_forward(int n, int E, int D, int Da, int version, int flags, int R, int S, const double *consts,
                          const float *instance_feature, const float *anchor_embed, const float *anchor,
                          const void *const *params, float *mlp_out,
                          float *anchor_out, float *means, float *scales, float *rotations, float *opacities,
                          float *semantics, float *original_means, float *delta_means, void *stream);

/* The refinement modules' training step: a forward that also keeps what the backward needs, and the backward
 * of the MLP and the tail together.
 *
 * gf_refine_mlp_train_sizes: host code; the bytes of the two caller-allocated regions for n rows (both 0 for n == 0, both
 * monotone in n).  GF_EINVAL for n < 0, a D outside 10 .. 43, a negative Da or a null result pointer.
 *
 * gf_refine_mlp_forward_train: gf_refine_mlp_forward's arguments and refusals, and every output, mlp_out included, has its bits;
 * it also fills `saved` (opaque, 16-byte aligned, at least saved_bytes of the query; GF_EINVAL when null or misaligned,
 * GF_EWORKSPACE when shorter): the four post-ReLU rows, the two LayerNorms' (mean, rstd), the last Linear's result before Scale
 * and o.  The input sum is not saved (the backward forms it again from the two inputs); the value before Scale is (it is not
 * recovered as o / scale: a scale entry may be 0).
 *
 * gf_refine_mlp_backward: the gradients of that forward.  instance_feature, anchor_embed, anchor, params, version, flags, R, S
 * and consts as given to the forward, saved as it left it; the eight grad_* of the tail's outputs as gf_refine_backward takes
 * them, each may be NULL (= zero).
 *   grad_x        f32 [n, 128], 16-byte aligned, written in full: the gradient of instance_feature + anchor_embed, which the
 *                 caller gives to both inputs
 *   grad_anchor   f32 [n, Da], written in full; zero beyond the first R (version 1) or 3 (version 2) columns, exactly as
 *                 gf_refine_backward leaves it
 *   grad_mlp_out  f32 [n, D] or NULL: the gradient with respect to o that the MLP's backward consumed, the bits
 *                 gf_refine_backward gives on (mlp_out, anchor, the same output gradients)
 *   grad_params   HOST table of GF_REFINE_MLP_PARAMS device pointers laid out like params, each tensor of its parameter's
 *                 shape; every gradient is STORED, not accumulated (the caller zeroes nothing); a NULL entry is refused
 *   workspace     16-byte aligned scratch of at least workspace_bytes of the query
 * No atomics: every sum over rows runs in a fixed order (per tile of 128 rows and per block of GF_REFINE_MLP_WGRAD_ROWS rows,
 * then one sum over the tiles and blocks), so two calls agree bit for bit; a row of grad_x, grad_anchor and grad_mlp_out does
 * not depend on n or on the row's position.  The rows are walked in chunks of GF_REFINE_MLP_CHUNK_ROWS, one after the other on
 * the stream, so the workspace holds one chunk's intermediate rows.  Nothing is loaded from beyond a tensor; no host
 * synchronisation, no allocation: graph-capturable.  n == 0 returns GF_OK without looking at the data pointers, the 15
 * parameter gradients zero-filled.  GF_EINVAL before any HIP call, the message naming the offending value: everything
 * gf_refine_mlp_forward refuses (the same messages), a null entry of grad_params, a null or misaligned saved, workspace or
 * grad_x, a null grad_anchor; GF_EWORKSPACE for a workspace shorter than the query's. */
#define GF_REFINE_MLP_WGRAD_ROWS 512
#define GF_REFINE_MLP_CHUNK_ROWS 32768
int gf_refine_mlp_train_sizes(int n, int D, int Da, size_t *saved_bytes, size_t *workspace_bytes);
int gf_refine_mlp_forward_train(int n, int E, int D, int Da, int version, int flags, int R, int S, const double *consts,
                                const float *instance_feature, const float *anchor_embed, const float *anchor,
                                const void *const *params, float *mlp_out,
                                float *anchor_out, float *means, float *scales, float *rotations, float *opacities,
                                float *semantics, float *original_means, float *delta_means,
                                void *saved, size_t saved_bytes, void *stream);
int gf_refine_mlp_backward(int n, int E, int D, int Da, int version, int flags, int R, int S, const double *consts,
                           const float *instance_feature, const float *anchor_embed, const float *anchor,
                           const void *const *params, const void *saved,
                           const float *grad_anchor_out, const float *grad_means, const float *grad_scales,
                           const float *grad_rotations, const float *grad_opacities, const float *grad_semantics,
                           const float *grad_original_means, const float *grad_delta_means,
                           float *grad_x, float *grad_anchor, float *grad_mlp_out, void *const *grad_params,
                           void *workspace, size_t workspace_bytes, void *stream);

/* ---- the anchor encoder ---------------------------------------------------------------------------------------------------
 * Replaces SparseGaussian3DEncoder.forward (model/encoder/gaussian_encoder/anchor_encoder_module.py:38-53; its layers are
 * linear_relu_ln(embed_dims, 1, 2, input_dims), utils.py:49-59): one launch instead of about 40 torch kernels, DESIGN.md
 * §3.13.  Per anchor row a (Da floats), E = 128, opa = include_opa != 0, ss = 10 + opa:
 *   branch inputs, in this order: a[0:3] (:39), a[3:6] (:40), a[6:10] (:41), a[10:11] when opa (:42-43), a[ss:ss+S] when
 *              S > 0 (:46-47)
 *   f_b      = LN2(relu(W2 LN1(relu(W1 x_b + b1)) + b2)); LayerNorm over the 128 features, biased variance, eps 1e-5, affine
 *   s        = xyz + scale + rot (+ opacity) (+ semantics), summed left to right (:51)
 *   out      = LN(relu(Wo2 LN(relu(Wo1 s + bo1)) + bo2))  (:52), f32 [n, 128]
 * Columns of a that no branch reads are never loaded: they cannot influence the result, NaN and Inf included.
 *   anchor     f32 [n, Da] (any 4-byte alignment)         out f32 [n, 128], 16-byte aligned (it is written 16 bytes at a time)
 *   params     HOST table of GF_ANCHOR_EMBED_PARAMS = 6 x 8 device pointers, the modules' own tensors in torch's layout,
 *              contiguous f32.  Stage s = 0 .. 5 is xyz_fc, scale_fc, rot_fc, opacity_fc, semantics_fc, output_fc; within a
 *              stage, in state_dict order:
 *                8 s + 0  .0.weight [128, k]  (k = 3, 3, 4, 1, S; 128 for output_fc)      8 s + 1  .0.bias [128]
 *                8 s + 2  .2.weight [128]  (LayerNorm)                                    8 s + 3  .2.bias [128]
 *                8 s + 4  .3.weight [128, 128]                                            8 s + 5  .3.bias [128]
 *                8 s + 6  .5.weight [128]  (LayerNorm)                                    8 s + 7  .5.bias [128]
 *              The eight of an absent branch (opacity_fc without opa, semantics_fc with S = 0) are ignored; pass NULL.
 *              Every pointer but a branch's .0.weight must be 16-byte aligned (torch's allocations are).
 * The table is read during the call and the weights by the kernel, in place: every call uses the parameters' current values,
 * nothing is cached or re-laid out, and there is no workspace.
 * GF_EINVAL before any HIP call: E != 128, S > 32, Da < 10 + opa + S, a null or misaligned parameter of a stage that is
 * present, a misaligned out.  n == 0 returns GF_OK without a launch.  Exact fp32 products (v_mfma_f32_32x32x2_f32), no atomics, bitwise
 * reproducible; a row's result does not depend on n or on the row's position; no host synchronisation, no allocation:
 * graph-capturable. */
#define GF_ANCHOR_EMBED_DIMS 128
#define GF_ANCHOR_EMBED_MAX_S 32
#define GF_ANCHOR_EMBED_PARAMS 48
int gf_anchor_embed_forward(int n, int Da, int E, int include_opa, int S, const float *anchor, const void *const *params,
                            float *out, void *stream);

/* The anchor encoder's training step: a forward that also saves what the backward needs, and the full
 * backward.  E, S, Da, the alignment limits and the 48-pointer params table are gf_anchor_embed_forward's.
 *
 * gf_anchor_embed_train_sizes: host code; the bytes of the two caller-allocated regions for n rows of a module with
 * include_opa and S (both 0 for n == 0).  GF_EINVAL: n < 0, S outside 0 .. 32, a null result pointer.
 *
 * gf_anchor_embed_forward_train: the forward, with out BITWISE gf_anchor_embed_forward's, plus `saved` (16-byte aligned, at
 * least the queried saved_bytes; opaque: every stage's post-ReLU row and LayerNorm (mean, rstd), and the branches' sum).
 *
 * gf_anchor_embed_backward: from grad_out f32 [n, 128] (16-byte aligned), the anchor, the parameters and `saved` of the
 * forward_train call on the same inputs,
 *   grad_anchor  f32 [n, Da], written in full: columns no branch reads (>= 10 + opa + S) are exactly 0.0
 *   grad_params  HOST table of 48 device pointers laid out like params, each tensor of its parameter's shape: every present
 *                parameter's gradient is STORED, not accumulated -- the caller zeroes nothing.  The eight of an absent
 *                branch are ignored.
 *   workspace    16-byte aligned, at least the queried workspace_bytes; scratch, nothing survives the call
 * Three kernels and a fixed-order sum: no atomics, bitwise reproducible; a row of grad_anchor does not depend on n or on the
 * row's position; no host synchronisation, no allocation: graph-capturable.  A read column that is NaN makes that row of
 * grad_anchor and the parameter gradients NaN (as torch's are); unread columns are never loaded.
 * GF_EINVAL as the forward, and for a null gradient of a present stage or a misaligned region; GF_EWORKSPACE for a region
 * shorter than the op's carve.  n == 0 returns GF_OK with the parameter gradients zero-filled.
 * GF_ANCHOR_EMBED_WGRAD_ROWS: the rows one workgroup of the weight-gradient kernel sums (the workspace holds one partial per
 * block of that many rows).  GF_ANCHOR_EMBED_CHUNK_ROWS: the backward walks the rows in chunks of this many, one after the
 * other on the stream, and the workspace holds the per-row intermediates of one chunk only.  Both are exported for tests that
 * place n at their edges. */
#define GF_ANCHOR_EMBED_WGRAD_ROWS 512
#define GF_ANCHOR_EMBED_CHUNK_ROWS 65536
int gf_anchor_embed_train_sizes(int n, int include_opa, int S, size_t *saved_bytes, size_t *workspace_bytes);
int gf_anchor_embed_forward_train(int n, int Da, int E, int include_opa, int S, const float *anchor, const void *const *params,
                                  float *out, void *saved, size_t saved_bytes, void *stream);
int gf_anchor_embed_backward(int n, int Da, int E, int include_opa, int S, const float *anchor, const void *const *params,
                             const void *saved, const float *grad_out, float *grad_anchor, void *const *grad_params,
                             void *workspace, size_t workspace_bytes, void *stream);

/* The encoder's feed-forward block in one launch: AsymmetricFFN.forward
 * (model/encoder/gaussian_encoder/ffn_module.py:66-75) with the "add" and "norm" that follow it in the encoder's
 * operation_order.  For every row x [Cin] of x f32 [n, Cin]:
 *   u   = LN_pre(x)                          if pre_norm is given, else x
 *   y   = W2 relu(W1 u + b1) + b2            W1 = layers.0.0.weight [F, Cin], W2 = layers.1.weight [E, F]
 *   y  += Wid u + bid                        if identity_fc is given (Wid [E, Cin])
 *   y  += residual                           if residual f32 [n, E] is given (added last: zeros change no bit)
 *   out = LN_post(y)                         if the post norm is given, else y;   out f32 [n, E]
 * Both LayerNorms: eps = 1e-5, biased variance, mean first, then the squared deviations.  ReLU keeps a NaN.
 *   params     HOST table of GF_FFN_PARAMS = 10 device pointers, the modules' own tensors in torch's layout, contiguous f32:
 *                0, 1  pre_norm.weight, .bias [Cin]          2, 3  layers.0.0.weight [F, Cin], .bias [F]
 *                4, 5  layers.1.weight [E, F], .bias [E]     6, 7  identity_fc.weight [E, Cin], .bias [E]
 *                8, 9  the post norm's weight, bias [E]
 *              A NULL pair = that part is absent; layers.* must be present.
 * Every pointer is 16-byte aligned; out aliases no input.  Nothing is read beyond x[n Cin] or residual[n E].
 * GF_EINVAL before any HIP call, the message naming the offending value: E != 128, F != 512, Cin not 128 or 256, n < 0, a
 * missing layers.* pointer, a half-present pair, a misaligned pointer.  n == 0 returns GF_OK without a launch.  Exact fp32
 * products (v_mfma_f32_32x32x2_f32), the F-wide hidden row never reaches memory; no workspace, no atomics, bitwise
 * reproducible; a row's result does not depend on n or on the row's position (up to 32 rows per compute unit a workgroup
 * owns 32 rows, beyond that 128: two kernels, the same bits); no host synchronisation, no allocation: graph-capturable. */
#define GF_FFN_PARAMS 10
#define GF_FFN_EMBED_DIMS 128
#define GF_FFN_HIDDEN 512
int gf_ffn_forward(int n, int Cin, int F, int E, const float *x, const void *const *params, const float *residual, float *out,
                   void *stream);

/* The feed-forward block's training step: a forward with the module's two dropouts that also saves what
 * the backward needs, and the full backward.  E, F, Cin, the alignment rules and the 10-pointer params table are
 * gf_ffn_forward's.  Per row:
 *   u   = LN_pre(x)
 *   h   = relu(W1 u + b1);   h' = h * (keep_hidden ? scale_hidden : 0)      keep_hidden u8 [n, 512], nonzero = keep
 *   a   = W2 h' + b2;        a' = a * (keep_out ? scale_out : 0)            keep_out u8 [n, 128]: the bias is dropped with it
 *   y   = a' + (Wid u + bid) + residual;   out = LN_post(y)
 * The masks are the caller's (the op draws nothing) and need no alignment; a NULL mask = no dropout there, its scale is
 * ignored.  A dropout is a product, as nn.Dropout's: a NaN stays a NaN under a dropped entry.
 *
 * gf_ffn_train_sizes: host code; the bytes of the two caller-allocated regions for n rows (both 0 for n == 0, both monotone
 * in n; saved_bytes <= 640 n + 4096).  GF_EINVAL: n < 0, Cin not 128 or 256, a null result pointer.
 *
 * gf_ffn_forward_train: with both masks NULL, and with all-ones masks at scales of 1, out is BITWISE gf_ffn_forward's at
 * every n.  `saved` (16-byte aligned, at least saved_bytes; opaque: the row before the post norm and the two norms' (mean,
 * rstd) -- no [n, 512] array: the backward forms the hidden row again from x by the forward's own chain of MFMAs, so which
 * hidden features are live is the forward's decision bit for bit).
 *
 * gf_ffn_backward: from grad_out f32 [n, 128], x, the parameters, the same masks and scales, and `saved` of the
 * forward_train call on them,
 *   grad_x         f32 [n, Cin], written in full
 *   grad_residual  f32 [n, 128] or NULL: the gradient of y, written in full
 *   grad_params    HOST table of 10 device pointers laid out like params, each tensor of its parameter's shape and 16-byte
 *                  aligned: every present parameter's gradient is STORED, not accumulated -- the caller zeroes nothing
 *   workspace      16-byte aligned, at least workspace_bytes; scratch, nothing survives the call
 * with da = dy * (keep_out ? scale_out : 0), dz = W2^T da * (keep_hidden ? scale_hidden : 0) where h > 0 (or h is NaN, as
 * torch's threshold) and 0 elsewhere.  Three kernels and a fixed-order sum: no atomics, bitwise reproducible; a row of grad_x /
 * grad_residual does not depend on n or on the row's position; no host synchronisation, no allocation: graph-capturable.
 * GF_EINVAL before any HIP call for everything gf_ffn_forward refuses, a misaligned or (n > 0) null region, a scale that is
 * not finite and positive where its mask is given, a null or misaligned gradient of a present parameter; GF_EWORKSPACE for a
 * region shorter than the query says.  n == 0: GF_OK, the parameter gradients zero-filled.
 * GF_FFN_WGRAD_ROWS: the rows one workgroup of the weight-gradient kernel sums (the workspace holds one partial of the three
 * matrices per block of that many rows).  GF_FFN_CHUNK_ROWS: the backward walks the rows in chunks of this many, one after the
 * other on the stream, and the workspace holds the per-row intermediates of one chunk only. */
#define GF_FFN_WGRAD_ROWS 512
#define GF_FFN_CHUNK_ROWS 32768
int gf_ffn_train_sizes(int n, int Cin, size_t *saved_bytes, size_t *workspace_bytes);
int gf_ffn_forward_train(int n, int Cin, int F, int E, const float *x, const void *const *params, const float *residual,
                         const unsigned char *keep_hidden, float scale_hidden, const unsigned char *keep_out, float scale_out,
                         float *out, void *saved, size_t saved_bytes, void *stream);
int gf_ffn_backward(int n, int Cin, int F, int E, const float *x, const void *const *params, const unsigned char *keep_hidden,
                    float scale_hidden, const unsigned char *keep_out, float scale_out, const void *saved, const float *grad_out,
                    float *grad_x, float *grad_residual, void *const *grad_params, void *workspace, size_t workspace_bytes,
                    void *stream);

/* The dense front of the deformable block in one launch: the two Linear layers that
 * DeformableFeatureAggregation.forward applies to the instance feature before the sampling -- kps_generator.learnable_fc
 * (model/encoder/gaussian_encoder/deformable_module.py:59-63) and weights_fc on instance_feature + anchor_embed (:250-262).
 * For every row f [E] of feature f32 [n, E] and e [E] of embed f32 [n, E]:
 *   learned = Wl f + bl              Wl = kps_generator.learnable_fc.weight [K3, E], K3 = 3 K    (f, not f + e)
 *   raw     = Ww (f + e) + bw        Ww = weights_fc.weight [Nw, E]
 * embed may be NULL: raw = Ww f + bw.  K3 = 0: no learnable_fc, learned is not written (and may be NULL).
 *   learned    f32 [n, K3]: gf_key_points' learned [n, K, 3]
 *   raw        f32 [n, Nw]: gf_daf_fused_forward's raw_anchor [n, L, pts, G] (use_camera_embed) or raw_weights
 *              [n, cams, L, pts, G] -- the reference's own column orders
 *   params     HOST table of GF_DEFORM_LOGITS_PARAMS = 4 device pointers, the modules' own tensors in torch's layout,
 *              contiguous f32:  0, 1  learnable_fc.weight [K3, E], .bias [K3] (not read when K3 = 0)
 *                               2, 3  weights_fc.weight [Nw, E], .bias [Nw]
 * The contract is gf_ffn_forward's: every pointer is 16-byte aligned; the outputs alias no input and not each other; nothing
 * is read beyond feature[n E] or embed[n E], nothing written beyond learned[n K3] or raw[n Nw].  GF_EINVAL before any HIP
 * call, the message naming the offending value: E != 128, K3 outside 0 .. GF_DEFORM_MAX_LEARNED, Nw < 4 or not a multiple of
 * 4 (no upper bound), n < 0, a missing or misaligned pointer, an output that aliases an input.  n == 0 returns GF_OK without a
 * launch.  Exact fp32 products (v_mfma_f32_32x32x2_f32); f + e is formed in registers and never reaches memory; no workspace,
 * no atomics, bitwise reproducible; a NaN stays in its row; a row's result does not depend on n or on the row's position (up
 * to 32 rows per compute unit a workgroup owns 32 rows, beyond that 128: two kernels, the same bits); no host
 * synchronisation, no allocation: graph-capturable. */
#define GF_DEFORM_EMBED_DIMS 128
#define GF_DEFORM_MAX_LEARNED 32
#define GF_DEFORM_LOGITS_PARAMS 4
int gf_deform_logits_forward(int n, int E, int K3, int Nw, const float *feature, const float *embed, const void *const *params,
                             float *learned, float *raw, void *stream);

/* The dense back of the deformable block in one launch: output_proj and the residual of
 * DeformableFeatureAggregation.forward (model/encoder/gaussian_encoder/deformable_module.py:243-248, proj_drop not applied:
 * eval semantics), and the "add", "norm" that follow the block in the prob configs' operation_order.  For every row x [E] of
 * features f32 [n, E] (gf_daf_fused_forward's output) and f [E] of instance_feature f32 [n, E]:
 *   y   = Wo x + bo                  Wo = output_proj.weight [E, E]
 *   out = y                          mode GF_DEFORM_NONE   out f32 [n, E]     (instance_feature is not read, may be NULL)
 *         y + f                      mode GF_DEFORM_ADD    out f32 [n, E]
 *         [y | f]                    mode GF_DEFORM_CAT    out f32 [n, 2 E]   (the right half is f bit for bit)
 *   out = LN(out + residual)         GF_DEFORM_NONE / GF_DEFORM_ADD only: + residual f32 [n, E] where given (added last:
 *                                    zeros change no bit), then the post norm where given (gf_ffn_forward's LayerNorm: eps =
 *                                    1e-5, biased variance, mean first, then the squared deviations)
 *   params     HOST table of GF_DEFORM_OUTPUT_PARAMS = 4 device pointers, torch's layout, contiguous f32:
 *                0, 1  output_proj.weight [E, E], .bias [E]      2, 3  the post norm's weight, bias [E] (a NULL pair: absent)
 * The contract is gf_ffn_forward's: every pointer is 16-byte aligned; out aliases no input; nothing is read beyond n E of an
 * input, nothing written beyond out[n E] (out[2 n E] with GF_DEFORM_CAT).  GF_EINVAL before any HIP call, the message naming
 * the offending value: E != 128, an unknown mode, n < 0, a missing output_proj pointer, a half-present norm pair, a post norm
 * or a residual with GF_DEFORM_CAT, a misaligned pointer, an out that aliases an input.  n == 0 returns GF_OK without a
 * launch.  Exact fp32 products, no workspace, no atomics, bitwise reproducible; a NaN stays in its row; a row's result does
 * not depend on n or on the row's position (two kernels as above, the same bits); no host synchronisation, no allocation:
 * graph-capturable. */
#define GF_DEFORM_OUTPUT_PARAMS 4
#define GF_DEFORM_NONE 0
#define GF_DEFORM_ADD 1
#define GF_DEFORM_CAT 2
int gf_deform_output_forward(int n, int E, int mode, const float *features, const float *instance_feature,
                             const void *const *params, const float *residual, float *out, void *stream);

/* The training step of the dense back: a forward that also saves what the backward needs, and the full
 * backward.  The modes, the 4-pointer params table, E == 128 and the alignment and aliasing rules are
 * gf_deform_output_forward's; proj_drop is not part of the op.
 *
 * gf_deform_output_train_sizes: host code; the bytes of the two caller-allocated regions for n rows (both 0 for n == 0, both
 * monotone in n).  with_norm: whether the call has a post norm.  saved_bytes is 0 without one (the op is linear then: its
 * backward needs features and Wo only), otherwise <= 520 n + 4096: the row the norm reads and its (mean, rstd).  The
 * workspace holds one partial of dWo per block of GF_DEFORM_OUTPUT_WGRAD_ROWS rows, one partial of the vector gradients per
 * tile of 128 rows (four a block) and, with a post norm, the [n, E] gradient before the norm.  GF_EINVAL: E != 128, an unknown
 * mode, a post norm with GF_DEFORM_CAT, n < 0, a null result pointer.
 *
 * gf_deform_output_forward_train: out is BITWISE gf_deform_output_forward's at every n and in every variant.  `saved`
 * (16-byte aligned, at least saved_bytes, opaque) is written with a post norm only and may be NULL without one.
 *
 * gf_deform_output_backward: from grad_out f32 [n, E] ([n, 2 E] with GF_DEFORM_CAT), features, the parameters and `saved` of
 * the forward_train call on them; g_s = the post norm's data backward of grad_out (grad_out itself without a norm), g_y = g_s
 * (the left half of grad_out with GF_DEFORM_CAT):
 *   grad_features  f32 [n, E]          Wo^T g_y, written in full
 *   grad_instance  f32 [n, E] or NULL  g_s with GF_DEFORM_ADD; the right half of grad_out bit for bit with GF_DEFORM_CAT;
 *                                      must be NULL with GF_DEFORM_NONE
 *   grad_residual  f32 [n, E] or NULL  g_s (not with GF_DEFORM_CAT)
 *   grad_params    HOST table of 4 device pointers laid out like params: dWo = sum g_y x^T, dbo = sum g_y, d(norm weight) =
 *                  sum grad_out x^, d(norm bias) = sum grad_out -- each STORED, never accumulated; a NULL slot is skipped
 *   workspace      16-byte aligned, at least workspace_bytes; scratch, nothing survives the call
 * Three kernels -- the data backward, the weight gradient on the matrix cores per block of rows, one fixed-order sum of the
 * partials -- no atomics, bitwise reproducible; a row of the three per-row outputs does not depend on n or on the row's
 * position; exact fp32 products; no host synchronisation, no allocation: graph-capturable.  GF_EINVAL before any HIP call, the
 * message naming the offending value, for everything gf_deform_output_forward refuses, a null or misaligned saved region or
 * workspace where one is needed, a gradient slot that is misaligned, grad_instance with GF_DEFORM_NONE, grad_residual with
 * GF_DEFORM_CAT, an output that aliases an input, the saved region, the workspace or another output; GF_EWORKSPACE for a
 * region shorter than the query says.  n == 0: GF_OK, the parameter gradients zero-filled. */
#define GF_DEFORM_OUTPUT_WGRAD_ROWS 512
int gf_deform_output_train_sizes(int n, int E, int mode, int with_norm, size_t *saved_bytes, size_t *workspace_bytes);
int gf_deform_output_forward_train(int n, int E, int mode, const float *features, const float *instance_feature,
                                   const void *const *params, const float *residual, float *out, void *saved, size_t saved_bytes,
                                   void *stream);
int gf_deform_output_backward(int n, int E, int mode, const float *features, const void *const *params, const void *saved,
                              const float *grad_out, float *grad_features, float *grad_instance, float *grad_residual,
                              void *const *grad_params, void *workspace, size_t workspace_bytes, void *stream);

/* The training step of the dense front.  The op is linear, so nothing is saved: the forward of the
 * training step IS gf_deform_logits_forward.  Here are its backward and the size query; K3, Nw, E == 128, the 4-pointer params
 * table and embed == NULL are the forward's.
 *
 * gf_deform_logits_train_sizes: host code.  saved_bytes is always 0 (kept so that the one size-query shape serves this op
 * too); workspace_bytes holds one partial of dWw and dWl per block of GF_DEFORM_LOGITS_WGRAD_ROWS rows ((Nw + 32) x 128
 * floats, Nw x 128 with K3 = 0) and one partial of the bias gradients per tile of 128 rows; 0 for n == 0, monotone in n and Nw.
 * GF_EINVAL: E != 128, K3 or Nw outside the forward's, n < 0, a null result pointer.
 *
 * gf_deform_logits_backward: with g_l = grad_learned f32 [n, K3] and g_r = grad_raw f32 [n, Nw], either NULL for a zero
 * cotangent (its weight and bias gradients, where asked for, are stored as zeros, its term is left out of the data chain):
 *   grad_embed    f32 [n, E] or NULL   g_r Ww = (G0 + G1) + .., Gq the accumulator chain of raw's columns 128 q .. 128 q + 127
 *   grad_feature  f32 [n, E] or NULL   g_r Ww + g_l Wl in ONE fixed order: ((G0 + G1) + ..) + L, L the learned columns'
 *                                      chain -- bitwise grad_embed where g_l is NULL or K3 = 0; written in full whenever given
 *   grad_params   HOST table of 4 device pointers laid out like params: dWl = g_l^T f [K3, E], dbl = sum over rows of g_l,
 *                 dWw = g_r^T (f + e) [Nw, E] with the sum formed in registers as the forward forms it, dbw = sum over rows of
 *                 g_r -- each STORED, never accumulated; a NULL slot is a gradient nobody asked for and is skipped
 *   workspace     16-byte aligned, at least workspace_bytes, needed when n > 0 and a parameter gradient is asked for; scratch
 * Three kernels -- the data backward with the per-tile bias partials (column sums in double), the weight gradients on the
 * matrix cores per block of rows and group of 128 gradient columns, one fixed-order sum of the partials -- no atomics,
 * bitwise reproducible; a row of grad_feature / grad_embed does not depend on n or on the row's position; a NaN in a row of
 * a cotangent or of feature stays out of every other row's data gradients; exact fp32 products; no host synchronisation, no
 * allocation: graph-capturable.
 * Every pointer is 16-byte aligned, grad_learned and the gradients of learnable_fc only 4 (a row of K3 floats).  GF_EINVAL
 * before any HIP call, the message naming the offending value: everything gf_deform_logits_forward refuses of the sizes and
 * the table, grad_learned with K3 = 0, a gradient slot for a parameter that is absent, a misaligned pointer, a null or
 * misaligned workspace where one is needed, an output that aliases an input, the workspace or an earlier output;
 * GF_EWORKSPACE for a workspace shorter than the query says.  n == 0: GF_OK, the parameter gradients asked for zero-filled. */
#define GF_DEFORM_LOGITS_WGRAD_ROWS 512
int gf_deform_logits_train_sizes(int n, int E, int K3, int Nw, size_t *saved_bytes, size_t *workspace_bytes);
int gf_deform_logits_backward(int n, int E, int K3, int Nw, const float *feature, const float *embed, const void *const *params,
                              const float *grad_learned, const float *grad_raw, float *grad_feature, float *grad_embed,
                              void *const *grad_params, void *workspace, size_t workspace_bytes, void *stream);

/* Time only every `every`-th dominant-kernel launch (default 1): the two event records cost a few
 * microseconds of stream time each, so sampling keeps the timed region close to the un-instrumented one. */
int gf_profile_stride(int every);
int gf_profile_read(float *ms_out, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* GF_HIP_H_INCLUDED */
