/*
 * idh_geometry.h — surface normals from depth (added without an ABI version change: nothing existing moved; this surface is versioned
 * through the struct_size of its argument structs).
 *
 * The reference estimates normals with NormalGenerator (utils/geometry_utils.py:92-138): kornia.filters.gaussian_blur2d of the depth,
 * BackprojectDepth (:55-63), kornia.filters.spatial_gradient of the 3-D points, torch.cross and F.normalize - four or five launches with
 * full-size temporaries.  Two entry points replace it:
 *
 *   idh_depth_normals_fwd   the dense form, one launch from a depth map to (B,3,H,W) normals      utils/geometry_utils.py:121-138
 *   idh_patch_normals_fwd   steps 3-4 (:129-138) at the centre of given 3x3 patches of points: the sparse form for hit tests
 *
 * Contract of idh_depth_normals_fwd (kornia 0.6.7 as called at :121-138, restated from the library's documented definition):
 *   1. blur     separable Gaussian, weights g[i] = exp(-(i - k/2)^2 / (2 s^2)) / sum in fp32, horizontal pass first, then vertical, each with
 *               `reflect` padding (index -1 -> 1, index H -> H - 2).  k = 1 is the identity and does no arithmetic.
 *   2. points   p = d_smooth * (invK[:3,:3] @ (x + 0.5, y + 0.5, 1)), each row of the product summed left to right.
 *   3. gradient the normalised Sobel pair ([[-1,0,1],[-2,0,2],[-1,0,1]] / 8 and its transpose) as a cross-correlation over the points with
 *               `replicate` padding of 1; all nine taps are multiplied and summed in row-major order, the zero taps included (0 * NaN = NaN).
 *   4. normal   n = cross(gx, gy) / max(||n||, 1e-12).  A fronto-parallel plane gives (0, 0, +1); an all-zero neighbourhood exactly (0, 0, 0).
 * Non-finite depths propagate as IEEE arithmetic propagates them.  fp32 throughout, no fused multiply-add.
 * Options (all off = the reference): `orient` negates the normal where n . p > 0 (p: the pixel's own point), so that it faces the camera;
 * `world_R_cam_b33` rotates the (oriented) normal, rows summed left to right; `flags_b1hw` + `need` mark the trustworthy depths: a pixel is
 * valid iff every depth its normal read - the (2 (k/2) + 3)^2 footprint under the two border maps - has flags == need; invalid pixels store
 * (0, 0, 0) and valid_b1hw holds 1 / 0.
 *
 * Conventions of include/idh.h: device pointers, dense tensors, caller-owned outputs, `stream` a hipStream_t, asynchronous, no allocation, no
 * synchronisation, no workspace, IDH_OK or a negative IDH_E* code.  Arguments are validated on the host before anything is launched.
 */
#ifndef IDH_GEOMETRY_H_
#define IDH_GEOMETRY_H_

#include <stddef.h>
#include <stdint.h>

#include "idh.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* Host struct, read during the call.  struct_size = sizeof(idh_normals_args) of the caller's header (must be >= the library's). */
typedef struct idh_normals_args {
    int64_t struct_size;
    const float *depth_b1hw;      /* (B,1,H,W) */
    const float *invK_b44;        /* (B,4,4); only [:3,:3] is read (:60) */
    const float *world_R_cam_b33; /* (B,3,3) rotation applied to the stored normal, or NULL */
    const uint8_t *flags_b1hw;    /* (B,1,H,W) or NULL: depths with flags != need are not to be trusted */
    float *normals_b3hw;          /* (B,3,H,W) */
    uint8_t *valid_b1hw;          /* (B,1,H,W) 1 / 0; required with flags_b1hw, ignored (may be NULL) without */
    float smoothing_std;          /* s > 0 (:110) */
    int32_t kernel_size;          /* k in {1, 3, 5, 7} (:109) */
    int32_t orient;               /* 1: the normal faces the camera */
    int32_t need;                 /* flags value of a trustworthy depth */
    int32_t B, H, W;
} idh_normals_args;

/* Host struct, read during the call.  struct_size as above. */
typedef struct idh_patch_normals_args {
    int64_t struct_size;
    const float *points_bn93;    /* (B,N,9,3): a 3x3 patch of points per query, row-major (index 4 is the centre) */
    const float *cam_centre_b3;  /* (B,3) the camera centre in the points' frame; required with orient, else may be NULL */
    const uint8_t *flags_bn9;    /* (B,N,9) or NULL */
    float *normals_bn3;          /* (B,N,3) */
    uint8_t *valid_bn;           /* (B,N) 1 / 0; required with flags_bn9 */
    int32_t orient;              /* 1: negate where n . (centre point - cam_centre) > 0 */
    int32_t need;
    int32_t B, N;
} idh_patch_normals_args;

/* sizeof of the two structs as compiled into the library (bindings assert their mirrors match). */
size_t idh_sizeof_normals_args(void);
size_t idh_sizeof_patch_normals_args(void);

/* utils/geometry_utils.py:121-138 (NormalGenerator.forward; BackprojectDepth :55-63 inside it) for B depth maps, in one launch.
 * IDH_EINVAL: args NULL, struct_size short, depth / invK / normals NULL, kernel_size not in {1,3,5,7}, smoothing_std <= 0 (or NaN),
 * H or W <= kernel_size / 2 (reflect padding is undefined there), B < 0, flags_b1hw without valid_b1hw;
 * IDH_EUNSUPPORTED: H * W or the number of tiles of the launch >= 2^31.  B == 0 is IDH_OK without a launch. */
int idh_depth_normals_fwd(const idh_normals_args *args, void *stream);

/* utils/geometry_utils.py:129-138 (spatial_gradient, cross, normalize) at the centre of each 3x3 patch: no padding is involved.  The same
 * device function as the dense kernel: on equal points the two give equal bits.
 * IDH_EINVAL: args NULL, struct_size short, points / normals NULL, B < 0, N < 0, flags_bn9 without valid_bn, orient without cam_centre_b3;
 * IDH_EUNSUPPORTED: B * N >= 2^31.  B == 0 or N == 0 is IDH_OK without a launch. */
int idh_patch_normals_fwd(const idh_patch_normals_args *args, void *stream);

/* ---- Multi-view depth consistency (csrc/mv_consistency.hip) -------------------------------------------------------
 *
 * A depth map is checked against K source depth maps of other cameras: per pixel and source, is the point visible there, does the
 * source agree with it, or does the point float in space the source saw through.  The arithmetic is the reference's MVDepthLoss
 * (losses.py:143-261: BackprojectDepth, Project3D, a nearest grid_sample tap, the 1.05 gate, |log - log|), operation by operation, so
 * the same launch also returns that loss's forward value - a quality score of a depth map that needs no ground truth.
 *
 * One launch, one lane per pixel (i, j) of map b, a loop over the sources k = 0 .. K - 1.  fp32; a row of a matrix product is summed
 * left to right with every product after the first fused into the running sum (fmaf), as the BLAS kernels under the reference's
 * matmuls do; nothing else is contracted:
 *   q = invK[b][:3,:3] (j + 0.5, i + 0.5, 1)        q.x = fma(k01, v, k00 u) + k02 ...                  utils/geometry_utils.py:60
 *   cam = d q;   X = world_T_cam[b] (cam, 1)         four components, X.x = fma(e03, 1, fma(e02, c.z, fma(e01, c.y, e00 c.x))) ...  :61, losses.py:165
 *   P = src_K[b,k] src_cam_T_world[b,k]              formed first, each entry fma(k_r3, e_3c, fma(k_r2, e_2c, fma(k_r1, e_1c, k_r0 e_0c)))    :82
 *   c = P[:3] X;   z = max(c.z, 1e-5), a NaN staying a NaN as torch.maximum keeps it;   px = c.x / z,  py = c.y / z          :84-87
 *   tap (rint(py - 0.5), rint(px - 0.5)), round-half-even: the nearest tap of grid_sample(align_corners=False); INSIDE when it is a
 *   pixel of the source; s = src_depth[b,k] there, 0 when not inside (padding zeros)                                 losses.py:179-185
 * With gate_depth_b1hw the chain is run twice: from the gate map's depth it gives px, py, s and z_gate (the reference's
 * cur_depth_b1hw), from depth_b1hw only z_test (its depth_pred_b1hw).  With gate_depth_b1hw NULL the tested map gates itself:
 * one chain, z_gate = z_test.
 *   visible = z_gate < ratio * s  &&  z_gate > 0  &&  s > 0          the reference's comparison as written: s = +inf passes      :187-189
 *   l = log(s) - log(z_test);   err = |l|                                                                                      :222-224
 *   counted = visible, d of depth_b1hw finite and > 0, s finite and > 0, INSIDE
 *   consistent = counted && err <= log_tol
 *   conflict   = counted && l > log_tol      the point lies in front of the surface the source saw: it violates the source's free space
 *   (a point behind the source's surface is occluded there and is neither)
 * Per pixel: n_visible, n_consistent, n_conflict over the K sources;
 *   kept = d finite and > 0  &&  n_consistent >= min_consistent  &&  n_conflict <= max_conflict
 *   weight = kept ? 1 + n_consistent : 0;   filtered_depth = kept ? d : 0      (0 is a hole to every consumer of depth maps here)
 * loss = (1 / K) sum_k mean(err over the pixels of all B maps that are visible for k and whose err is not NaN): nanmean of :226, so NaN
 * when a source has no such pixel.  Which pixels count is decided by the fp32 values above; the err that is summed is evaluated once
 * more in fp64 from the same fp32 inputs (z_test's chain and the two logarithms), so the value returned is the fp64 mean rounded once -
 * the fp32 chain's rounding has a bias per source that a mean over a map does not remove.  Wave reduction, the workgroup's four waves through LDS, one partial
 * per workgroup and source in the workspace, and a second small launch that adds the partials in a fixed order.  No atomics: two calls
 * return the same bits.  Without `loss` neither the reduction nor the second launch happens and no workspace is needed.
 * Every per-pixel output of map b depends on map b alone: B maps in one call equal B calls, bit for bit. */
#define IDH_MV_MAX_SOURCES 16 /* K of one call: pipeline.MAX_RING_CAPACITY */
#define IDH_MV_MAX_MAPS 128   /* B of one call */

/* Host struct, read during the call.  struct_size as above. */
typedef struct idh_mv_consistency_args {
    int64_t struct_size;
    const float *depth_b1hw;            /* (B,1,h,w) the map under test */
    const float *gate_depth_b1hw;       /* (B,1,h,w) the map the visibility gate is computed from, or NULL: depth_b1hw gates itself */
    const float *invK_b44;              /* (B,4,4); only [:3,:3] is read */
    const float *world_T_cam_b44;       /* (B,4,4) */
    const float *src_depth_bk1hw;       /* (B,K,1,src_h,src_w) */
    const float *src_K_bk44;            /* (B,K,4,4) intrinsics at src_h x src_w */
    const float *src_cam_T_world_bk44;  /* (B,K,4,4) */
    uint8_t *counts_b3hw;               /* out (B,3,h,w): n_visible, n_consistent, n_conflict; or NULL */
    float *weight_b1hw;                 /* out (B,1,h,w), or NULL */
    float *filtered_depth_b1hw;         /* out (B,1,h,w), or NULL */
    uint8_t *visible_bkhw;              /* out (B,K,h,w) 1 / 0, or NULL */
    float *err_bkhw;                    /* out (B,K,h,w), NaN where not visible, or NULL */
    float *loss;                        /* out, one float on the device, or NULL */
    double *loss_sum_k;                 /* out (K) the sums behind loss, or NULL; only with loss */
    int64_t *loss_count_k;              /* out (K) their pixel counts, or NULL; only with loss */
    void *workspace;                    /* idh_mv_consistency_workspace_bytes(B, K, h, w) bytes, 8-byte aligned; read only with loss */
    int64_t workspace_bytes;            /* what the caller allocated */
    float ratio;                        /* > 0, finite: the reference's 1.05 */
    float log_tol;                      /* > 0, finite */
    int32_t min_consistent;             /* >= 0 */
    int32_t max_conflict;               /* >= 0 */
    int32_t B, K, h, w;
    int32_t src_h, src_w;               /* must equal h, w */
} idh_mv_consistency_args;

size_t idh_sizeof_mv_consistency_args(void);

/* 16 * K * B * ceil(h * w / 256) bytes: a double and an int64 per workgroup and source.  0 if an argument is <= 0. */
size_t idh_mv_consistency_workspace_bytes(int B, int K, int h, int w);

/* IDH_EINVAL: args NULL, struct_size short, B < 0, K, h, w, src_h or src_w <= 0, ratio or log_tol not finite and > 0, min_consistent or
 * max_conflict < 0, a null depth / invK / world_T_cam / src_depth / src_K / src_cam_T_world, loss_sum_k or loss_count_k without loss,
 * workspace not 8-byte aligned (with loss);
 * IDH_EUNSUPPORTED: K > IDH_MV_MAX_SOURCES, B > IDH_MV_MAX_MAPS, (src_h, src_w) != (h, w), B * K * h * w >= 2^31;
 * IDH_EWORKSPACE (with loss): workspace NULL or workspace_bytes short.  B == 0 is IDH_OK without a launch. */
int idh_mv_consistency_fwd(const idh_mv_consistency_args *args, void *stream);

/* ---- Edge mask of a depth map and the validation losses that read it (csrc/edge_mask.hip) --------------------------
 *
 * The reference's get_edge_mask (utils/generic_utils.py:286-292; with q = 0.975, no dilation and a bool result the dataset's variant,
 * datasets/generic_mvs_dataset.py:650-658) without kornia and without a sort:
 *   S    = kornia.filters.sobel(1 / depth) of kornia 0.6.7 (normalized=True, eps=1e-6), restated from its documented definition:
 *          x = 1 / depth as an IEEE fp32 division (depth 0 gives +inf); gx, gy the 3x3 Sobel taps / 8 as a cross-correlation with
 *          `replicate` padding, all nine products formed and added in row-major order, the zero taps included (0 * inf = NaN);
 *          S = sqrt((gx gx + gy gy) + 1e-6).  fp32, nothing contracted.  The NaN set and the inf set of S are the composition's.
 *   thr  = torch.nanquantile(S.flatten(1), q, dim=1), linear interpolation, per image: n = the number of non-NaN values (+inf counts
 *          and sorts last); rank = max(q * (n - 1), 0) in fp32; the order statistics floor(rank) and ceil(rank) combined by at::lerp
 *          with the weight rank - floor(rank): a + w (b - a) for w < 0.5, b - (b - a) (1 - w) otherwise, so that a non-finite threshold
 *          has the class torch's has; n == 0 gives NaN.  The selection is exact (a radix select over order-preserving keys, integer
 *          histograms): the two order statistics are the ones a sort finds.
 *   mask = S > thr (a NaN on either side: 0); with `dilate` F.max_pool2d(mask, 5, 1, 2): 1 where any in-image pixel of the 5x5 window is 1.
 * Three launches (S; one workgroup per image for thr; mask), no floating-point atomics, no workgroup waits on another: two calls return
 * the same bits. */

/* Host struct, read during the call.  struct_size as above. */
typedef struct idh_edge_mask_args {
    int64_t struct_size;
    const float *depth_b1hw; /* (B,1,H,W) */
    void *mask_b1hw;         /* out (B,1,H,W): float 1 / 0, or uint8 1 / 0 with mask_u8 */
    float *sobel_b1hw;       /* out (B,1,H,W) the map S, or NULL */
    float *threshold_b;      /* out (B) the per-image threshold, or NULL */
    void *workspace;         /* idh_edge_mask_workspace_bytes(B, H, W) bytes, 4-byte aligned */
    int64_t workspace_bytes; /* what the caller allocated */
    float q;                 /* in [0, 1]: the reference's 0.95 (the dataset's 0.975) */
    int32_t dilate;          /* 1: the 5x5 max-pool */
    int32_t mask_u8;         /* 1: mask_b1hw is uint8 */
    int32_t B, H, W;
} idh_edge_mask_args;

size_t idh_sizeof_edge_mask_args(void);

/* Room for S and the thresholds (each rounded up to 256 bytes); 0 if an argument is <= 0. */
size_t idh_edge_mask_workspace_bytes(int B, int H, int W);

/* IDH_EINVAL: args NULL, struct_size short, depth or mask NULL, B < 0, H or W < 1, q outside [0, 1] (or NaN), workspace not 4-byte
 * aligned; IDH_EUNSUPPORTED: H * W > 2^24 (the rank is formed in fp32) or the number of tiles of a launch >= 2^31;
 * IDH_EWORKSPACE: workspace NULL or workspace_bytes short.  B == 0 is IDH_OK without a launch. */
int idh_edge_mask_fwd(const idh_edge_mask_args *args, void *stream);

/* The phase != "train" branch of BDModel.compute_binary_losses (experiment_modules/bd_model.py:451-495), forward value only:
 *   target = rendered < depth;  mask = depth > 0 && rendered > 0 (depth broadcast over the D planes);
 *   reg_mask = mask && edge_mask != 0 (edge_mask broadcast; NULL: reg_mask = mask, the reference without bd_edge_regularision);
 *   binary_loss/0 = mean over mask of BCEWithLogits(pred, target; pos_weight):  (1 - t) x + (1 + (pos_weight - 1) t) (log1p(exp(-|x|)) + max(-x, 0));
 *   reg_loss/0    = mean over reg_mask of 2 (0.5 - |sigmoid(pred) - 0.5|);
 *   total         = binary_loss/0 + (bd_regularisation_weight > 0 ? reg_loss/0 * bd_regularisation_weight : 0), in fp32 on the two fp32 means.
 * An empty mask gives total = 0 (the reference's edge case) with both means NaN; an empty reg_mask gives reg_loss/0 = NaN, the mean of
 * nothing.  Which elements count is decided on the fp32 inputs; the terms are evaluated in fp64 from the fp32 logits and each mean is
 * rounded to fp32 once.  One partial per chunk of 2048 elements in the workspace and a second launch that adds them in a fixed order: the
 * result does not depend on the grid (max_workgroups) and two calls return the same bits.  No atomics.
 * out5 (device, five doubles): count(mask), count(reg_mask), binary_loss/0, reg_loss/0, total. */
typedef struct idh_bd_val_losses_args {
    int64_t struct_size;
    const float *pred_bdhw;         /* (B,D,h,w) logits: outputs["pred_0"] */
    const float *rendered_bdhw;     /* (B,D,h,w) */
    const float *depth_b1hw;        /* (B,1,h,w) */
    const float *edge_mask_b1hw;    /* (B,1,h,w) float, or NULL */
    double *out5;                   /* out, 8-byte aligned */
    void *workspace;                /* idh_bd_val_losses_workspace_bytes(B, D, h, w) bytes, 8-byte aligned */
    int64_t workspace_bytes;        /* what the caller allocated */
    float bd_regularisation_weight; /* not NaN */
    float positive_weight;          /* run_opts.binary_loss_positive_weight (1.0 in every shipped configuration); not NaN */
    int32_t max_workgroups;         /* 0: the default grid; > 0: at most that many workgroups (the result is the same) */
    int32_t B, D, h, w;
} idh_bd_val_losses_args;

size_t idh_sizeof_bd_val_losses_args(void);

/* 32 bytes per chunk of 2048 elements of B * D * h * w; 0 if an argument is <= 0. */
size_t idh_bd_val_losses_workspace_bytes(int B, int D, int h, int w);

/* IDH_EINVAL: args NULL, struct_size short, pred / rendered / depth / out5 NULL, B, D, h or w < 1, max_workgroups < 0, a NaN weight,
 * out5 or workspace not 8-byte aligned; IDH_EUNSUPPORTED: B * D * h * w >= 2^31; IDH_EWORKSPACE: workspace NULL or workspace_bytes short. */
int idh_bd_val_losses_fwd(const idh_bd_val_losses_args *args, void *stream);

/* ---- DepthModel's validation losses (csrc/reg_losses.hip) -----------------------------------------------------------
 *
 * DepthModel.compute_losses (experiment_modules/depth_model.py:442-540), forward value only: MSGradientLoss (losses.py:77-101 with
 * pyrdown, utils/generic_utils.py:85-91), NormalsLoss (losses.py:119-140), the masked point-wise terms (:480-508) and the cocktail
 * (:527).  The multi-view term (:517-525) is idh_mv_consistency_fwd's `loss`; its device scalar is read here through `mv_loss`.
 *
 * kornia's two functions are restated from the documented definition of kornia 0.6.7; kornia is not installed where this project is
 * built and tested, so this part of the contract is not machine-checked against the library (as for §4.18 and §4.27):
 *   blur_pool2d(x, 3)    the kernel outer([1,2,1],[1,2,1]) / 16 as a cross-correlation with zero padding 1 and stride 2: an output of
 *                        ceil(H/2) x ceil(W/2); out[Y][X] = sum_ij k[i][j] x[2Y-1+i][2X-1+j] over the taps inside the image, row-major.
 *                        All nine weights are non-zero: a NaN or inf input makes every output that touches it non-finite.
 *   spatial_gradient(x)  (sobel, order 1, normalised) the pair [[-1,0,1],[-2,0,2],[-1,0,1]] / 8 and its transpose as a cross-correlation
 *                        with `replicate` padding of 1; all nine taps are multiplied and summed in row-major order, the zero taps
 *                        included (0 * NaN = 0 * inf = NaN): which gradients are finite is part of the contract.
 * Terms (every mean is sum / count, so the mean of nothing is 0 / 0 = NaN, as nn.L1Loss and torch.mean give on empty input):
 *   grad_loss    = sum over levels l < num_scales of mean |g_pred - g_gt|, level 0 the two depth maps, level l + 1 = blur_pool2d of level
 *                  l; the mean of a level runs over the gx and the gy entries, separately, at which that component of g_gt is finite
 *                  (C = 1: isfinite().all(dim=1) is per component).  A non-finite g_pred there makes the loss non-finite.   losses.py:83-101
 *   ms_loss      = sum over the present scales i of mean |log gt - nearest(log_pred_s[i])| / 2^i over mask_b; scale i has size
 *                  (scale_h[i], scale_w[i]) dividing (h, w), and the nearest tap of pixel (y, x) is (y / (h / scale_h), x / (w / scale_w)),
 *                  which is F.interpolate(mode="nearest") for integer ratios.  Scale 0 is required (the reference reads it at :477).  :480-492
 *   abs_loss     = mean |gt - pred| over mask_b;   log_l1_loss = mean |d| with d = log gt - log_pred_s[0] over mask_b         :502, :508
 *   si_loss      = sqrt(mean(d^2) - si_lambda * mean(d)^2) over mask_b                                              losses.py:111-116
 *   inv_abs_loss = mean |1 / gt - 1 / pred| over mask_b && pred > 0.1f                                                        :505-506
 *   normals_loss = mean 0.5 (1 - n_gt . n_pred) over the pixels whose six components are all finite                  losses.py:119-140
 *   loss         = ((ms_loss + grad_loss) + normals_loss) + 0.2f * mv_loss in fp32 on the fp32 values, as :527 forms it.
 * With `hypersim` grad_loss, normals_loss and mv_loss are the reference's literal 0 (:498-515): their inputs may be NULL and the launches
 * of pyramid levels 1 .. 3 are skipped.
 * Which elements count is decided as above; every value is then evaluated in fp64 from the fp32 inputs - the pyramid levels are kept as
 * doubles in the workspace - and rounded to fp32 once, so the finite / non-finite pattern is the fp32 composition's as long as that does
 * not overflow.  One launch per pyramid level: a workgroup owns 32 x 32 tiles of a level of one image, stages them with a one-pixel halo
 * in LDS (a lane's four pixels are one 16-byte load per map where the rows are 16-byte aligned: w a multiple of 4 and aligned bases;
 * anything else takes scalar loads), and writes one record of fp64 partial sums per tile - not per workgroup - plus its 16 x 16 tile of the next level; level 0's
 * launch also evaluates the point-wise terms and the normals.  A last launch of one workgroup adds the records in tile order.  At most five
 * launches, no floating-point atomics: the result is the same for every grid (max_workgroups) and two calls return the same bits.
 * out16 (device, sixteen doubles): loss, si_loss, grad_loss, abs_loss, normals_loss, ms_loss, inv_abs_loss, log_l1_loss, mv_loss - each
 * an fp32 value - then the element counts behind the means: gradient levels 0 .. 3, mask_b, mask_b && pred > 0.1, the normals mask.
 * A term that `terms` leaves out is NaN with a count of 0 (under `hypersim` the three terms above are 0). */
#define IDH_REG_TERM_GRAD 1    /* the gradient pyramid */
#define IDH_REG_TERM_POINT 2   /* ms, abs, log_l1, si, inv_abs */
#define IDH_REG_TERM_NORMALS 4 /* normals_loss */
#define IDH_REG_TERM_ALL 7

typedef struct idh_reg_val_losses_args {
    int64_t struct_size;
    const float *depth_gt_b1hw;        /* (B,1,h,w) cur_data["depth_b1hw"]; with GRAD or POINT */
    const float *depth_pred_b1hw;      /* (B,1,h,w) outputs["depth_pred_s0_b1hw"]; with GRAD or POINT */
    const uint8_t *mask_b_b1hw;        /* (B,1,h,w) bool bytes, cur_data["mask_b_b1hw"]; with POINT */
    const float *log_depth_pred_s[4];  /* (B,1,scale_h[i],scale_w[i]) outputs["log_depth_pred_s{i}_b1hw"], NULL: absent; [0] required with POINT */
    const float *normals_gt_b3hw;      /* (B,3,h,w); with NORMALS unless hypersim */
    const float *normals_pred_b3hw;    /* (B,3,h,w); with NORMALS unless hypersim */
    const float *mv_loss;              /* one float on the device, read by the last launch in stream order; NULL: 0 */
    double *out16;                     /* out, 8-byte aligned */
    void *workspace;                   /* idh_reg_val_losses_workspace_bytes(B, h, w) bytes, 8-byte aligned */
    int64_t workspace_bytes;           /* what the caller allocated */
    float si_lambda;                   /* not NaN: the reference's 0.85 */
    int32_t hypersim;                  /* != 0: run_opts.dataset == "hypersim" */
    int32_t num_scales;                /* pyramid levels of grad_loss, 1 .. 4; 0: 4 */
    int32_t terms;                     /* a combination of IDH_REG_TERM_*; 0: all */
    int32_t max_workgroups;            /* 0: the default grid; > 0: at most that many workgroups per launch (the result is the same) */
    int32_t B, h, w;
    int32_t scale_h[4], scale_w[4];    /* read for the present scales: each must divide h, w */
} idh_reg_val_losses_args;

size_t idh_sizeof_reg_val_losses_args(void);

/* Levels 1 .. 3 of both pyramids as doubles (each map rounded up to 256 bytes) and the tile records: 128 bytes per 32 x 32 tile of level 0,
 * 16 bytes per tile of levels 1 .. 3.  0 if an argument is <= 0. */
size_t idh_reg_val_losses_workspace_bytes(int B, int h, int w);

/* IDH_EINVAL: args NULL, struct_size short, out16 NULL, B < 0, h or w < 1, max_workgroups < 0, num_scales outside 0 .. 4, unknown bits in
 * terms, a NaN si_lambda, a pointer NULL that the terms need (above), no scale present / scale 0 absent with POINT, a present scale whose size
 * is < 1 or does not divide (h, w), out16 or workspace not 8-byte aligned; IDH_EUNSUPPORTED: B * h * w >= 2^31;
 * IDH_EWORKSPACE: workspace NULL or workspace_bytes short.  B == 0 is IDH_OK without a launch. */
int idh_reg_val_losses_fwd(const idh_reg_val_losses_args *args, void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* IDH_GEOMETRY_H_ */
