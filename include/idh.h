/*
 * idh.h — C ABI of the MI355X-native cost-volume hot path of nianticlabs/implicit-depth.
 *
 * The reference has no native/FFI layer: its hot path is a set of Python nn.Module
 * attributes of BDModel / DepthModel that are swapped by attribute replacement
 * (reference test_bd.py:80-81, `model.cost_volume = model.cost_volume.to_fast()`).
 * Each entry point below replaces the body of one such module's forward(); the
 * reference file:line it replaces is cited per function.  INTEGRATION.md shows the
 * ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (gfx950 HBM) unless the name ends in _host;
 *   - tensors are dense fp32; layouts are spelled in the parameter names
 *     (nchw / nhwc / bdhw ...), strides are in floats;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are
 *     asynchronous on that stream, never synchronise the device and never allocate:
 *     the caller owns outputs and the workspace (size from the *_workspace_bytes call);
 *   - return value: IDH_OK (0) or a negative IDH_E* code; nothing throws.
 */
#ifndef IDH_H_
#define IDH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the declarations of this header are its whole dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define IDH_OK 0
#define IDH_EINVAL (-1)      /* bad shape / null pointer / unsupported parameter */
#define IDH_EUNSUPPORTED (-2) /* valid request the kernels do not cover (e.g. C != 16) */
#define IDH_ELAUNCH (-3)      /* hipLaunchKernel reported an error */
#define IDH_EWORKSPACE (-4)   /* workspace pointer null or too small */

#define IDH_MAX_SOURCE_VIEWS 16

/* activation codes for the conv / MLP epilogues */
#define IDH_ACT_NONE 0
#define IDH_ACT_LRELU 1 /* LeakyReLU(slope) */
#define IDH_ACT_ELU 2   /* ELU(alpha=1) */

int idh_version(void);
const char *idh_error_string(int code);

/* ---- layout helpers ------------------------------------------------------------ */
/* (n_img, C, HW) -> (n_img, HW, C).  Replaces the implicit .contiguous()/permute the
 * reference does around grid_sample (reference bd_model.py:170-171). */
int idh_nchw_to_nhwc_f32(const float *src_nchw, float *dst_nhwc, int n_img, int C, int HW, void *stream);
int idh_nhwc_to_nchw_f32(const float *src_nhwc, float *dst_nchw, int n_img, int C, int HW, void *stream);

/* ---- options shared by the two plane-sweep volumes ------------------------------ */
/* Optional extras of the two volume entry points (the *_ex_fwd forms; NULL = all defaults).
 *   cur/src_batch_stride  floats between consecutive batch elements of cur_nhwc / src_nhwc (0 = dense:
 *                         H*W*C and K*H*W*C).  Lets the matching-encoder head hand over ONE
 *                         (B, K+1, H, W, C) buffer — frame b's current image followed by its K source images, the
 *                         order reference bd_model.py:149-160 produces — without a regrouping copy.
 *   planes                caller-supplied depth planes = the reference's `depth_planes_bdhw` argument
 *                         (modules/cost_volume.py:324-347, used instead of generate_depth_planes): element
 *                         (b,d,pixel) at planes[b*planes_batch_stride + d*planes_plane_stride +
 *                         pixel*planes_pixel_stride]; pixel stride 0 (an expand()ed (B,D,1,1) view) or 1
 *                         (dense per-pixel planes).  NULL = log-spaced planes from dmin/dmax; when given,
 *                         dmin/dmax are ignored and planes_d is not written.
 * Host struct, read during the call. */
typedef struct idh_volume_opts {
    int64_t cur_batch_stride;
    int64_t src_batch_stride;
    const float *planes;
    int64_t planes_batch_stride;
    int64_t planes_plane_stride;
    int32_t planes_pixel_stride;
    int32_t kernel; /* dot-product volume only: 0 = automatic (the launcher's choice), or force one IDH_CV_KERNEL_* —
                       a test / profiling hook so that every kernel can be checked against the same goldens */
    float *scratch; /* dot-product volume only, optional: >= idh_cost_volume_dot_scratch_floats(...) floats of device memory.
                       When the launch splits the depth planes over workgroups, each group leaves its (best cost, plane) per
                       pixel here and the arg-max pass combines those instead of re-reading the whole volume (same result:
                       first maximum wins).  NULL: no scratch, the pass reads the volume. */
    int64_t scratch_floats;
    int64_t struct_size; /* = sizeof(idh_volume_opts) of the header the caller was built against.  The fields from `scratch` on exist since ABI
                            version 101; the library honours them only when struct_size >= offsetof(struct_size) + 8, i.e. when the caller says
                            its struct reaches at least this far (a LARGER value - a later header with more fields appended - is accepted).
                            This is a consistency check between a caller and the header it was built with, NOT protection for a caller built
                            against the shorter version-100 struct: for such a caller the field itself lies past the end of its struct.  A
                            binding must therefore compare idh_sizeof_volume_opts() / idh_version() with its own mirror when it loads the
                            library (implicit-depth_amd/_lib.py does, and refuses to bind on a mismatch). */
    int32_t fv_keep_empty_views; /* MLP feature volume only (C = 16, K <= 8, fp32).  There are two kernels per view count, both instances of one
                                    template (fv_mlp_k<KT, kSkip>).  The skipping one (<KT, true>) drops a source view from a 16-voxel tile's plane
                                    when none of the voxels has a non-zero bilinear weight in it - no taps, blend or layer-1 MFMAs; the same values
                                    for finite features (csrc/feature_volume.hip names the Inf / NaN and -0 footnotes) - and is slower than the
                                    all-views one (<KT, false>) where nothing can be dropped.  0 (default): each launch runs the faster of the two
                                    for its cameras (a device-side estimate, no synchronisation); 1: always the all-views kernel, every view
                                    processed; 2: always the skipping kernel (A/B timing, tests).
                                    Appended after struct_size: honoured when struct_size reaches past it. */
    int32_t win_units_per_split; /* dot-product volume, window kernel only (was reserved0: same offset, same struct size): 0 = automatic (the launcher's
                                    rule), otherwise the number of 4-plane units one workgroup of cv_dot_win_k processes - a test / profiling hook so
                                    that every plane split (4- and 8-plane slices, whole super-groups of 16 planes, several super-groups per
                                    workgroup) can be checked against the same oracle at a small shape.  Must be 1, 2 or a multiple of 4; values
                                    beyond the planes there are count as 4 * ceil(ceil(D / 4) / 4), and (units / 4) * K must stay <= 16 (the
                                    per-workgroup pair table): anything else is IDH_EINVAL before any launch.  Results do not depend on it.  No
                                    effect when another kernel takes the launch.  Honoured when struct_size reaches past it;
                                    idh_cost_volume_dot_plan reports the split and the scratch a launch with this value wants. */
} idh_volume_opts;

/* sizeof(idh_volume_opts) as compiled into the library (bindings assert their mirror matches; idh_version() >= 101). */
size_t idh_sizeof_volume_opts(void);

#define IDH_CV_KERNEL_LANE 1   /* cv_dot_k: one lane per sample, taps through the vector L1 */
#define IDH_CV_KERNEL_QUAD 2   /* cv_dot_quad_k: four lanes per sample, quad-coalesced taps */
#define IDH_CV_KERNEL_WINDOW 3 /* cv_dot_win_k: source windows staged in LDS (needs a map of >= 48 x 12 texels) */

/* ---- plane-sweep dot-product cost volume --------------------------------------- */
/* Replaces CostVolumeManager.build_cost_volume + forward
 * (reference modules/cost_volume.py:221-358; geometry utils/geometry_utils.py:55-89):
 *   cost[b,d,y,x] = sum_k sum_c cur[b,y,x,c] * bilinear_zeros(src[b,k], proj_k(x,y,depth_d))[c]
 *   lowest[b,y,x] = depth_{argmax_d cost[b,d,y,x]}   (first maximum wins)
 * with depth_d log-spaced in [dmin,dmax] (cost_volume.py:98-132).
 *   cur_nhwc   (B,H,W,C)      src_nhwc (B,K,H,W,C)        C must be 16
 *   src_K_44   (B,K,4,4) source intrinsics at matching scale
 *   src_E_44   (B,K,4,4) src_cam_T_cur_cam
 *   cur_invK_44(B,4,4)
 *   cost       out: (B,D,H,W) when cost_nhwc_cs == 0 (the reference's layout), or NHWC
 *              (B,H,W,cost_nhwc_cs >= D) so the CVEncoder's first conv reads it directly
 *   lowest_bhw (B,H,W) out or NULL; planes_d (D) out or NULL
 * One volume kernel (plus a small arg-max pass when the planes are split over workgroups), no workspace needed.
 */
int idh_cost_volume_dot_fwd(const float *cur_nhwc, const float *src_nhwc, const float *src_K_44,
                            const float *src_E_44, const float *cur_invK_44, float dmin, float dmax,
                            int B, int K, int C, int H, int W, int D, float *cost, int cost_nhwc_cs,
                            float *lowest_bhw, float *planes_d, void *stream);
int idh_cost_volume_dot_ex_fwd(const float *cur_nhwc, const float *src_nhwc, const float *src_K_44,
                               const float *src_E_44, const float *cur_invK_44, float dmin, float dmax,
                               int B, int K, int C, int H, int W, int D, float *cost, int cost_nhwc_cs,
                               float *lowest_bhw, float *planes_d, const idh_volume_opts *opts, void *stream);

/* Floats of idh_volume_opts.scratch the window kernel can use for this shape (0: another kernel takes it): the arg-max partials of a launch that
 * splits the planes over workgroups (2 * groups * B * H * W), followed - since ABI 105 - by the run lists of every (frame, tile, plane group) task,
 * which a small kernel (cv_runs_k) then builds AHEAD of the volume kernel instead of every workgroup in its own prologue (~10 % of its life).  Results
 * are bit-identical with any scratch size: a scratch that only covers the first part just forgoes the second. */
long long idh_cost_volume_dot_scratch_floats(int B, int K, int C, int H, int W, int D);

/* Host-only query (additive: idh_version() stays as it is; no device access, usable without a GPU): what a launch of these dimensions with
 * idh_volume_opts.kernel = `kernel` and .win_units_per_split = `win_units_per_split` (0 / 0 = automatic) would do - the function the launch calls.
 *   psplit            plane groups = workgroups per tile; > 1: a second, small kernel finishes the arg-max
 *   units_per_split   4-plane units per workgroup (the effective value of the hook)
 *   partial_floats    floats of arg-max partials at the start of the scratch (0 when psplit == 1); the run lists start behind them
 *   runs_stride       ints per (frame, tile, plane group) task in the run-list part: {count, (xy, info) x capacity}, task = ((b ty) tx) psplit + group
 *   scratch_floats    partial_floats + tasks * runs_stride = idh_cost_volume_dot_scratch_floats for kernel = win_units_per_split = 0
 * All five are 0 when another kernel takes the launch.  Any output pointer may be NULL.  IDH_EINVAL for dimensions, a kernel or a split the launch
 * refuses too. */
int idh_cost_volume_dot_plan(int B, int K, int C, int H, int W, int D, int kernel, int win_units_per_split, int *psplit, int *units_per_split,
                             long long *partial_floats, int *runs_stride, long long *scratch_floats);

/* Name of the kernel idh_cost_volume_dot*_fwd launches for this shape (what rocprofv3 --kernel-trace will show);
 * lets bench.py label its roofline without guessing the launcher's choice. */
const char *idh_cost_volume_dot_kernel_name(int B, int K, int H, int W, int D);

/* ---- plane-sweep MLP feature volume ---------------------------------------------------- */
/* Replaces FeatureVolumeManager.build_cost_volume + forward (reference
 * modules/cost_volume.py:437-706, 324-358) for K <= 8 source views, C = 16, hidden width 128:
 *   vol[b,d,y,x] = MLP([warped src feats (16K), cur feats (16), mask (K), depths (K), plane depth,
 *                       dot products (K), ray angles (K), rays (3(K+1)), pose distances (3K)])
 * with MLP = Linear -> LeakyReLU(.01) -> Linear -> LeakyReLU(.01) -> Linear (networks.py:218-233).
 * The first Linear's weight W1 (128 x 16(K+1)+10K+4) is passed in three pieces, in the K order
 * the kernel builds its operands in (implicit-depth_amd/cost_volume.py:pack_feature_mlp):
 *   w1_voxel_packed  per-voxel columns [warped K*16 | 4 metadata blocks], MFMA fragment order.  Metadata blocks of the fp32 kernel for
 *                    K <= 8, C = 16 (fv_mlp_k, ABI >= 103): lane quarter q carries [z, dot, ray angle, ray xyz] of views q and q + 4 at slots
 *                    0..5 / 6..11 of three 16-column blocks; the plane depth sits in quarter 3's slot 6 when K < 8, else alone in block 3
 *                    (quarter 0, k-step 0).  The K per-view "valid" columns are NOT in the blob: those inputs are identically 1 (z is
 *                    clamped to 1e-5 before the z > 0 test, geometry_utils.py:86), so the caller adds their weight columns to `b1`
 *                    (implicit-depth_amd/cost_volume.py: feature_mlp_column_maps(fold_mask=True), feature_mlp_mask_columns).  The generic
 *                    kernel (K > 8 / C = 32, fv_mlp_gen_k) takes EIGHT slots per view group j (views q + 4j): [valid, z, dot, ray angle |
 *                    ray xyz, plane depth (group 0, quarter 0) / 0] = 2 ceil(K/4) blocks (layout="gen8"); the f16x3 kernel keeps the
 *                    seven-slot packing with the mask column (the default of feature_mlp_column_maps).
 *   w1_pixel_packed  per-pixel columns [cur feats 16 | cur ray 3 + pad], MFMA fragment order
 *   w1_pose_rowmajor (128, 3K) columns of the pose-distance / R / t measures (folded into a
 *                    per-batch-element bias on the device)
 *   vecs_b2_w3_b3    3 x 128 floats: b2, W3[0,:], [b3, 0...]
 *   vol              (B,D,H,W) when vol_nhwc_cs == 0, else NHWC (B,H,W,vol_nhwc_cs >= D)
 *   lowest_bhw       (B,H,W) or NULL; mask_bhw (B,H,W) uint8 "overall mask" of the LAST plane or
 *                    NULL; planes_d (D) or NULL (written together with lowest_bhw)
 *   workspace        >= idh_feature_volume_workspace_bytes(B)
 * One frame's K source maps are addressed through a buffer descriptor: K*H*W*C*4 bytes must stay below 2 GiB (else IDH_EUNSUPPORTED).
 */
size_t idh_feature_volume_workspace_bytes(int B);
/* Host-only query (ABI >= 107): how idh_feature_volume*_fwd splits the D depth planes of this shape over tasks.  A task is one tile of 16
 * pixels times one group of consecutive planes [g * planes_per_group, min(D, (g + 1) * planes_per_group)); `groups` of them cover D, the
 * last one may be shorter.  The launch calls the same function, so the answer is the partition the kernels run (K, C and the math mode
 * do not enter the choice).  IDH_EINVAL for non-positive sizes, D > 4096 or a NULL output pointer. */
int idh_feature_volume_plane_groups(int B, int H, int W, int D, int *groups, int *planes_per_group);
/* Host-only queries (additive: idh_version() stays as it is): the order in which the kernel that drops views (fv_mlp_k<KT, true>) walks its
 * ntasks = B * ceil(H * W / 16) * groups tasks.  idh_feature_volume_grid: the number of workgroups the launch uses (8 waves each; 0 for
 * ntasks <= 0).  idh_feature_volume_skip_task: the task that wave `wave` (0..7) of workgroup `block` (0..grid-1, the hardware's block index)
 * takes in round `round` (0, 1, ...), or -1 when it takes none there - the slot lies past ntasks, or an argument is out of range.  Task t is
 * plane group t % groups of tile (t / groups) % tiles of frame t / (groups * tiles).  The kernel calls the same function. */
int idh_feature_volume_grid(long long ntasks);
long long idh_feature_volume_skip_task(long long ntasks, int grid, int block, int wave, int round);
int idh_feature_volume_fwd(const float *cur_nhwc, const float *src_nhwc, const float *src_K_44,
                           const float *src_E_44, const float *src_poses_44, const float *cur_invK_44,
                           float dmin, float dmax, int B, int K, int C, int H, int W, int D,
                           const float *w1_voxel_packed, const float *w1_pixel_packed,
                           const float *w1_pose_rowmajor, const float *b1, const float *w2_packed,
                           const float *vecs_b2_w3_b3, float *vol, int vol_nhwc_cs, float *lowest_bhw,
                           unsigned char *mask_bhw, float *planes_d, void *workspace,
                           size_t workspace_bytes, void *stream);

/* Same with idh_volume_opts (batch strides, caller-supplied planes); f16x3 != 0 selects the split-precision
 * variant below (then w1_voxel / w2 are the f16 packs). */
int idh_feature_volume_ex_fwd(const float *cur_nhwc, const float *src_nhwc, const float *src_K_44,
                              const float *src_E_44, const float *src_poses_44, const float *cur_invK_44,
                              float dmin, float dmax, int B, int K, int C, int H, int W, int D,
                              const void *w1_voxel, const float *w1_pixel_packed,
                              const float *w1_pose_rowmajor, const float *b1, const void *w2,
                              const float *vecs_b2_w3_b3, float *vol, int vol_nhwc_cs, float *lowest_bhw,
                              unsigned char *mask_bhw, float *planes_d, void *workspace,
                              size_t workspace_bytes, int f16x3, const idh_volume_opts *opts, void *stream);

/* Split-precision ("f16x3") variant of the same kernel: the two 128-wide layers run on
 * v_mfma_f32_16x16x32_f16 with every fp32 operand expanded into two round-to-nearest f16 pieces
 * (power-of-two scaled per hidden unit for the weights, per voxel for the activations) and the three
 * significant cross products accumulated in fp32 — fp32-equivalent results (tests/test_mlp_split_gpu.py)
 * at 3/16 of the fp32-MFMA cost.  Same arguments, except that w1_voxel_f16 / w2_f16 come from
 * idh_pack_mlp_weight_f16 and the voxel columns are ordered [4 metadata blocks | warped K*16]
 * (implicit-depth_amd/cost_volume.py).  idh_pack_mlp_weight_f16 packs columns [col0, col0+n_in) of a
 * row-major (128, ld) matrix as [ceil(n_in/32)][8][piece 2][lane 64][8 halves] followed by the 128
 * per-row scale floats. */
size_t idh_packed_mlp_weight_f16_bytes(int n_in);
int idh_pack_mlp_weight_f16(const float *w_row_major, void *dst, int ld, int col0, int n_in, void *stream);
int idh_feature_volume_f16x3_fwd(const float *cur_nhwc, const float *src_nhwc, const float *src_K_44,
                                 const float *src_E_44, const float *src_poses_44, const float *cur_invK_44,
                                 float dmin, float dmax, int B, int K, int C, int H, int W, int D,
                                 const void *w1_voxel_f16, const float *w1_pixel_packed,
                                 const float *w1_pose_rowmajor, const float *b1, const void *w2_f16,
                                 const float *vecs_b2_w3_b3, float *vol, int vol_nhwc_cs, float *lowest_bhw,
                                 unsigned char *mask_bhw, float *planes_d, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* ---- per-pixel occlusion MLP over all query planes ---------------------------------- */
/* Replaces the per-plane loop bd_model.py:293-304 -> run_mlp_val (:412-442) ->
 * BinaryMLPNetwork scale 0 (modules/networks.py:98-115): for every pixel m and plane p
 *   x = [depth[b,p,pix], feat[m, 0:Cf], (prior[b,p,pix])]
 *   out[b,p,pix] = W3 . ELU(W2 . ELU(W1 . x + b1) + b2) + b3          (hidden width 128)
 * W1's feature columns and W2 are passed in MFMA fragment order (idh_pack_mlp_weight);
 * vecs6x128 = rows {b1, W1[:,depth], W1[:,prior], b2, W3[0,:], [b3,0,...]}.
 *   feat_nhwc  rows of Cf floats, feat_cs floats apart (B*HW rows); any feat_cs >= Cf and any 4-byte-aligned base since ABI 105
 *              (rows that are not 16-byte aligned - the reference's 65- / 66-float [depth | feat | prior] rows - are read with dword loads)
 *   depth_bphw (B,P,HW); prior_bphw (B,P,HW) or NULL (then prior_const is used when has_prior)
 *   out_bphw   (B,P,HW) logits
 * Feature alignment per entry point (enforced: IDH_EINVAL otherwise; ABI 109):
 *   idh_binary_mlp_fwd                    any feat_cs >= Cf, base 4-byte aligned
 *   idh_binary_mlp_strided_fwd            base 4-byte aligned, pixel and channel stride > 0, batch stride >= 0
 *   idh_binary_mlp_f16x3_fwd and the three idh_binary_mlp_search_*_fwd
 *                                         feat_cs % 4 == 0 and base 16-byte aligned (rows are read with dwordx4 loads only)
 * Cf % 4 == 0 everywhere; B * HW < 2^31 (IDH_EUNSUPPORTED beyond).  B == 0 (and P == 0 for the logit entry points) is IDH_OK and launches nothing.
 */
size_t idh_packed_mlp_weight_floats(int n_in);
int idh_pack_mlp_weight(const float *w_row_major, float *dst, int ld, int col0, int n_in, void *stream);
int idh_binary_mlp_fwd(const float *feat_nhwc, int feat_cs, int Cf, const float *depth_bphw,
                       const float *prior_bphw, int has_prior, float prior_const,
                       const float *w1f_packed, const float *w2_packed, const float *vecs6x128, int B,
                       int P, int HW, float *out_bphw, void *stream);
/* The same pass over features with arbitrary strides: element (b, pix, c) at feat[b * feat_batch_stride + pix * feat_pixel_stride +
 * c * feat_channel_stride] (floats).  (1, HW-contiguous planes) reads the channel planes of an NCHW tensor in place: BDModel.run_mlp_val
 * (bd_model.py:415-439) concatenates [rendered_depth | feature_s0 | prior] along dim 1 and hands the MLP a permute(0, 2, 3, 1) VIEW of it -
 * with this entry point the drop-in's BinaryMLPNetwork.forward reads that view without materialising (B,H,W,65) rows.  ABI 105. */
int idh_binary_mlp_strided_fwd(const float *feat, long long feat_batch_stride, int feat_pixel_stride, int feat_channel_stride, int Cf,
                               const float *depth_bphw, const float *prior_bphw, int has_prior, float prior_const,
                               const float *w1f_packed, const float *w2_packed, const float *vecs6x128, int B, int P, int HW,
                               float *out_bphw, void *stream);
/* Same, with the per-plane 128x128 layer in "f16x3" split precision (w2_f16 from
 * idh_pack_mlp_weight_f16, csrc/split_f16.h) and ELU's exp on v_exp_f32: fp32-equivalent results
 * (tests/test_mlp_split_gpu.py) at a fraction of the fp32-MFMA cost.  feat_cs % 4 == 0, feat_nhwc 16-byte aligned. */
int idh_binary_mlp_f16x3_fwd(const float *feat_nhwc, int feat_cs, int Cf, const float *depth_bphw,
                             const float *prior_bphw, int has_prior, float prior_const,
                             const float *w1f_packed, const void *w2_f16, const float *vecs6x128, int B,
                             int P, int HW, float *out_bphw, void *stream);

/* Fused per-pixel binary depth search (reference bd_model.py:273-292, infer_depth=True): `iters`
 * dependent evaluations of the same MLP at each pixel's current query depth, bounds [lo,hi], first
 * query (hi-lo)/2, a pixel is "visible" when sigmoid(logit) < threshold.  Outputs the final query
 * depths and the logits of the last evaluation (the reference's outputs["search_depths"] / ["pred_0"]).
 * Constant threshold; idh_binary_mlp_search_thr_fwd takes the per-depth Thresholder.
 * All three search entry points: feat_cs % 4 == 0 and feat_nhwc 16-byte aligned (IDH_EINVAL otherwise, ABI 109); iters > 0, hi > lo,
 * threshold in (0, 1); prior_b1hw is (B,1,HW) or NULL (prior_const). */
int idh_binary_mlp_search_fwd(const float *feat_nhwc, int feat_cs, int Cf, const float *prior_b1hw,
                              int has_prior, float prior_const, const float *w1f_packed,
                              const float *w2_packed, const float *vecs6x128, int B, int HW, int iters,
                              float lo, float hi, float threshold, float *search_depths_b1hw,
                              float *last_logits_b1hw, void *stream);
/* The same search with the per-depth Thresholder (binary_metrics_utils.py:42-52; bd_model.py:282-283):
 * threshold = thresholds[bucketize(query depth, bins)]; pass thr_logits[i] = logit(thresholds[i]). */
int idh_binary_mlp_search_thr_fwd(const float *feat_nhwc, int feat_cs, int Cf, const float *prior_b1hw,
                                  int has_prior, float prior_const, const float *w1f_packed,
                                  const float *w2_packed, const float *vecs6x128, int B, int HW, int iters,
                                  float lo, float hi, const float *bins, const float *thr_logits, int n_bins,
                                  float *search_depths_b1hw, float *last_logits_b1hw, void *stream);
/* f16x3 variant of both searches (w2_f16 from idh_pack_mlp_weight_f16): n_bins == 0 -> constant
 * `threshold`, else the per-depth table. */
int idh_binary_mlp_search_f16x3_fwd(const float *feat_nhwc, int feat_cs, int Cf, const float *prior_b1hw,
                                    int has_prior, float prior_const, const float *w1f_packed,
                                    const void *w2_f16, const float *vecs6x128, int B, int HW, int iters,
                                    float lo, float hi, float threshold, const float *bins,
                                    const float *thr_logits, int n_bins, float *search_depths_b1hw,
                                    float *last_logits_b1hw, void *stream);

/* ---- temporal prior ------------------------------------------------------------------ */
/* Replaces BDModel.sample_prior (reference experiment_modules/bd_model.py:395-410): back-project
 * the rendered depth, project into the previous frame's camera, nearest-neighbour sample the
 * previous prediction (zeros outside), -1 where the rendered depth is not positive.
 *   rendered_depth_bphw (B,P,H,W); prior_pred_bqhw (B,Q,H,W) (plane p samples channel min(p,Q-1))
 *   cur_world_T_cam_44, prior_cam_T_world_44, K_44, invK_44: (B,4,4) at the prediction resolution
 */
int idh_sample_prior_fwd(const float *rendered_depth_bphw, const float *prior_pred_bqhw, int Q,
                         const float *cur_world_T_cam_44, const float *prior_cam_T_world_44,
                         const float *K_44, const float *invK_44, int B, int P, int H, int W,
                         float *out_bphw, void *stream);

/* ---- occlusion queries at sparse rays and 3D points (additive: idh_version() stayed 111; csrc/mlp_rays.hip) -------- */
/* Fused form of BDModel.run_mlp_train's ray path (reference experiment_modules/bd_model.py:313-393): per ray, the feature row is
 * sampled bilinearly from an NHWC map (F.grid_sample, align_corners=False, zero padding, :357-362) and the S depth samples of the ray go
 * through the MLP of idh_binary_mlp_fwd on that one row:
 *   out[b, j, s] = MLP([depth[b, j*ray_step, s] | feat(rays[b, j*ray_step]) | (prior[b, j*ray_step, s])]),  j < Nq = ceil(N / ray_step)
 * (ray_step = scale + 1 is the reference's rays[:, ::(scale + 1)], :352-353).
 *   feat_nhwc   B*H*W rows of Cf floats, feat_cs floats apart: any feat_cs >= Cf, base 4-byte aligned (a channel slice of a wider buffer);
 *               dwordx4 loads when the base is 16-byte aligned and feat_cs % 4 == 0, dword loads otherwise.  Cf % 4 == 0.
 *   rays_bn2    (x, y) in pixel-centre units of a grid_w x grid_h grid: pixel (i, j) of that grid is (i + 0.5, j + 0.5) (:325-326)
 *   depth_bns   (B,N,S); prior_bns (B,N,S) or NULL (then prior_const when has_prior); out_bqs (B,Nq,S) dense
 *   w1f_packed / w2_packed / vecs6x128: as idh_binary_mlp_fwd.  fp32 only (there is no f16x3 form of this entry point).
 * The gather, in fp32 with one rounding per operation (no contraction), per ray and for y alike:
 *   g  = (x / (float)grid_w - 0.5f) * 2.f                  ix = ((g + 1.f) * (float)W - 1.f) * 0.5f
 *   x0 = floorf(ix)        wx0 = (x0 + 1.f) - ix           wx1 = ix - x0
 *   w_nw = wx0 * wy0   w_ne = wx1 * wy0   w_sw = wx0 * wy1   w_se = wx1 * wy1         (torch's (x0+1-ix)(y0+1-iy) ...)
 *   f[c] = (((0 + F[y0][x0][c] * w_nw) + F[y0][x0+1][c] * w_ne) + F[y0+1][x0][c] * w_sw) + F[y0+1][x0+1][c] * w_se
 * where a corner outside [0,W-1] x [0,H-1] contributes nothing and is not read (a non-finite ray has no corner: f = 0).
 * IDH_EINVAL: a NULL pointer (prior_bns may be NULL), negative B or N, S, H, W, Cf <= 0, Cf % 4, feat_cs < Cf, ray_step < 1, grid_w or
 * grid_h <= 0, a pointer that is not 4-byte aligned.  B == 0 or N == 0: IDH_OK, no launch.  IDH_EUNSUPPORTED: B * Nq or B * H * W >= 2^31.
 * Everything is checked on the host before the device is touched. */
int idh_binary_mlp_rays_fwd(const float *feat_nhwc, int feat_cs, int Cf, int B, int H, int W, const float *rays_bn2,
                            const float *depth_bns, const float *prior_bns, int has_prior, float prior_const, int N, int S,
                            int ray_step, int grid_w, int grid_h, const float *w1f_packed, const float *w2_packed,
                            const float *vecs6x128, float *out_bqs, void *stream);
/* Depth and hit point per ray: the binary search of idh_binary_mlp_search_*_fwd (reference BDModel.forward(infer_depth=True),
 * bd_model.py:273-292) at the sparse rays of idh_binary_mlp_rays_fwd, in one launch.  Per ray, once: exactly the gather above (a corner
 * outside the map is not read; a non-finite ray has no corner, f = 0) and pre1 = W1f . f + b1.  Then `iters` dependent evaluations:
 *   q_0 = (hi - lo) * 0.5f   (the reference's first query, not the midpoint)
 *   visible = logit(q_n) < thr(q_n):  visible -> hi = q_n, otherwise lo = q_n;   q_{n+1} = (hi + lo) * 0.5f
 *   thr = logf(threshold / (1 - threshold)) when n_bins == 0, else thr_logits[min(#{bins[e] < q_n}, n_bins - 1)]   (bd_model.py:282-283)
 *   prior_bn (B,N): one value per ray, or NULL (then prior_const when has_prior) - as plane 0 of the dense search's prior
 * Outputs (B,N): depth_bn = q_iters, the final query; last_logits_bn = logit(q_{iters-1}); optional flags_bn (uint8): bit 0 = hi moved at
 * some step, bit 1 = lo moved: 3 = the surface was bracketed inside [lo, hi], 1 or 2 = the search ran into a bound (no hit in range).
 * Optional points_bn3 (B,N,3), needs invK_44 (B,4,4) at the resolution of the rays' grid: with d = depth_bn and (x, y) the ray - whose
 * pixel-centre units already carry BackprojectDepth's + 0.5 (reference utils/geometry_utils.py:39,60-61) - and iK = invK_44[b], T =
 * world_T_cam_44[b], in fp32 with one rounding per operation / fma:
 *   c_i = fmaf(iK[4i], x, fmaf(iK[4i+1], y, iK[4i+2]))     X_i = d * c_i                                                  i = 0..2
 *   p_i = fmaf(T[4i], X_0, fmaf(T[4i+1], X_1, fmaf(T[4i+2], X_2, T[4i+3])))      (world_T_cam_44 == NULL: p_i = X_i, camera space)
 * fp32 only.  IDH_EINVAL: the conditions of idh_binary_mlp_rays_fwd that apply (NULL feat / rays / weights, negative B or N, H, W, Cf <= 0,
 * Cf % 4, feat_cs < Cf, grid_w or grid_h <= 0), iters <= 0, !(hi > lo), n_bins < 0, n_bins == 0 with threshold outside (0, 1), n_bins > 0
 * with a NULL table, points_bn3 without invK_44, a NULL depth_bn or last_logits_bn, a pointer that is not 4-byte aligned (flags_bn: any).
 * B == 0 or N == 0: IDH_OK, no launch.  IDH_EUNSUPPORTED: B * N or B * H * W >= 2^31.  Everything is checked on the host first. */
int idh_binary_mlp_rays_search_fwd(const float *feat_nhwc, int feat_cs, int Cf, int B, int H, int W, const float *rays_bn2,
                                   const float *prior_bn, int has_prior, float prior_const, int N, int grid_w, int grid_h,
                                   const float *w1f_packed, const float *w2_packed, const float *vecs6x128, int iters, float lo, float hi,
                                   float threshold, const float *bins, const float *thr_logits, int n_bins, const float *invK_44,
                                   const float *world_T_cam_44, float *depth_bn, float *last_logits_bn, unsigned char *flags_bn,
                                   float *points_bn3, void *stream);
/* Dense occlusion in a moving camera: every pixel of a depth map rendered in ANY camera is asked against the keyframe's scale-0 features, in one
 * launch, with nothing intermediate in memory (view_mlp_k).  Per pixel (b, p, row, col) of rendered_bphw (B,P,h,w), in fp32 with one rounding per
 * operation / fma (no contraction), with d = rendered[b,p,row,col], iK = invK_44[b], T = world_T_cam_44[b] of the VIEW:
 *   BackprojectDepth (reference utils/geometry_utils.py:55-63, pixel centres :39), as idh_binary_mlp_rays_search_fwd's points:
 *     x = (float)col + 0.5f   y = (float)row + 0.5f
 *     c_i = fmaf(iK[4i], x, fmaf(iK[4i+1], y, iK[4i+2]))     X_i = d * c_i                                                i = 0..2
 *     p_i = fmaf(T[4i], X_0, fmaf(T[4i+1], X_1, fmaf(T[4i+2], X_2, T[4i+3])))                                             the world point
 *   Project3D (:77-89) into the keyframe, exactly idh_project_points_fwd on p with key_cam_T_world_44 / key_K_44 (K at H x W; the product of
 *   BDModel.sample_prior, experiment_modules/bd_model.py:400-403): P = K cam_T_world, c = P[:3] (p, 1), z = fmaxf(c_z, 1e-5f), (u, v) = c_xy / z
 *   prior (has_prior): with prior_pred_b1hw (B,1,H,W), prior_cam_T_world_44 and prior_K_44 the nearest sample of idh_project_points_fwd
 *     (bd_model.py:405-409; -1 behind that camera or outside the map); without a map the constant prior_const
 *   logit = MLP([z | feat(u, v) | (prior)]): the gather of idh_binary_mlp_rays_fwd with grid = (H, W) on F.grid_sample(bilinear, zeros,
 *     align_corners=False) of feature_s0, then BinaryMLPNetwork - the depth is the point's z in the KEYFRAME camera
 * A pixel is valid when d is finite and d > 0, c_z > 0, 0 <= u < W and 0 <= v < H (decided on floats before any integer conversion).  An
 * invalid pixel stores `fill` in logits_bphw and reads no feature corner and no prior texel; a 16-pixel tile without a valid pixel skips the MLP.
 * Outputs: logits_bphw (B,P,h,w); optional (NULL: not written) valid_bphw uint8 0 / 1, view_depth_bphw = z, view_points_bphw3 (B,P,h,w,3) = p;
 * where d is not finite and positive, view_depth and view_points are 0.  For every other pixel logits / view_depth / valid carry the bits
 * of idh_project_points_fwd + idh_binary_mlp_rays_fwd (S = 1) on view_points.
 * fp32 only.  IDH_EINVAL: a NULL required pointer (feat, rendered, the four matrices, weights, logits), a prior map without has_prior or without
 * its two matrices, negative B, P, h or w, H, W, Cf <= 0, Cf % 4, feat_cs < Cf, a float pointer that is not 4-byte aligned.  B == 0 or an empty map
 * (P, h or w == 0): IDH_OK, no launch.  IDH_EUNSUPPORTED: B * P * h * w or B * H * W >= 2^31, B > 128 (the cameras of a launch sit in LDS).
 * Everything is checked on the host before the device is touched. */
int idh_binary_mlp_view_fwd(const float *feat_nhwc, int feat_cs, int Cf, int B, int H, int W, const float *rendered_bphw, int P, int h, int w,
                            const float *invK_44, const float *world_T_cam_44, const float *key_cam_T_world_44, const float *key_K_44,
                            const float *prior_pred_b1hw, const float *prior_cam_T_world_44, const float *prior_K_44, int has_prior,
                            float prior_const, const float *w1f_packed, const float *w2_packed, const float *vecs6x128, float fill,
                            float *logits_bphw, unsigned char *valid_bphw, float *view_depth_bphw, float *view_points_bphw3, void *stream);
/* Depth in a moving camera: the binary search of idh_binary_mlp_rays_search_fwd (reference BDModel.forward(infer_depth=True),
 * experiment_modules/bd_model.py:273-292) along the rays of ANY camera, against the keyframe's scale-0 features, in one launch (view_search_k).
 * A ray is one pixel (b, row, col) of an h x w grid of the view - x = (float)col + 0.5f, y = (float)row + 0.5f - or, with rays_bn2 != NULL, one
 * entry (x, y) of a (B,N,2) list in pixel-centre units of that camera (h and w are then ignored; the view has no bounds, any finite ray is
 * legal; a non-finite ray has no valid probe).  In fp32 with one rounding per operation / fma (no contraction), iK = invK_44[b], T =
 * world_T_cam_44[b] of the VIEW.  Per ray, once:
 *     c_i = fmaf(iK[4i], x, fmaf(iK[4i+1], y, iK[4i+2]))                                                                  i = 0..2
 * then `iters` dependent steps at the query q_n - the z-depth in the VIEW camera, the d of BackprojectDepth (utils/geometry_utils.py:55-63):
 *   1. X_i = q_n * c_i,  p_i = fmaf(T[4i], X_0, fmaf(T[4i+1], X_1, fmaf(T[4i+2], X_2, T[4i+3]))),  Project3D (:77-89) into the keyframe:
 *      P = K cam_T_world, c = P[:3] (p, 1), z = fmaxf(c_z, 1e-5f), (u, v) = c_xy / z, and the nearest prior sample (bd_model.py:405-409) -
 *      idh_binary_mlp_view_fwd's expressions, verbatim
 *   2. the probe is valid when c_z > 0, 0 <= u < W and 0 <= v < H (on floats, before any integer conversion).  A valid probe's
 *      logit = MLP([z | feat(u, v) | (prior)]); an invalid probe reads no feature corner and no prior texel and its logit IS `fill`.
 *      One step is, by definition, idh_binary_mlp_view_fwd on the map rendered = q_n.
 *   3. thr = logf(threshold / (1 - threshold)) when n_bins == 0, else thr_logits[min(#{bins[e] < z}, n_bins - 1)]: keyed by the probe's
 *      KEYFRAME z, the depth the MLP sees and Thresholder.get_thresholds is calibrated on (bd_model.py:282-283); an invalid probe uses its z too
 *   4. q_0 = (hi - lo) * 0.5f;  logit < thr -> hi = q_n (flag bit 0), otherwise lo = q_n (flag bit 1);  q_{n+1} = (hi + lo) * 0.5f
 *      (bd_model.py:286-290).  Flag bit 2: some probe of the ray was invalid.  A NaN or infinite `fill` simply goes through `<`:
 *      fill = -inf (or any value below every threshold) makes "outside the keyframe's view" count as visible, so the search retreats
 *      towards lo; fill = +inf or NaN makes it count as hidden, so the search advances towards hi.
 * Outputs, (B,h,w) or (B,N): depth = q_iters; last_logits = the logit of step iters - 1 (`fill` when that probe was invalid); optional flags
 * (uint8, any alignment); optional points (...,3) = the world point p of q_iters by the expressions of step 1.
 * The MLP answers occlusion AS SEEN FROM THE KEYFRAME: along a ray of the view the search finds the crossing into the region hidden from the
 * keyframe - the surface only to the extent that both cameras see the same side of it - and assumes one crossing inside [lo, hi], as the
 * reference's search does along its own rays.
 * fp32 only.  IDH_EINVAL: the conditions of both parents that apply (a NULL feat / matrix / weights / depth / last_logits, a prior map
 * without has_prior or without its two matrices, negative B, h, w (grid form) or N (list form), H, W, Cf <= 0, Cf % 4, feat_cs < Cf,
 * iters <= 0, n_bins < 0, n_bins == 0 with threshold outside (0, 1), n_bins > 0 with a NULL table, a float pointer that is not 4-byte
 * aligned), !(lo > 0), !(hi > lo), a non-finite lo or hi.  B == 0 or an empty grid / list: IDH_OK, no launch.  IDH_EUNSUPPORTED: B * rays or
 * B * H * W >= 2^31, B > 128 (the cameras of a launch sit in LDS).  Everything is checked on the host before the device is touched. */
int idh_binary_mlp_view_search_fwd(const float *feat_nhwc, int feat_cs, int Cf, int B, int H, int W, int h, int w, const float *rays_bn2, int N,
                                   const float *invK_44, const float *world_T_cam_44, const float *key_cam_T_world_44, const float *key_K_44,
                                   const float *prior_pred_b1hw, const float *prior_cam_T_world_44, const float *prior_K_44, int has_prior,
                                   float prior_const, const float *w1f_packed, const float *w2_packed, const float *vecs6x128, int iters, float lo,
                                   float hi, float threshold, const float *bins, const float *thr_logits, int n_bins, float fill, float *depth,
                                   float *last_logits, unsigned char *flags, float *points, void *stream);
/* Dense occlusion in a moving camera against SEVERAL remembered keyframes, in one launch (view_keys_k): idh_binary_mlp_view_fwd with the
 * projection looped over M keys and ONE MLP pass per pixel.  The keys live in rings indexed by slot s in [0, n_slots):
 *   feat_ring: the (B,H,W,feat_cs) NHWC block of slot s starts at feat_ring + s * key_stride (key_stride in floats)
 *   key_cam_T_world_s44, key_K_s44: (n_slots,B,4,4);  optional prior ring: prior_pred_sb1hw (n_slots,B,1,H,W) with prior_cam_T_world_s44 and
 *   prior_K_s44 (n_slots,B,4,4) - the prior of slot s belongs to the key of slot s
 *   key_slots: HOST array of M distinct slots in priority order (copied into the kernel arguments; it may be freed on return)
 * Per pixel (b, p, row, col), in fp32 with one rounding per operation / fma (no contraction):
 *   the world point p: idh_binary_mlp_view_fwd's BackprojectDepth expressions, verbatim, once
 *   for m = 0 .. M-1: Project3D of p into key key_slots[m] - P_m = K cam_T_world, c = P_m[:3] (p, 1), z_m = fmaxf(c_z, 1e-5f),
 *     (u_m, v_m) = c_xy / z_m, idh_project_points_fwd's expressions - and idh_binary_mlp_view_fwd's validity rule: d finite and > 0,
 *     c_z > 0, 0 <= u_m < W, 0 <= v_m < H
 *   sel = the first m that is valid.  logit = MLP([z_sel | feat_sel(u_sel, v_sel) | prior_sel]): the gather, the nearest prior sample (in
 *     the prior camera of slot key_slots[sel]; without a prior ring the constant prior_const) and the network of idh_binary_mlp_view_fwd on
 *     the selected key alone - no feature corner and no prior texel of another key is read
 *   no valid m: the logit IS `fill`, nothing is gathered; a 16-pixel tile without a pixel that has a valid key skips the MLP
 * Outputs: logits_bphw (B,P,h,w); optional (NULL: not written) key_bphw uint8 = sel (the position in key_slots, NOT the slot), 255 = none;
 * view_depth_bphw = z_sel, z_0 where no key is valid, 0 where d is not finite and positive; view_points_bphw3 (B,P,h,w,3) = p (0 where d
 * is not finite and positive).  By construction the outputs carry the bits of M launches of idh_binary_mlp_view_fwd, one per key in
 * key_slots order, followed by a per-pixel select of the first launch whose valid byte is 1; with M = 1 they are that launch's.
 * fp32 only.  IDH_EINVAL: every condition of idh_binary_mlp_view_fwd that applies, and - with a non-empty map - M <= 0, n_slots <= 0, a NULL
 * key_slots, a slot outside [0, n_slots), a duplicate slot, key_stride < 0, key_stride < B * H * W * feat_cs when n_slots > 1.  IDH_EUNSUPPORTED:
 * M > 16, M * B > 128 (the cameras of a launch sit in LDS: 24 floats per key and batch element, 24 per batch element for the view),
 * n_slots * B * H * W >= 2^31, and the parent's size limits.  The 16-byte loads need feat_ring, feat_cs and key_stride all 16-byte compatible;
 * anything else takes the dword path.  B == 0 or an empty map: IDH_OK, no launch.  Everything is checked on the host before the device is touched. */
int idh_binary_mlp_view_keys_fwd(const float *feat_ring, int feat_cs, int Cf, int B, int H, int W, long long key_stride, int n_slots,
                                 const int *key_slots, int M, const float *rendered_bphw, int P, int h, int w, const float *invK_44,
                                 const float *world_T_cam_44, const float *key_cam_T_world_s44, const float *key_K_s44,
                                 const float *prior_pred_sb1hw, const float *prior_cam_T_world_s44, const float *prior_K_s44, int has_prior,
                                 float prior_const, const float *w1f_packed, const float *w2_packed, const float *vecs6x128, float fill,
                                 float *logits_bphw, unsigned char *key_bphw, float *view_depth_bphw, float *view_points_bphw3, void *stream);
/* Depth in a moving camera against several remembered keyframes, in one launch (view_keys_search_k): idh_binary_mlp_view_search_fwd's rule,
 * step by step, with every step one pixel of idh_binary_mlp_view_keys_fwd on the map rendered = q_n - every step selects its own key.
 * The rings, key_slots and their limits are idh_binary_mlp_view_keys_fwd's; rays, h, w, N, iters, lo, hi, the thresholds and `fill` are
 * idh_binary_mlp_view_search_fwd's.  Per step: thr is keyed by z_sel, by z_0 (key key_slots[0]) when no key is valid; flag bit 2: no key
 * was valid at some probe.  Outputs as the parent's - depth, last_logits, optional flags, optional world points - plus optional key
 * (uint8, any alignment): the sel of step iters - 1, 255 = none.
 * IDH_EINVAL / IDH_EUNSUPPORTED: the conditions of both parents.  B == 0 or an empty grid / list: IDH_OK, no launch. */
int idh_binary_mlp_view_keys_search_fwd(const float *feat_ring, int feat_cs, int Cf, int B, int H, int W, long long key_stride, int n_slots,
                                        const int *key_slots, int M, int h, int w, const float *rays_bn2, int N, const float *invK_44,
                                        const float *world_T_cam_44, const float *key_cam_T_world_s44, const float *key_K_s44,
                                        const float *prior_pred_sb1hw, const float *prior_cam_T_world_s44, const float *prior_K_s44, int has_prior,
                                        float prior_const, const float *w1f_packed, const float *w2_packed, const float *vecs6x128, int iters,
                                        float lo, float hi, float threshold, const float *bins, const float *thr_logits, int n_bins, float fill,
                                        float *depth, float *last_logits, unsigned char *flags, float *points, unsigned char *key, void *stream);
/* First-hit depth in a moving camera, in one launch (view_march_k): the FIRST depth along a ray of the view at which the probe is behind the
 * surface, where idh_binary_mlp_view_search_fwd assumes the one crossing that the reference's search (experiment_modules/bd_model.py:273-292)
 * may assume along the rays of its own camera.  Along a ray of another camera the occlusion seen from the keyframe can be entered, left and
 * entered again, and the ray can leave the keyframe's image part way: bisection then converges on whichever crossing its midpoints fall into.
 * Rays (grid or list form), cameras, prior, network, thresholds and `fill` are idh_binary_mlp_view_search_fwd's; lo / hi / iters are replaced by
 *   march_depths: DEVICE pointer to n_march fp32 samples shared by all rays, 1 <= n_march <= 255.  PRECONDITION, not checked (the host entry
 *                 point cannot read them): finite, positive, strictly increasing
 *   refine:       R >= 0 bisection steps inside the bracket
 * A probe at the view's z-depth q IS one pixel of idh_binary_mlp_view_fwd on rendered = q: steps 1 - 3 of idh_binary_mlp_view_search_fwd (world
 * point by BackprojectDepth, utils/geometry_utils.py:55-63; Project3D, :77-89; validity; nearest prior texel, bd_model.py:405-409; logit = `fill`
 * at an invalid probe, which reads nothing; thr keyed by the probe's keyframe z), verbatim.  A probe is BEHIND when logit < thr, IN FRONT otherwise.
 * Per ray:
 *   march:  probe q_s = march_depths[s], s = 0, 1, ..., and stop at the first s* that is behind.
 *           no s*:    depth = march_depths[n_march-1], flags = bit 1
 *           s* == 0:  depth = march_depths[0], flags = bit 0, no refinement
 *           else:     lo = q_{s*-1}, hi = q_{s*}, flags = bits 0 and 1
 *   refine: R steps at the query (hi + lo) * 0.5f: behind -> hi = query, in front -> lo = query; depth = (hi + lo) * 0.5f after the last step
 *           (bd_model.py:286-290) - with R == 0 the midpoint of the bracket
 *   flag bit 2: some probe the ray EVALUATED was invalid.  Probes a ray never reaches do not exist: they set no flag and read no memory.
 *   `fill` goes through `<`: a `fill` below every threshold makes "outside the keyframe's view" a hit; positive, +inf or NaN marches on.
 * Outputs, (B,h,w) or (B,N): depth; last_logits = the logit of the ray's last evaluated probe; optional (NULL: not written) flags (uint8),
 * hit_step (uint8: s*, 255 = none), points (...,3) = the world point of `depth` by the expressions of the probes.
 * By construction the outputs carry the bits of at most n_march + R launches of idh_binary_mlp_view_fwd on per-ray maps rendered = q with the
 * rule above applied in fp32 between them.  A 16-ray tile skips the gather and the MLP of a step at which none of its unfinished rays has a
 * valid probe, and stops when all of its rays are finished.
 * fp32 only.  IDH_EINVAL: the conditions of idh_binary_mlp_view_search_fwd that apply (all but those on iters, lo, hi), n_march <= 0 or > 255,
 * refine < 0, a NULL or misaligned march_depths.  IDH_EUNSUPPORTED: the parent's limits.  B == 0 or an empty grid / list: IDH_OK, no launch.
 * Everything is checked on the host before the device is touched. */
int idh_binary_mlp_view_march_fwd(const float *feat_nhwc, int feat_cs, int Cf, int B, int H, int W, int h, int w, const float *rays_bn2, int N,
                                  const float *invK_44, const float *world_T_cam_44, const float *key_cam_T_world_44, const float *key_K_44,
                                  const float *prior_pred_b1hw, const float *prior_cam_T_world_44, const float *prior_K_44, int has_prior,
                                  float prior_const, const float *w1f_packed, const float *w2_packed, const float *vecs6x128,
                                  const float *march_depths, int n_march, int refine, float threshold, const float *bins, const float *thr_logits,
                                  int n_bins, float fill, float *depth, float *last_logits, unsigned char *flags, unsigned char *hit_step,
                                  float *points, void *stream);
/* First-hit depth in a moving camera against several remembered keyframes, in one launch (view_keys_march_k): idh_binary_mlp_view_march_fwd's
 * rule with every probe one pixel of idh_binary_mlp_view_keys_fwd on rendered = q - every probe selects the first key in which it is valid,
 * exactly as idh_binary_mlp_view_keys_search_fwd does (Project3D per key, utils/geometry_utils.py:77-89).  thr is keyed by z_sel, by z_0 (key
 * key_slots[0]) when no key is valid; flag bit 2: no key was valid at some evaluated probe.  Outputs as idh_binary_mlp_view_march_fwd's plus
 * optional key (uint8): the sel of the ray's last evaluated probe, 255 = none.
 * IDH_EINVAL / IDH_EUNSUPPORTED: the conditions of both parents.  B == 0 or an empty grid / list: IDH_OK, no launch. */
int idh_binary_mlp_view_keys_march_fwd(const float *feat_ring, int feat_cs, int Cf, int B, int H, int W, long long key_stride, int n_slots,
                                       const int *key_slots, int M, int h, int w, const float *rays_bn2, int N, const float *invK_44,
                                       const float *world_T_cam_44, const float *key_cam_T_world_s44, const float *key_K_s44,
                                       const float *prior_pred_sb1hw, const float *prior_cam_T_world_s44, const float *prior_K_s44, int has_prior,
                                       float prior_const, const float *w1f_packed, const float *w2_packed, const float *vecs6x128,
                                       const float *march_depths, int n_march, int refine, float threshold, const float *bins,
                                       const float *thr_logits, int n_bins, float fill, float *depth, float *last_logits, unsigned char *flags,
                                       unsigned char *hit_step, float *points, unsigned char *key, void *stream);
/* World points -> rays of a view, as Project3D (reference utils/geometry_utils.py:77-89): P = K cam_T_world (fma dots, m = 0..3),
 * c = P[:3] (X, 1) as fma(P0, X0, fma(P1, X1, fma(P2, X2, P3))), depth = max(c_z, 1e-5), (u, v) = c_xy / depth.
 *   points_bn3 (B,N,3); cam_T_world_44, K_44 (B,4,4), K at the resolution H x W the rays are to be in
 *   rays_bn2 (B,N,2) = (u, v); depth_bn (B,N); valid_bn (B,N) uint8 = c_z > 0 && 0 <= u < W && 0 <= v < H
 * Optional prior_pred_b1hw (B,1,H,W) with prior_cam_T_world_44 and prior_K_44 (B,4,4): prior_bn (B,N) is the nearest sample of
 * BDModel.sample_prior (bd_model.py:395-410) with the point projected directly into the prior camera - the same normalise /
 * un-normalise / rintf chain as idh_sample_prior_fwd - and -1 where that camera's z <= 0 or the texel lies outside.
 * IDH_EINVAL: a NULL required pointer, a prior without its matrices or output, negative B or N, H or W <= 0, B > 65535.
 * B == 0 or N == 0: IDH_OK, no launch. */
int idh_project_points_fwd(const float *points_bn3, const float *cam_T_world_44, const float *K_44, int B, int N, int H, int W,
                           float *rays_bn2, float *depth_bn, unsigned char *valid_bn, const float *prior_pred_b1hw,
                           const float *prior_cam_T_world_44, const float *prior_K_44, float *prior_bn, void *stream);

/* ---- evaluation metrics (the step right after the path; rows of the metrics all-gather) ---- */
/* Plane IoU — PlaneEvaluator.compute_batch_scores / compute_batch_scores_test (reference
 * utils/binary_metrics_utils.py:59-192): out[b,d,t,{iou, iou_pos, iou_neg}] over pixels with gt > 0 and
 * query > 0; target = query < gt; prediction = pred > threshold.  Either T (<= 8) constant thresholds
 * (bins == NULL) or the per-depth Thresholder (:42-52): bins (n_bins sorted edges), thresholds has
 * n_bins entries, T must be 1.  Depth metrics — compute_depth_metrics_batched (utils/metrics_utils.py:52-120):
 * out[b, 12] = abs_diff, abs_rel, sq_rel, rmse, rmse_log, a5, a10, a25, a0, a1, a2, a3 over valid_bn != 0.
 * workspace >= idh_metrics_workspace_bytes(B, D, N, T) (8-byte aligned). */
size_t idh_metrics_workspace_bytes(int B, int D, int N, int T);
int idh_plane_iou_fwd(const float *query_depth_bdn, const float *gt_depth_b1n, const float *prediction_bdn,
                      const float *thresholds, int T, const float *bins, int n_bins, int B, int D, int N,
                      float *out_bdt3, void *workspace, size_t workspace_bytes, void *stream);
int idh_depth_metrics_fwd(const float *gt_bn, const float *pred_bn, const unsigned char *valid_bn, int B, int N,
                          int mult_a, float *out_b12, void *workspace, size_t workspace_bytes, void *stream);

/* ---- fused per-frame test evaluation ------------------------------------------------------------------------------------ */
/* What reference test_bd.py:185-318 and test_reg.py:189-268 do between the model outputs at model resolution (h, w) and
 * the per-frame metric rows at ground-truth resolution (H, W), without materialising any (B, P, H, W) tensor:
 *   - get_surface_mask / get_boundary_mask (utils/binary_metrics_utils.py:23-39) at (h, w);
 *   - sigmoid_custom(pred_0, bd_sigmoid_multiplier) (test_bd.py:225-227, modules/layers.py:138);
 *   - F.interpolate of the prediction (bilinear, align_corners=False, or nearest), of the query planes and of the
 *     surface- / boundary-masked query planes (nearest) up to (H, W) (test_bd.py:238-264, test_reg.py:189-233);
 *   - PlaneEvaluator.compute_batch_scores(_test) (binary_metrics_utils.py:59-192) or compute_regressed_depth_batch_scores
 *     (:194-244) for the untagged, "surface" and "boundary" families (test_bd.py:287-318, test_reg.py:235-261);
 *   - compute_depth_metrics_batched (utils/metrics_utils.py:52-120) over an upsampled search_depths or regressed depth
 *     (test_bd.py:266-285, test_reg.py:263-268).
 * Upsampling reproduces PyTorch's legacy nearest (src = min(floor(dst * (float)in / out), in - 1)) and its bilinear
 * source index / tap / lambda order.  IoU counts are integers. */
#define IDH_EVAL_PRED_LOGITS 0 /* prediction = occlusion logits (B,P,h,w); positive when sigmoid(m * logit), upsampled, > threshold */
#define IDH_EVAL_PRED_DEPTH 1  /* prediction = regressed depth (B,1,h,w); positive when query < upsampled depth (T = 1) */
#define IDH_EVAL_BILINEAR 0
#define IDH_EVAL_NEAREST 1      /* temporal_eval */
#define IDH_EVAL_TAG_ALL 1      /* the untagged family (query > 0) */
#define IDH_EVAL_TAG_SURFACE 2  /* query inside the surface mask */
#define IDH_EVAL_TAG_BOUNDARY 4 /* query inside the boundary mask */

/* Host struct, read during the call.  struct_size = sizeof(idh_eval_args) of the caller's header (must be >= the library's). */
typedef struct idh_eval_args {
    int64_t struct_size;
    const float *prediction;    /* see pred_kind */
    int32_t pred_kind;          /* IDH_EVAL_PRED_* */
    int32_t sampling;           /* IDH_EVAL_BILINEAR / IDH_EVAL_NEAREST: how the prediction is upsampled */
    float sigmoid_multiplier;   /* bd_sigmoid_multiplier (logits only) */
    float surface_threshold;    /* get_surface_mask's threshold (0.05) */
    const float *rendered_bphw; /* (B,P,h,w) query planes (cur_data["rendered_depth"]) */
    const float *depth_b1hw;    /* (B,1,h,w) model-resolution depth (cur_data["depth_b1hw"]); NULL when tag_mask == IDH_EVAL_TAG_ALL */
    const float *gt_b1HW;       /* (B,1,H,W) full-resolution ground truth */
    const float *thresholds;    /* logits: T constant thresholds (bins == NULL) or n_bins per-bin thresholds; unused for depth */
    const float *bins;          /* NULL, or the Thresholder's n_bins (<= 8) sorted bin edges (T must be 1) */
    int32_t T;                  /* 1..8 */
    int32_t n_bins;
    int32_t tag_mask;           /* IDH_EVAL_TAG_* bits */
    int32_t B, P, h, w, H, W;
} idh_eval_args;

/* sizeof(idh_eval_args) as compiled into the library. */
size_t idh_sizeof_eval_args(void);
/* Bytes of workspace (8-byte aligned) that idh_eval_plane_scores_fwd and idh_eval_depth_metrics_fwd need at most. */
size_t idh_eval_frame_workspace_bytes(int B, int P, int h, int w, int H, int W, int T);
/* Surface / boundary masks at model resolution: surface_out, boundary_out (B,P,h,w) 0/1 floats as the reference functions
 * return them, code_out (B,P,h,w) bit 0 surface, bit 1 boundary.  Any output may be NULL, not all three.  No workspace. */
int idh_eval_masks_fwd(const float *depth_b1hw, const float *rendered_bphw, int B, int P, int h, int w, float surface_threshold,
                       float *surface_out, float *boundary_out, unsigned char *code_out, void *stream);
/* out[b, tag, d, t, {iou, iou_pos, iou_neg}] (B,3,P,T,3) with tag 0 untagged, 1 surface, 2 boundary (families outside tag_mask are
 * not counted: NaN); counts_out (B,3,P,2+2T) {valid, target, pred[T], inter[T]} or NULL (then they live in the workspace). */
int idh_eval_plane_scores_fwd(const idh_eval_args *args, float *out, unsigned *counts_out, void *workspace, size_t workspace_bytes,
                              void *stream);
/* compute_depth_metrics_batched(gt, upsample(pred_b1hw), gt > valid_above, mult_a): out[b, 12] in the order of idh_depth_metrics_fwd. */
int idh_eval_depth_metrics_fwd(const float *gt_b1HW, const float *pred_b1hw, int B, int h, int w, int H, int W, int sampling,
                               float valid_above, int mult_a, float *out_b12, void *workspace, size_t workspace_bytes, void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* IDH_H_ */
