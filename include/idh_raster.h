/*
 * idh_raster.h — depth-only mesh rasterisation and the vertex bookkeeping of the temporal evaluation (added without an ABI version change: nothing existing moved).
 * The shaded render of an asset in a live camera - depth, winning face, barycentrics, attributes, lit RGBA - follows, and the warp of
 * keyframe depth maps into a live camera is at the end of the file.
 *
 * Under --temporal_eval the reference (test_bd.py:109-116, 157-183, 214-236; utils/binary_metrics_utils.py:247-388) renders a
 * 1024 x 1024-vertex plane and the scene's ground-truth mesh into every frame with pytorch3d's CUDA rasteriser, samples the
 * prediction at every projected ground-truth vertex and counts how often a vertex's occlusion decision flips between frames.
 * The three *_fwd entry points replace those three steps (idh_raster_workspace_bytes sizes the first one's workspace):
 *
 *   idh_raster_depth_fwd                 Pytorch3DRasterizer.render_depth                 binary_metrics_utils.py:336-358
 *   idh_vertex_predictions_fwd           Pytorch3DRasterizer.update_gt_vertex_predictions binary_metrics_utils.py:360-388 (after its render)
 *   idh_vertex_occlusion_changes_fwd     TemporalEvaluator.compute_vertex_occlusion_changes binary_metrics_utils.py:273-280
 *
 * Rasterisation semantics
 *   - camera point X_c = R X_w + t from cam_T_world; OpenCV intrinsics fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2];
 *   - pixel (row i, col j) samples the ray through image point (u, v) = (j + 0.5, i + 0.5): direction ((u - cx) / fx, (v - cy) / fy, 1)
 *     (pytorch3d's convention behind cameras_from_opencv_projection: pixel centres at half-integers of the screen);
 *   - the output is the smallest camera-space z > 0 over all triangles the ray hits (faces_per_pixel = 1, blur_radius = 0,
 *     perspective-correct: the ray / triangle intersection depth), both windings, -1 where nothing is hit;
 *   - the ray test runs in camera space, so a triangle that straddles z = 0 is drawn correctly for its z > 0 part (pytorch3d does not
 *     clip such triangles; geometric correctness is the definition chosen here); triangles wholly at z <= 0 are skipped;
 *   - an edge shared by two triangles is evaluated from its lower-numbered vertex in both, so the two see exactly negated values and
 *     a pixel centre on the edge is covered by at least one of them (>= 0 is inside);
 *   - zero-area triangles, faces with an index outside [0, V) and non-finite vertices contribute nothing.
 * The z-buffer is resolved with a 32-bit unsigned atomic minimum on the float's bit pattern: the result does not depend on the order
 * in which triangles arrive and is bit-reproducible from run to run.
 *
 * Conventions of include/idh.h: device pointers, dense fp32 (faces int32), caller-owned outputs and workspace, `stream` a hipStream_t,
 * asynchronous, IDH_OK or a negative IDH_E* code.  Arguments are validated on the host before anything is launched.
 */
#ifndef IDH_RASTER_H_
#define IDH_RASTER_H_

#include <stddef.h>
#include <stdint.h>

#include "idh.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* Bytes of workspace (256-byte aligned) idh_raster_depth_fwd needs for V vertices and F faces in B cameras: the camera-space and
 * screen-space vertices (24 B per vertex and camera) and the queue of large triangles (4 B per face and camera).  0 for bad arguments. */
size_t idh_raster_workspace_bytes(int B, int V, int F);

/* verts_v3 (V,3) fp32 world space; faces_f3 (F,3) int32 (may be NULL when F == 0: every pixel is then -1);
 * cam_T_world_b44, K_b44 (B,4,4) row-major; out_b1hw (B,1,H,W) also serves as the z-buffer.
 * IDH_EINVAL: null pointer, B < 0, V < 0, F < 0, H <= 0, W <= 0, H * W >= 2^31; IDH_EWORKSPACE: workspace null, misaligned or short;
 * IDH_EUNSUPPORTED: B > 65535 or B * H * W >= 2^31. */
int idh_raster_depth_fwd(const float *verts_v3, int V, const int32_t *faces_f3, int F, const float *cam_T_world_b44,
                         const float *K_b44, int B, int H, int W, float *out_b1hw, void *workspace, size_t workspace_bytes,
                         void *stream);

/* Per vertex: camera-space z and screen position (x_s, y_s) = (fx x / z + cx, fy y / z + cy); the nearest sample
 * (grid_sample(mode="nearest", align_corners=False, zero padding): column nearbyint(x_s - 0.5), row nearbyint(y_s - 0.5), 0 outside)
 * of pred_11hw and of the visibility render depth_11hw (both (1,1,H,W)); valid = depth_s > 0 && z > 0 && |z - depth_s| < depth_tolerance
 * && pred_s > 0 (the reference's 0.05); out_v[v] = pred_s where valid, else -1.  One camera (4,4), as the reference's batch of 1. */
int idh_vertex_predictions_fwd(const float *verts_v3, int V, const float *cam_T_world_44, const float *K_44, const float *pred_11hw,
                               const float *depth_11hw, int H, int W, float depth_tolerance, float *out_v, void *stream);

/* hist_tv (T,V): the stacked per-frame vertex predictions.  -1 and NaN are "unknown", > 0.5 -> 1, < 0.5 -> 0, exactly 0.5 stays 0.5;
 * *half_units_out (one int64 on the device) = 2 * sum over t, v of |p[t+1,v] - p[t,v]| ignoring pairs with an unknown: the flips
 * counted exactly in units of 0.5.  T < 2 or V == 0 gives 0. */
int idh_vertex_occlusion_changes_fwd(const float *hist_tv, int T, int V, long long *half_units_out, void *stream);

/* ---- shaded render: depth, winning face, barycentrics, interpolated attributes and lit RGBA in one call (additive: idh_version()
 * stays as it is; this surface is versioned through idh_raster_shaded_args.struct_size; csrc/raster_shade.hip) --------
 *
 * Geometry, culls and the edge rule are exactly those of idh_raster_depth_fwd above.  Visibility is resolved on one 64-bit key per pixel,
 *   key = ((uint64)float_bits(z) << 32) | face_index,        empty: float_bits(+inf) << 32 | 0xffffffff,
 * with a 64-bit unsigned atomic minimum.  z is the fp32 value idh_raster_depth_fwd computes for that face and pixel, so the upper word of
 * the final key is, bit for bit, that entry point's depth; among faces with the same fp32 z at a pixel the lowest face index wins.  No
 * output depends on the order in which faces arrive: two renders are bit-identical.
 *
 * The shade pass, one lane per pixel, then redoes the triangle setup of the winning face alone.  With camera-space corners A, B, C
 * (vertices face[0], face[1], face[2]), the pixel's ray d = ((j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy, 1) and the plane normal N signed so
 * that N.A > 0, all in fp32 without contraction:
 *   e0 = d.(B x C), e1 = d.(C x A), e2 = d.(A x B)            (the edge functions of the coverage test, same expressions)
 *   s = e0 + e1 + e2;  w_i = e_i / s  if s > 0, else w = (1/3, 1/3, 1/3)
 * These are the barycentrics of the 3D hit point (perspective-correct: no 1 / z correction is involved in camera space).
 *   depth        upper key word; `empty_depth` where nothing is hit
 *   pix_to_face  lower key word; -1 where nothing is hit
 *   bary         w_0, w_1, w_2; zeros where nothing is hit
 *   attr_out[c]  w_0 * a0[c] + w_1 * a1[c] + w_2 * a2[c], summed in this order, a_i = attrs_vc[face[i]]; zeros where nothing is hit
 *   rgba         per channel v = w_0 * (float)c0 + w_1 * (float)c1 + w_2 * (float)c2 from colors_v4[face[i]]; R, G and B are multiplied by
 *                ambient + (1 - ambient) * lam, lam = d.N / sqrtf((N.N) * (d.d))  (a headlight at the camera on the face's own normal,
 *                two-sided; ambient = 1 is unlit); alpha is not lit; stored as (uint8)(fminf(fmaxf(v, 0), 255) + 0.5f).
 *                (0, 0, 0, 0) where nothing is hit: alpha 0 is "no asset" for idh_composite_fwd's virtual_rgba_bHW4. */
typedef struct idh_raster_shaded_args {
    int64_t struct_size;          /* sizeof(idh_raster_shaded_args) of the caller's header (must be >= the library's) */
    const float *verts_v3;        /* (V,3) fp32, the space cam_T_world maps from */
    const int32_t *faces_f3;      /* (F,3); may be NULL when F == 0 (every pixel is then empty) */
    const float *cam_T_world_b44; /* (B,4,4) row-major */
    const float *K_b44;           /* (B,4,4) */
    const uint8_t *colors_v4;     /* (V,4) RGBA per vertex, or NULL */
    const float *attrs_vc;        /* (V,C) fp32 per vertex, or NULL */
    float *depth_b1hw;            /* outputs: each may be NULL (not written), at least one must be given */
    int32_t *pix_to_face_bhw;     /* (B,H,W) */
    float *bary_bhw3;             /* (B,H,W,3) */
    float *attr_out_bhwc;         /* (B,H,W,C); needs attrs_vc */
    uint8_t *rgba_bhw4;           /* (B,H,W,4); needs colors_v4 */
    void *workspace;              /* 256-byte aligned, idh_raster_shaded_workspace_bytes(B, V, F, H, W) */
    int64_t workspace_bytes;
    float ambient;                /* in [0, 1] */
    float empty_depth;            /* written to depth where nothing is hit (idh_raster_depth_fwd writes -1) */
    int32_t V, F, B, H, W, C;     /* C: channels of attrs_vc, 1..16 (0 without attrs_vc) */
} idh_raster_shaded_args;

/* sizeof(idh_raster_shaded_args) as compiled into the library (bindings assert their mirror matches). */
size_t idh_sizeof_raster_shaded_args(void);

/* Bytes of workspace (256-byte aligned): what idh_raster_workspace_bytes(B, V, F) counts plus the key plane, 8 B per pixel and camera.
 * 0 for bad arguments (a negative count, H <= 0, W <= 0). */
size_t idh_raster_shaded_workspace_bytes(int B, int V, int F, int H, int W);

/* Validated on the host before anything is launched.
 * IDH_EINVAL: args NULL, struct_size short, B < 0, V < 0, F < 0, H <= 0, W <= 0, H * W >= 2^31, C < 0 or C > 16, attrs_vc with C == 0,
 * ambient not finite or outside [0, 1]; then (B > 0) a null verts (V > 0) / faces (F > 0) / cam_T_world / K, no output requested,
 * attr_out without attrs_vc, rgba without colors_v4; IDH_EWORKSPACE: workspace null, misaligned or short;
 * IDH_EUNSUPPORTED: B > 65535 or B * H * W >= 2^31.  B == 0 is IDH_OK. */
int idh_raster_shaded_fwd(const idh_raster_shaded_args *args, void *stream);

/* ---- depth reprojection: M keyframe depth maps warped into B live cameras (additive: idh_version() stays as it is; versioned through
 * idh_depth_warp_args.struct_size; csrc/depth_warp.hip) -------------------------------------------------------------
 *
 * The depth path of the reference's compositor (inference/composite.py:104-134: the `predicted_depth` and `lidar` methods, fed with
 * depth_pred_s0_b1hw of the regression baseline or a sensor's map) takes a depth map in the camera it composites into.  This entry
 * point moves maps predicted or measured at keyframes into the camera of any frame between them.
 *
 * Each source map m (h x w, inverse intrinsics src_invK[m]) is a triangulated surface:
 *   - vertex (i, j) = depth[m, i, j] * src_invK[m][:3,:3] (j + 0.5, i + 0.5, 1)   (BackprojectDepth, utils/geometry_utils.py:39,60-61),
 *     taken into target camera b by cam_T_src[b, m]; it is valid when its depth is finite and > 0;
 *   - quad q = i * (w - 1) + j, 0 <= i < h - 1, 0 <= j < w - 1, with corners v00 = (i, j), v01 = (i, j + 1), v10 = (i + 1, j),
 *     v11 = (i + 1, j + 1) gives face 2q = (v00, v10, v01) and face 2q + 1 = (v01, v10, v11); vertex numbers i * w + j order shared edges;
 *   - a face draws when its three vertices are valid and zmax <= zmin * tear_ratio over its three SOURCE depths (one fp32 multiply and
 *     one compare); tear_ratio = +inf never tears;
 *   - everything else is idh_raster_depth_fwd's rule: the ray / plane intersection in the target camera's space, >= 0 is inside, both
 *     windings, a face crossing z = 0 is drawn for its front part.
 * All M sources of a target go into one z-buffer of 64-bit keys (float_bits(z) << 32) | (m * 2 (h - 1) (w - 1) + face), resolved with
 * a 64-bit unsigned atomic minimum:
 *   depth   the smallest target-camera z over all faces of all sources; `empty_depth` where nothing is hit
 *   source  m * 2 (h - 1) (w - 1) + face of the winner, the lowest among equal depths; -1 where nothing is hit
 * Two calls return the same bits.  Where pixel centres fall exactly on mesh vertices (the identity pose, an integer zoom) coverage is
 * decided by rounding and single-pixel holes can appear. */
typedef struct idh_depth_warp_args {
    int64_t struct_size;         /* sizeof(idh_depth_warp_args) of the caller's header (must be >= the library's) */
    const float *depth_m1hw;     /* (M,1,h,w) source depth maps */
    const float *src_invK_m44;   /* (M,4,4) inverse intrinsics of the sources at h x w, row-major */
    const float *cam_T_src_bm44; /* (B,M,4,4) source camera frame -> target camera frame */
    const float *K_b44;          /* (B,4,4) target intrinsics at H x W */
    float *depth_b1hw;           /* out (B,1,H,W) */
    int32_t *source_bhw;         /* out (B,H,W), or NULL */
    void *workspace;             /* 256-byte aligned, idh_depth_warp_workspace_bytes(B, M, h, w, H, W) */
    int64_t workspace_bytes;
    float tear_ratio;            /* >= 1; +inf: the rubber sheet */
    float empty_depth;           /* written to depth where nothing is hit */
    int32_t B, M, h, w, H, W;
} idh_depth_warp_args;

/* sizeof(idh_depth_warp_args) as compiled into the library (bindings assert their mirror matches). */
size_t idh_sizeof_depth_warp_args(void);

/* Bytes of workspace (256-byte aligned): 4 B per face and (target, source) pair for the queue of large faces, 8 B per target pixel for
 * the key plane.  0 for bad sizes (any <= 0, h < 2, w < 2). */
size_t idh_depth_warp_workspace_bytes(int B, int M, int h, int w, int H, int W);

/* Validated on the host before anything is launched.
 * IDH_EINVAL: args NULL, struct_size short, B, M, H or W <= 0, h < 2, w < 2, tear_ratio < 1 or NaN, a null
 * input or depth_b1hw; IDH_EUNSUPPORTED: h * w >= 2^30, M * 2 (h - 1) (w - 1) >= 2^31, B * H * W >= 2^31, B * M > 65535;
 * IDH_EWORKSPACE: workspace null, misaligned or short (the code every entry point of the library gives a short workspace). */
int idh_depth_warp_fwd(const idh_depth_warp_args *args, void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* IDH_RASTER_H_ */
