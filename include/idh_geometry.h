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

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* IDH_GEOMETRY_H_ */
