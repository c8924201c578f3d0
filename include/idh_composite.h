/*
 * idh_composite.h — AR compositing: from the model's outputs to the frame a user sees (added without an ABI version change: nothing existing
 * moved; this surface is versioned through idh_composite_args.struct_size).
 *
 * The reference does this on the CPU with numpy / cv2 (inference/inference.py:117-128, :159-162; inference/composite.py:19-24, :75-143).
 * Two entry points replace it:
 *
 *   idh_prep_rendered_depth_fwd   hole filling (7x7 max-pool into the zero pixels) + nearest resize of the asset's depth render
 *                                 to the model's resolution                                  inference/inference.py:117-128
 *   idh_composite_fwd             sigmoid_custom, bilinear resize to the camera image, soft depth band / hard compare, valid-pixel
 *                                 masking, fade-in, blend, truncation to uint8               inference/inference.py:159-162,
 *                                                                                            inference/composite.py:19-24, :75-143
 *
 * Arithmetic contract of idh_composite_fwd: numpy's dtypes, statement by statement.
 *   rgb = u8 / 255 and alpha = u8 / 255 of the render are fp32 (composite.py:82-84); the resized map, get_mask against a depth MAP, valid and
 *   the matte are fp32; against a PLANE distance get_mask and 1 - mask are fp64 (np.ones((h, w)) * virtual_depth is float64, :131-134) and the
 *   matte is rounded to fp32 once (:137).  im = u8 / 255.0 is fp64, so matte * im, the sum and * 255.0 are fp64 (:138-142);
 *   (1 - matte) * virtual_rgb is an fp32 product with a render (both fp32) and an fp64 product with the constant colour (np.zeros((h, w, 3))
 *   is float64, :86-90).  The result is truncated toward zero to uint8.
 * Resizing is bilinear with half-pixel centres (align_corners = False, no antialiasing), rounded as torch's CPU upsample_bilinear2d rounds a
 * contiguous one-channel map: FMA source index; row-wise FMA blend when H + W > 128 (torch's generic kernel; every camera frame), four weight
 * products accumulated by FMA when H + W <= 128 (torch's vectorised kernel, which it picks by that condition on the OUTPUT size): DESIGN.md
 * §4.9.  The two forms differ by at most 3 ulp of the resized value.  A map that already has the image's size is used as it is.
 *
 * Conventions of include/idh.h: device pointers, dense tensors, caller-owned outputs, `stream` a hipStream_t, asynchronous, no allocation, no
 * synchronisation, no workspace, IDH_OK or a negative IDH_E* code.  Arguments are validated on the host before anything is launched.
 */
#ifndef IDH_COMPOSITE_H_
#define IDH_COMPOSITE_H_

#include <stddef.h>
#include <stdint.h>

#include "idh.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* idh_composite_args.mode: where the matte comes from */
#define IDH_COMPOSITE_MASK_LOGITS 0 /* map = occlusion logits (pred_0): sigmoid_custom(x, multiplier) in the kernel (inference.py:159) */
#define IDH_COMPOSITE_MASK_PROB 1   /* map = occlusion probabilities, as inference.py:162 saved them (composite.py:98-102) */
#define IDH_COMPOSITE_DEPTH_SOFT 2  /* map = regressed / lidar depth, get_mask(soft=True): clip(5 * (pred - virtual + 0.1), 0, 1) (:19-22) */
#define IDH_COMPOSITE_DEPTH_HARD 3  /* map = regressed / lidar depth, get_mask(soft=False): pred > virtual (:24) */

/* Host struct, read during the call.  struct_size = sizeof(idh_composite_args) of the caller's header (must be >= the library's). */
typedef struct idh_composite_args {
    int64_t struct_size;
    const uint8_t *image_bHW3;        /* (B,H,W,3) camera image, RGB (composite.py:76) */
    const uint8_t *virtual_rgba_bHW4; /* (B,H,W,4) render of the asset (:82-84), or NULL with has_colour = 1 */
    const float *map_b1hw;            /* (B,1,h,w) occlusion logits / probabilities or depth, by `mode` */
    const float *virtual_depth_bHW;   /* (B,H,W) depth of the render, 0 = no asset (:121-123); depth modes only, NULL with has_plane = 1 */
    const float *fade_b;              /* (B) multiplied into the valid pixels (:92-94, :124-126), or NULL for 1.0 */
    uint8_t *out_bHW3;                /* (B,H,W,3) composited frame (:138-142) */
    float *matte_out_bHW;             /* (B,H,W) the fp32 matte (:137), or NULL */
    double plane_distance;            /* has_plane: virtual_depth of composite(), matte = 1 - mask without valid pixels or fade (:131-134) */
    double colour[3];                 /* has_colour: constant RGB in [0, 1] (:86-89), valid = 1 (:90) */
    float sigmoid_multiplier;         /* IDH_COMPOSITE_MASK_LOGITS */
    int32_t mode;                     /* IDH_COMPOSITE_* */
    int32_t has_colour;               /* exactly one of virtual_rgba_bHW4 / has_colour */
    int32_t has_plane;                /* depth modes: exactly one of virtual_depth_bHW / has_plane; mask modes: neither */
    int32_t bgr;                      /* write B,G,R (cv2.imwrite's order, :142) instead of R,G,B */
    int32_t B, h, w, H, W;
} idh_composite_args;

/* sizeof(idh_composite_args) as compiled into the library (bindings assert their mirror matches). */
size_t idh_sizeof_composite_args(void);

/* inference/inference.py:117-128.  rendered_b1HW (B,1,Hr,Wr) fp32, 0 = no asset; out_b1hw (B,1,h,w).  Each output pixel takes its nearest source
 * pixel (src = min(floor(dst * in / out), in - 1)); a source value that is exactly 0 is replaced by the maximum over the in-bounds part of its
 * 7x7 neighbourhood (which may still be 0).  Bit-exact.  Hr == h && Wr == w is allowed.
 * IDH_EINVAL: null pointer, B < 0, a size <= 0, Hr * Wr or h * w >= 2^31; IDH_EUNSUPPORTED: B > 65535. */
int idh_prep_rendered_depth_fwd(const float *rendered_b1HW, int B, int Hr, int Wr, int h, int w, float *out_b1hw, void *stream);

/* inference/inference.py:159-162 + inference/composite.py:19-24, :75-143 for B frames.
 * IDH_EINVAL: args NULL, struct_size short, B < 0, a size <= 0, unknown mode, image / map / out NULL, neither or both of render and constant
 * colour, a depth mode with neither or both of virtual depth map and plane distance, a mask mode with either;
 * IDH_EUNSUPPORTED: B * H * W or B * h * w >= 2^31 - 4.  B == 0 is IDH_OK. */
int idh_composite_fwd(const idh_composite_args *args, void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* IDH_COMPOSITE_H_ */
