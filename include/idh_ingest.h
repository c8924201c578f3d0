/*
 * idh_ingest.h — frame ingest: from a camera's uint8 frame and uint16 depth to the tensors the model reads (added without an ABI version
 * change: nothing existing moved; this surface is versioned through the struct_size of its argument structs).
 *
 * The reference does this in its dataset code on the CPU with Pillow and torchvision (datasets/generic_mvs_dataset.py:560-634,
 * utils/generic_utils.py:149-214, datasets/scannet_dataset.py:490-561).  Entry points:
 *
 *   idh_resize_coeffs_sizes / _pack   Pillow's resampling coefficients of one dimension, host only      Image.resize (generic_utils.py:210)
 *   idh_ingest_color_fwd              antialiased resize + to_tensor + ImageNet normalisation           generic_utils.py:149-152, :210-212
 *   idh_ingest_depth_fwd              NEAREST resize, * value_scale, validity masks, NaN where invalid   scannet_dataset.py:515-530, :550-561
 *
 * Arithmetic contract: the resize is Pillow's 8-bit one, byte for byte.  Per dimension, in C doubles: scale = in / out,
 * filterscale = max(scale, 1), support = S * filterscale (S = 1 bilinear, 2 bicubic with a = -0.5), ksize = 2 * ceil(support) + 1;
 * for output index i: center = (i + 0.5) * scale, first = max((int)(center - support + 0.5), 0),
 * count = min((int)(center + support + 0.5), in) - first, taps filter((k + first - center + 0.5) / filterscale) divided by their sum and
 * converted as (int)(+-0.5 + tap * 2^22).  A pass accumulates in int32 from 1 << 21, shifts right by 22 and clips to 0..255; the horizontal
 * pass runs first, its result IS uint8, and a pass whose dimension does not change is skipped.  The floats are u8 / 255 and then
 * (x - mean) / std in IEEE fp32, which is what torch's CPU to_tensor / normalize compute.  Nothing is cropped: read_image_file drops the
 * result of crop_image_to_target_ratio (generic_utils.py:195-196).
 *
 * Conventions of include/idh.h: device pointers, dense tensors, caller-owned outputs, `stream` a hipStream_t, asynchronous, no allocation, no
 * synchronisation, no workspace, IDH_OK or a negative IDH_E* code.  Arguments are validated on the host before anything is launched.
 */
#ifndef IDH_INGEST_H_
#define IDH_INGEST_H_

#include <stddef.h>
#include <stdint.h>

#include "idh.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define IDH_RESIZE_BILINEAR 0 /* PIL.Image.BILINEAR: scannet, hypersim */
#define IDH_RESIZE_BICUBIC 1  /* PIL.Image.BICUBIC: arkit, vdr, 7scenes, colmap, scanniverse */

#define IDH_INGEST_MAX_RATIO 8 /* in <= 8 * out per dimension (4032x3024 -> 512x384 is 7.875): at most 33 bicubic taps */

/* Image.resize's coefficients for one dimension (generic_utils.py:210).  Host only, no GPU call.
 * n_bounds = 2 * out int32: (first source index, tap count) per output index; n_taps = out * ksize int32: the fixed-point taps of output
 * index i at taps[i * ksize ..], zero past its count.
 * IDH_EINVAL: in or out <= 0, unknown filter, null pointer; IDH_EUNSUPPORTED: in > IDH_INGEST_MAX_RATIO * out. */
int idh_resize_coeffs_sizes(int in, int out, int filter, int64_t *n_bounds, int64_t *n_taps);
int idh_resize_coeffs_pack(int in, int out, int filter, int32_t *bounds_out, int32_t *taps_out);

/* Host struct, read during the call.  struct_size = sizeof(idh_ingest_color_args) of the caller's header (must be >= the library's). */
typedef struct idh_ingest_color_args {
    int64_t struct_size;
    const uint8_t *frames_bHW3; /* (B,Hs,Ws,3) camera frames, RGB */
    const int32_t *x_bounds;    /* idh_resize_coeffs_pack(Ws, w, filter) on the device; NULL exactly when Ws == w (pass skipped) */
    const int32_t *x_taps;
    const int32_t *y_bounds;    /* idh_resize_coeffs_pack(Hs, h, filter) on the device; NULL exactly when Hs == h */
    const int32_t *y_taps;
    float *image_b3hw;          /* (B,3,h,w) to_tensor + normalisation (generic_utils.py:212, :149-152), or NULL */
    uint8_t *resized_bhw3;      /* (B,h,w,3) Pillow's resized bytes (:210), or NULL; at least one output */
    int32_t filter;             /* IDH_RESIZE_*: fixes the row length (ksize) of the tap tables */
    int32_t normalize;          /* 0: image = u8 / 255 only (to_tensor); else (u8 / 255 - mean) / std with the ImageNet statistics */
    int32_t B, Hs, Ws, h, w;
} idh_ingest_color_args;

/* Host struct, read during the call.  One launch writes the target-size triple, the full-resolution triple, or both, from one source. */
typedef struct idh_ingest_depth_args {
    int64_t struct_size;
    const uint16_t *depth_bHW;  /* (B,Hs,Ws) depth in integer units (millimetres) */
    float *depth_b1hw;          /* (B,1,h,w) NEAREST resize * value_scale, NaN where invalid (scannet_dataset.py:515-528); NULL: no target-size triple */
    float *mask_b1hw;           /* (B,1,h,w) 1.0 where valid (:525) */
    uint8_t *mask_b_b1hw;       /* (B,1,h,w) bool, one byte each (:524) */
    float *full_depth_b1HW;     /* (B,1,Hs,Ws) the same at the source's resolution (:550-559); NULL: no full-resolution triple */
    float *full_mask_b1HW;
    uint8_t *full_mask_b_b1HW;
    float value_scale;          /* depth = (float)v * value_scale in fp32 (generic_utils.py:212) */
    float min_valid, max_valid; /* valid = depth > min_valid && depth < max_valid */
    int32_t B, Hs, Ws, h, w;    /* h, w are read only with a target-size triple; h == Hs && w == Ws copies */
} idh_ingest_depth_args;

/* sizeof of the two structs as compiled into the library (bindings assert their mirrors match). */
size_t idh_sizeof_ingest_color_args(void);
size_t idh_sizeof_ingest_depth_args(void);

/* utils/generic_utils.py:210-212 + :149-152 for B frames, one launch, no intermediate image in device memory.  Bit-exact.
 * The tables are read as data: indices and counts are clamped to the source, so a wrong table gives wrong pixels, never an access outside
 * the frames.
 * IDH_EINVAL: args NULL, struct_size short, B < 0, a size <= 0, unknown filter, frames NULL, both outputs NULL, a table missing for a
 * dimension that changes or given for one that does not; IDH_EUNSUPPORTED: Hs > 8 * h or Ws > 8 * w, B > 65535, h > 8 * 65535,
 * Hs * Ws or h * w >= 2^29.  B == 0 is IDH_OK. */
int idh_ingest_color_fwd(const idh_ingest_color_args *args, void *stream);

/* datasets/scannet_dataset.py:515-530 and :550-561 for B frames.  Source index of output index i: (int)((i + 0.5) * ((double)in / out)),
 * Pillow's NEAREST.  Bit-exact.
 * IDH_EINVAL: args NULL, struct_size short, B < 0, a size <= 0, depth NULL, no triple requested, a triple with one of its three outputs
 * NULL; IDH_EUNSUPPORTED: B * Hs * Ws or B * h * w >= 2^31 - 4.  B == 0 is IDH_OK. */
int idh_ingest_depth_fwd(const idh_ingest_depth_args *args, void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* IDH_INGEST_H_ */
