/*
 * idh_model.h — whole-model entry points: BDModel.forward / DepthModel.forward from the matching features onwards (ABI 106).
 *
 *   idh_model_fwd   replaces pipeline.HotPath.forward   experiment_modules/bd_model.py:221-304, depth_model.py:378-433
 *                   (+ the temporal loop of inference/inference.py:139-157 as a device-side frame chain)
 *
 * One call enqueues the whole forward on the caller's stream: the matching-encoder head on the backbone's layer1 map (or the NCHW import of
 * finished matching features), the cost / feature volume written
 * straight into the CVEncoder's input buffer, the CVEncoder + UNet++ decoder as ONE op list (csrc/networks.hip, the same kernel selection,
 * split-K, level schedule and buffer reuse as nhwc.Plan inside HotPath, so results are bit-identical to it), the DepthDecoderPP heads, and for
 * a BDModel the temporal prior warp and the occlusion MLP over the query planes (or the 12-step per-pixel depth search).  It allocates
 * nothing, synchronises nothing and reads nothing back to the host, so it can be captured in a graph.
 *
 * Conventions of include/idh_net.h: device pointers, caller-owned weight blob / workspace / outputs (256-byte aligned blob and workspace),
 * fp32 throughout, 0 or a negative IDH_E* code, never throws.
 *
 *   idh_model_sizes(desc, B, &sizes)   host only: blob and workspace sizes and the plan key of (ABI, desc, B, every conv's kernel choice)
 *   idh_model_pack(desc, params, B, blob, stream)
 *                                     fills the blob from the reference's raw parameters (what a state_dict gives a C host)
 *   idh_model_fwd(desc, blob, weight_floats, plan_key, B, inputs, outputs, ws, ws_floats, stream)
 *                                     validates everything on the host before it launches anything: a plan_key / weight_floats that
 *                                     are not those of (desc, B) -> IDH_EINVAL (a blob packed for another shape is never read); a short
 *                                     workspace -> IDH_EWORKSPACE; an output range that overlaps an input, another output, the blob or
 *                                     the workspace -> IDH_EINVAL.
 *
 * Covered: volume FEATURE_MLP (K <= 8 source views, C = 16) or DOT (C = 16 / 32), D a multiple of 16, the CVEncoder of four levels, the
 * UNet++ decoders; matching input = finished NCHW features, or the backbone's layer1 map (NCHW or channels-last), whose encoder head
 * (networks.py:279-283) then runs inside the same op list.  IDH_EUNSUPPORTED: the zero volume, skip decoders, f16x3 math, matching_scale != 1,
 * other C / K.
 */
#ifndef IDH_MODEL_H_
#define IDH_MODEL_H_

#include <stddef.h>
#include <stdint.h>

#include "idh_net.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define IDH_MODEL_BD 0    /* BDModel: occlusion MLP over query planes */
#define IDH_MODEL_DEPTH 1 /* DepthModel: DepthDecoderPP 1x1 log-depth heads */

#define IDH_VOLUME_FEATURE_MLP 0 /* mlp_feature_volume (FeatureVolumeManager) */
#define IDH_VOLUME_DOT 1         /* simple_cost_volume (CostVolumeManager) */
#define IDH_VOLUME_ZERO 2        /* ZeroCostVolumeManager: IDH_EUNSUPPORTED */

#define IDH_MATCH_FEATS_NCHW 0   /* finished matching features, NCHW */
#define IDH_MATCH_LAYER1_NCHW 1  /* the matching backbone's layer1 map, dense NCHW: the encoder head runs inside the call (its 1x1 conv reads the map in place) */
#define IDH_MATCH_LAYER1_NHWC 2  /* the same map channels-last per image ((B (K+1), H, W, 64) dense) */

#define IDH_QUERY_PLANES 0     /* occlusion logits of P rendered-depth planes per frame */
#define IDH_QUERY_SEARCH 1     /* infer_depth: per-pixel binary search, constant threshold */
#define IDH_QUERY_SEARCH_THR 2 /* infer_depth with the Thresholder table (bins + thresholds in idh_model_params) */

#define IDH_PRIOR_NONE 0   /* a prior-enabled MLP sees the constant -1 (bd_model.py:433-434) */
#define IDH_PRIOR_WARPED 1 /* inputs.prior: an already-warped (B, P, H0, W0) prior channel */
#define IDH_PRIOR_INPUTS 2 /* inputs.prior_prediction & co: warped here by sample_prior (bd_model.py:395-431) */
#define IDH_PRIOR_CHAIN 3  /* the B batch entries are consecutive frames of one sequence: frame b's prior is frame b-1's sigmoid(pred_0),
                              warped on the device; frame 0 starts from inputs.prior_prediction / prior_cam_T_world (or none) */

typedef struct idh_model_params idh_model_params;

typedef struct idh_model_desc {
    int32_t kind;           /* IDH_MODEL_* */
    int32_t volume;         /* IDH_VOLUME_* */
    int32_t K, C, D;        /* source views, matching channels, depth planes */
    int32_t H, W;           /* matching resolution (the volume's); the decoder's top level and the query planes are (H0, W0) = (2H, 2W) */
    int32_t P;              /* query planes per frame (IDH_QUERY_PLANES; also the planes of rendered_depth for the prior warp) */
    int32_t use_prior;      /* the occlusion MLP's first Linear has a prior column */
    int32_t matching_input; /* IDH_MATCH_* */
    int32_t query;          /* IDH_QUERY_* (BD) */
    int32_t prior_mode;     /* IDH_PRIOR_* (BD) */
    int32_t n_thr_bins;     /* IDH_QUERY_SEARCH_THR: entries of the Thresholder table */
    int32_t search_iters;   /* infer_depth: 12 */
    float search_lo, search_hi, search_threshold; /* 0.5, 8.0, 0.5 */
    float min_depth, max_depth;                    /* the log-spaced depth planes (bd_model.py:226-229) */
    int32_t matching_scale; /* must be 1 */
    int32_t math;           /* 0 = fp32 MFMA; anything else (f16x3) -> IDH_EUNSUPPORTED */
    int32_t skip_decoder;   /* != 0 -> IDH_EUNSUPPORTED */
    int32_t return_mask;    /* FEATURE_MLP: write outputs.overall_mask */
    const idh_model_params *net; /* the architecture: the shape fields of the conv stack (cout / cin / ks / stride) are read by all three
                                    calls; the parameter POINTERS only by idh_model_pack */
} idh_model_desc;

/* The reference's raw parameters, reference layout (nn.Linear: (out, in) row-major + bias; nn.Conv2d: OIHW + bias). */
struct idh_model_params {
    idh_block_params cv_blocks[12];  /* CVEncoder: ds_conv_i, conv_i[0], conv_i[1], i = 0..3 (idh_cvencoder_fwd order) */
    idh_block_params dec_blocks[IDH_UNETPP_BLOCKS]; /* UNet++ decoder blocks (idh_unetpp_fwd order) */
    idh_conv_params depth_heads[4];  /* DEPTH: output_i[1], the 1x1 log-depth heads */
    idh_conv_params match_head[2];   /* IDH_MATCH_LAYER1_*: matching encoder net[5] (1x1, 64 -> 128) / net[8] (3x3, 128 -> C) */
    const float *fv_w[3], *fv_b[3];  /* FEATURE_MLP: cost_volume.mlp.net[0 / 2 / 4] weight / bias (128 x (C(K+1)+10K+4), 128 x 128, 1 x 128) */
    const float *mlp_w[3], *mlp_b[3];/* BD: binary_mlp.mlps["s0"][0 / 2 / 4] weight / bias (128 x (1 + F [+ 1]), 128 x 128, 1 x 128) */
    const float *thr_bins, *thr_values; /* IDH_QUERY_SEARCH_THR: Thresholder.bins / .thresholds (n_thr_bins each, thresholds in (0, 1)) */
};

typedef struct idh_model_inputs {
    const float *matching_cur;      /* (B, C, H, W) NCHW */
    const float *matching_src;      /* (B, K, C, H, W) */
    const float *matching_layer1;   /* IDH_MATCH_LAYER1_*: (B, K+1, 64, H, W): frame b's current image, then its K source images */
    const float *pyramid[5];        /* the image encoder's five maps, dense NCHW, level i at (2H / 2^i, 2W / 2^i) */
    const float *src_cam_T_cur_cam; /* (B, K, 4, 4) */
    const float *cur_cam_T_src_cam; /* (B, K, 4, 4) */
    const float *src_K;             /* (B, K, 4, 4) */
    const float *cur_invK;          /* (B, 4, 4) */
    const float *rendered_depth;    /* BD: (B, P, H0, W0) query depths (also what the prior warp projects) */
    const float *prior;             /* IDH_PRIOR_WARPED: (B, P, H0, W0) (the search reads plane 0) */
    const float *prior_prediction;  /* IDH_PRIOR_INPUTS: (B, prior_channels, H0, W0) probabilities; CHAIN: (1, prior_channels, H0, W0) or NULL */
    int32_t prior_channels;
    const float *prior_cam_T_world; /* IDH_PRIOR_INPUTS: (B, 4, 4); CHAIN: (1, 4, 4), NULL with prior_prediction */
    const float *world_T_cam;       /* IDH_PRIOR_INPUTS / CHAIN: (B, 4, 4) */
    const float *cam_T_world;       /* CHAIN: (B, 4, 4), the frames' poses */
    const float *K_s0, *invK_s0;    /* IDH_PRIOR_INPUTS / CHAIN: (B, 4, 4) */
} idh_model_inputs;

typedef struct idh_model_outputs {
    float *pred_0;         /* BD: (B, P, H0, W0) logits [search: (B, 1, H0, W0), the last evaluation] */
    float *search_depths;  /* IDH_QUERY_SEARCH*: (B, 1, H0, W0) */
    float *prior_mask;     /* optional: the warped prior (B, P, H0, W0) (PRIOR_INPUTS; CHAIN with a start prior) */
    float *log_depth[4];   /* DEPTH: (B, 1, H0 / 2^i, W0 / 2^i) "log_depth_pred_s{i}_b1hw" */
    float *depth[4];       /* DEPTH, optional: exp() of them */
    float *lowest_cost;    /* (B, H, W) "lowest_cost_bhw" */
    uint8_t *overall_mask; /* FEATURE_MLP with desc.return_mask: (B, H, W) 0 / 1 bytes */
    float *prior_out;      /* CHAIN: (1, P, H0, W0) = sigmoid(pred_0 of frame B-1): the next call's prior_prediction */
} idh_model_outputs;

typedef struct idh_model_size_info {
    size_t weight_floats;
    size_t workspace_floats;
    uint64_t plan_key;
    int32_t conv_ops;      /* idh_op descriptors of the conv stage (CVEncoder + decoder) */
    int32_t conv_launches; /* their kernel launches (idh_count_launches) */
} idh_model_size_info;

int idh_model_sizes(const idh_model_desc *desc, int B, idh_model_size_info *sizes);
int idh_model_pack(const idh_model_desc *desc, const idh_model_params *params, int B, float *weight_blob, void *stream);
int idh_model_fwd(const idh_model_desc *desc, const float *weight_blob, size_t weight_floats, uint64_t plan_key, int B,
                  const idh_model_inputs *inputs, const idh_model_outputs *outputs, float *workspace, size_t workspace_floats, void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
