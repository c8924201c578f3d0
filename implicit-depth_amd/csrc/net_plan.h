// Internal (not exported) interface between the whole-model entry (csrc/model.hip) and the builders / launchers it composes.
// The conv-stage builder of csrc/networks.hip:
// one op list carrying the CVEncoder and the UNet++ decoder (+ DepthDecoderPP heads) with HotPath's level schedule and buffer reuse
// (implicit-depth_amd/pipeline.py HotPath._plan: cost volume -> CVEncoder -> decoder in one nhwc.Plan).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "idh_common.h"
#include "../../include/idh_net.h"

namespace idh_internal {

enum { STAGE_SIZES = 0, STAGE_PACK = 1, STAGE_RUN = 2 };

struct ConvStage {
    // ---- in
    const idh_block_params *enc;  // CVEncoder blocks, 3 per level (idh_cvencoder_fwd order)
    int n_enc;                    // levels
    const idh_block_params *dec;  // IDH_UNETPP_BLOCKS decoder blocks (idh_unetpp_fwd order)
    const idh_conv_params *heads; // NULL (BDDecoderPP) or the four 1x1 heads (DepthDecoderPP)
    unsigned scales;              // bit i: the decoder's output_i result is read (idh_unetpp_fwd_ex); IDH_SCALES_ALL with heads
    int N, H, W, D;               // the volume: (N, H, W, D) NHWC, written by the caller into cv_in before the ops run
    idh_tensor img[5];            // the image-encoder pyramid, IDH_LAYOUT_NCHW (level 0 feeds the decoder, 1..4 the CVEncoder)
    float *const *log_depth;      // heads: 4 dense (N,1,Hi,Wi) outputs (STAGE_RUN)
    float *const *depth;          // heads: exp() of them, may be NULL
    // matching-encoder head (networks.py:279-283) inside the plan, as HotPath with matching_layer1: 0 = none (finished features),
    // 1 = the backbone's layer1 map NCHW (N (K+1), head[0].cin, H, W), 2 = the same channels-last per image
    int head_mode;
    int K;                        // source views: the head runs over N (K+1) images, frame b's current image then its K sources
    const idh_conv_params *head;  // net[5] (1x1) and net[8] (3x3)
    const float *layer1;          // STAGE_RUN, head_mode != 0
    // ---- out
    float *cv_in;                 // the CVEncoder's input buffer (in the workspace)
    int cv_cs;
    const float *feat0;           // the decoder's full-resolution result (BDDecoderPP feature_s0), channel 0
    int feat0_cs, feat0_C, feat0_H, feat0_W;
    const float *match;           // head_mode != 0: the (N, K+1, H, W, C) matching features the head wrote
    int n_head_ops;               // ops of the head segment (run before `before_ops`, the rest after)
    int level_H[5], level_W[5];   // pyramid level sizes the plan expects
    size_t ws_floats, weight_floats;
    uint64_t layout_hash;         // FNV-1a over every op's kind, shape and kernel choice (tile, split-K)
    int ops, launches;
};

// Runs the builder in one of the three modes on (workspace, blob).  STAGE_RUN: `before_ops(ctx)` is called after the op list is built and
// validated, after the head segment and before the rest (the whole-model entry launches the volume kernel there, into s->cv_in).
int conv_stage(int mode, ConvStage *s, float *ws, size_t ws_cap, float *blob, hipStream_t st, int (*before_ops)(void *), void *ctx);

// sample_prior_k with the sigmoid applied on load (csrc/mlp.hip): `logits` (B, Q, H, W) of the previous frame
int sample_prior_from_logits(const float *depth, const float *logits, int Q, const float *cur_world_T_cam, const float *prior_cam_T_world,
                             const float *K, const float *invK, int B, int P, int H, int W, float *out, hipStream_t st);

}  // namespace idh_internal
