// Arithmetic shared by the evaluation-metric kernels of metrics.hip and eval_frame.hip: the IoU of the
// reference's PlaneEvaluator from integer counts, and compute_depth_metrics_batched's per-pixel terms and
// per-frame finalise.  Both files must produce the same numbers from the same counts / sums.
#pragma once
#include "idh_common.h"

namespace idh_metrics {

constexpr int kMaxThr = 8;
constexpr int kDM = 12;  // abs_diff abs_rel sq_rel rmse rmse_log a5 a10 a25 a0 a1 a2 a3
constexpr int kDmChunk = 4096;

// {iou, iou_pos, iou_neg} from (valid, target, pred, inter) counts with the reference's float arithmetic
// (utils/binary_metrics_utils.py:88-100; 0/0 -> NaN kept)
__device__ inline void iou_from_counts(unsigned cv, unsigned ct, unsigned cp, unsigned ci, float *o3) {
    const float nv = (float)cv, nt = (float)ct, np = (float)cp, ni = (float)ci;
    const float pos = ni / (nt + np - ni);
    const float nn_t = nv - nt, nn_p = nv - np, nn_i = nv - nt - np + ni;  // counts of the negated masks
    const float neg = nn_i / (nn_t + nn_p - nn_i);
    o3[0] = 2.f * (pos * neg) / (pos + neg);
    o3[1] = pos;
    o3[2] = neg;
}

// one valid pixel's terms of utils/metrics_utils.py:52-120, added to s[0..kDM] (s[kDM] counts pixels)
__device__ inline void depth_metric_terms(float g, float p, double *s) {
    const float d = g - p;
    const float th = fmaxf(g / p, p / g);
    const float lg = logf(g) - logf(p);
    s[0] += fabsf(d); s[1] += fabsf(d) / g; s[2] += d * d / g; s[3] += d * d; s[4] += lg * lg;
    s[5] += th < 1.05f; s[6] += th < 1.10f; s[7] += th < 1.25f; s[8] += th < 1.10f; s[9] += th < 1.25f;
    s[10] += th < 1.25f * 1.25f; s[11] += th < 1.25f * 1.25f * 1.25f;
    s[12] += 1.0;
}

// block of 256: reduce the per-thread sums and write the chunk's kDM + 1 partials
__device__ inline void depth_metric_block_store(double *s, double *part_chunk) {
    __shared__ double red[4][kDM + 1];
    for (int k = 0; k <= kDM; ++k) {
        double v = s[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x <= kDM) part_chunk[threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// metric k of frame b from the chunk partials (fixed order, double): nanmean over the valid pixels, sqrt for the
// two rmse terms, x100 for the ratios when mult_a
__device__ inline float depth_metric_finalise(const double *part, int b, int nchunks, int k, int mult_a) {
    double s = 0.0, n = 0.0;
    for (int c = 0; c < nchunks; ++c) {
        s += part[((size_t)b * nchunks + c) * (kDM + 1) + k];
        n += part[((size_t)b * nchunks + c) * (kDM + 1) + kDM];
    }
    double m = s / n;  // 0/0 -> NaN like torch.nanmean of an all-NaN row
    if (k == 3 || k == 4) m = sqrt(m);
    if (k >= 5 && mult_a) m *= 100.0;
    return (float)m;
}

}  // namespace idh_metrics
