// Fused per-frame test evaluation: what reference test_bd.py:185-318 / test_reg.py:189-268 do between the model's
// outputs and the per-frame metric rows, without materialising any full-resolution tensor.
//
//   eval_masks_k     get_surface_mask / get_boundary_mask (utils/binary_metrics_utils.py:23-39) at model resolution,
//                    one 16x64 tile of one (frame, query plane) per workgroup, inputs staged with a 4-pixel halo in LDS.
//                    Writes a per-pixel code (bit 0 surface, bit 1 boundary) and optionally the two float masks.
//   eval_iou3_k      F.interpolate of the prediction / query planes / masked query planes up to the ground-truth
//                    resolution, followed by the three PlaneEvaluator calls (untagged, "surface", "boundary"): one
//                    4096-pixel strip of one frame per workgroup, every query plane in turn, integer counts.
//   eval_depth_partial_k
//                    compute_depth_metrics_batched (utils/metrics_utils.py:52-120) over a prediction upsampled on
//                    the fly (nearest or bilinear).
// Upsampling follows PyTorch's legacy "nearest" (src = min(floor(dst * in/out), in - 1)) and bilinear with
// align_corners=False (area_pixel_compute_source_index, guard_index_and_lambda, the tap / lambda order of
// upsample_bilinear2d), built with -ffp-contract=off.
#include <algorithm>

#include "metrics_common.h"

namespace {

using idh_metrics::kDM;
using idh_metrics::kDmChunk;
using idh_metrics::kMaxThr;

constexpr int kTags = 3;  // untagged, surface, boundary (idh_eval_args.tag_mask bits 0..2)

// ---- masks -------------------------------------------------------------------------------------------------
constexpr int kMTH = 16, kMTW = 64, kHalo = 4;  // halo: 1 for the 3x3 edge pool + 3 for the 7x7 dilation
constexpr int kSH = kMTH + 2 * kHalo, kSW = kMTW + 2 * kHalo;

struct MaskArgs {
    const float *depth;  // (B,1,h,w)
    const float *rend;   // (B,P,h,w)
    int P, h, w, tiles_x;
    float surface_thr;
    float *surface_out;   // (B,P,h,w) or null
    float *boundary_out;  // (B,P,h,w) or null
    unsigned char *code;  // (B,P,h,w) or null
};

__global__ __launch_bounds__(256) void eval_masks_k(const MaskArgs a) {
    __shared__ float sd[kSH][kSW], sr[kSH][kSW];
    __shared__ signed char st[kSH][kSW];              // target = (r < depth), -1 outside the map (max_pool2d's -inf padding)
    __shared__ signed char se[kSH - 2][kSW - 2];      // edges on the 3-pixel ring around the tile, -1 outside the map
    __shared__ signed char sh[kSH - 2][kMTW];         // 7-wide row maximum of se
    const int bp = blockIdx.y, b = bp / a.P;
    const int x0 = (blockIdx.x % a.tiles_x) * kMTW, y0 = (blockIdx.x / a.tiles_x) * kMTH;
    const size_t plane = (size_t)a.h * a.w;
    const float *dep = a.depth + (size_t)b * plane;
    const float *ren = a.rend + (size_t)bp * plane;
    for (int i = threadIdx.x; i < kSH * kSW; i += 256) {
        const int iy = i / kSW, ix = i - iy * kSW;
        const int y = y0 - kHalo + iy, x = x0 - kHalo + ix;
        float d = 0.f, r = 0.f;
        signed char t = -1;
        if (y >= 0 && y < a.h && x >= 0 && x < a.w) {
            d = dep[(size_t)y * a.w + x];
            r = ren[(size_t)y * a.w + x];
            t = r < d;  // false for NaN depth (:25)
        }
        sd[iy][ix] = d;
        sr[iy][ix] = r;
        st[iy][ix] = t;
    }
    __syncthreads();
    // edges = max_pool2d(t, 3, 1, 1) - t, zeroed where depth is NaN (:26-28)
    for (int i = threadIdx.x; i < (kSH - 2) * (kSW - 2); i += 256) {
        const int ey = i / (kSW - 2), ex = i - ey * (kSW - 2);
        const int iy = ey + 1, ix = ex + 1;
        const int t = st[iy][ix];
        int e = -1;
        if (t >= 0) {
            int m = t;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) m = max(m, (int)st[iy + dy][ix + dx]);
            e = m - t;
            if (sd[iy][ix] != sd[iy][ix]) e = 0;
        }
        se[ey][ex] = (signed char)e;
    }
    __syncthreads();
    // separable 7x7 max_pool2d(edges, 7, 1, 3) (:29): rows first
    for (int i = threadIdx.x; i < (kSH - 2) * kMTW; i += 256) {
        const int ry = i / kMTW, ox = i - ry * kMTW;
        int m = -1;
#pragma unroll
        for (int k = 0; k < 7; ++k) m = max(m, (int)se[ry][ox + k]);
        sh[ry][ox] = (signed char)m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kMTH * kMTW; i += 256) {
        const int oy = i / kMTW, ox = i - oy * kMTW;
        const int y = y0 + oy, x = x0 + ox;
        if (y >= a.h || x >= a.w) continue;
        int m = -1;
#pragma unroll
        for (int k = 0; k < 7; ++k) m = max(m, (int)sh[oy + k][ox]);
        const float d = sd[oy + kHalo][ox + kHalo], r = sr[oy + kHalo][ox + kHalo];
        const bool surf = fabsf(d - r) / d < a.surface_thr;  // (:36-38): false for NaN and zero depth
        const bool bnd = m > 0 && !(d != d);                  // NaN where depth is NaN, and NaN > 0 is false (:30-31)
        const size_t o = (size_t)bp * plane + (size_t)y * a.w + x;
        if (a.code) a.code[o] = (unsigned char)(surf | (bnd << 1));
        if (a.surface_out) a.surface_out[o] = surf ? 1.f : 0.f;
        if (a.boundary_out) a.boundary_out[o] = bnd ? 1.f : 0.f;
    }
}

// ---- upsampling helpers --------------------------------------------------------------------------------------
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
    return min((int)floorf((float)dst * scale), in - 1);
}

struct Lin {
    int i0, i1;  // taps (i1 = i0 or i0 + 1)
    float l0, l1;
};

__device__ __forceinline__ Lin linear_src(int dst, float scale, int in) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    Lin r;
    r.i0 = min((int)floorf(src), in - 1);
    r.l1 = fminf(fmaxf(src - (float)r.i0, 0.f), 1.f);
    r.l0 = 1.f - r.l1;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    return r;
}

// sigmoid_custom(logits, m) (modules/layers.py:138, test_bd.py:225-227) once per model-resolution value: the counting pass interpolates
// these instead of evaluating four sigmoids per ground-truth pixel and plane
__global__ __launch_bounds__(256) void eval_sigmoid_k(const float *__restrict__ x, float m, long long n, float *__restrict__ y) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) y[i] = 1.f / (1.f + expf(-m * x[i]));
}

// ---- plane IoU at ground-truth resolution ----------------------------------------------------------------------
constexpr int kStrip = 4096;  // ground-truth pixels per workgroup (16 per thread per plane)

enum PredMode { kSigBilinear = 0, kSigNearest = 1, kRegBilinear = 2, kRegNearest = 3 };

struct Iou3Args {
    const float *pred;          // sigmoid(m * logits) (B,P,h,w) or regressed depth (B,1,h,w)
    const float *rend;          // (B,P,h,w) query planes
    const unsigned char *code;  // (B,P,h,w) mask codes, or null when only the untagged family is counted
    const float *gt;            // (B,1,H,W)
    const float *thr;           // T constant thresholds, or nb per-bin thresholds when bins != null
    const float *bins;
    int nb, T, tag_mask;
    int P, h, w, H, W;
    float sy, sx;               // (float)h / H, (float)w / W
    unsigned *counts;           // (B, 3, P, 2 + 2T): valid, target, pred[T], inter[T]
};

// NT: the most thresholds this instance counts (1 for the Thresholder and the regressed compare, kMaxThr for constant thresholds)
template <int MODE, int NT>
__global__ __launch_bounds__(256) void eval_iou3_k(const Iou3Args a) {
    constexpr bool kReg = MODE >= kRegBilinear, kBil = MODE == kSigBilinear || MODE == kRegBilinear;
    __shared__ float sg[kStrip];
    __shared__ float sbin[kMaxThr], sthr[kMaxThr];
    __shared__ unsigned red[4][kTags * (kMaxThr + 1)];
    const int b = blockIdx.y;
    const int N = a.H * a.W;
    const int i0 = blockIdx.x * kStrip, n = min(kStrip, N - i0);
    const float *g = a.gt + (size_t)b * N + i0;
    for (int k = threadIdx.x; k < n; k += 256) sg[k] = g[k];
    if (threadIdx.x < kMaxThr) {
        sbin[threadIdx.x] = a.bins && (int)threadIdx.x < a.nb ? a.bins[threadIdx.x] : 0.f;
        sthr[threadIdx.x] = a.thr && (int)threadIdx.x < (a.bins ? a.nb : a.T) ? a.thr[threadIdx.x] : 0.f;
    }
    __syncthreads();
    const size_t plane = (size_t)a.h * a.w;
    const bool tagged = a.code != nullptr;
    const int T = NT == 1 ? 1 : a.T;
    for (int d = 0; d < a.P; ++d) {
        const float *q = a.rend + ((size_t)b * a.P + d) * plane;
        const float *pp = a.pred + (kReg ? (size_t)b : (size_t)b * a.P + d) * plane;
        const unsigned char *cd = tagged ? a.code + ((size_t)b * a.P + d) * plane : nullptr;
        // two 16-bit counters per word: [valid | target], [pred_t | inter_t]; a wave counts at most 64 * 16 pixels
        unsigned c[kTags][NT + 1];
#pragma unroll
        for (int tg = 0; tg < kTags; ++tg)
#pragma unroll
            for (int t = 0; t <= NT; ++t) c[tg][t] = 0;
        int y = (i0 + (int)threadIdx.x) / a.W, x = (i0 + (int)threadIdx.x) - y * a.W;
        for (int k = threadIdx.x; k < n; k += 256, x += 256) {
            while (x >= a.W) { x -= a.W; ++y; }
            const float gd = sg[k];
            const int ny = nearest_src(y, a.sy, a.h), nx = nearest_src(x, a.sx, a.w);
            const float qd = q[(size_t)ny * a.w + nx];
            if (!(gd > 0.f && qd > 0.f)) continue;  // valid mask (binary_metrics_utils.py:143-145); NaN gt is invalid too
            const unsigned code = tagged ? cd[(size_t)ny * a.w + nx] : 0u;
            float pv;
            if (kBil) {
                const Lin ly = linear_src(y, a.sy, a.h), lx = linear_src(x, a.sx, a.w);
                const float v00 = pp[(size_t)ly.i0 * a.w + lx.i0], v01 = pp[(size_t)ly.i0 * a.w + lx.i1];
                const float v10 = pp[(size_t)ly.i1 * a.w + lx.i0], v11 = pp[(size_t)ly.i1 * a.w + lx.i1];
                pv = ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
            } else {
                pv = pp[(size_t)ny * a.w + nx];
            }
            const unsigned tgt = qd < gd;
            unsigned pr = 0;  // bit t: prediction positive at threshold t
            if (kReg) {
                pr = qd < pv;  // compute_regressed_depth_batch_scores (:212)
            } else if (a.bins) {  // thresholds[bucketize(query, bins)] (:49-51, right=False); beyond the last edge: last threshold
                int lo = 0, hi = a.nb;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (sbin[mid] < qd) lo = mid + 1; else hi = mid; }
                if (lo >= a.nb) lo = a.nb - 1;
                pr = pv > sthr[lo];
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < T) pr |= (unsigned)(pv > sthr[t]) << t;
            }
            // the surface / boundary families differ only in validity: the reference writes -1 into their query (test_bd.py:250-264)
            const unsigned in_tag[kTags] = {1u, code & 1u, (code >> 1) & 1u};
#pragma unroll
            for (int tg = 0; tg < kTags; ++tg) {
                const unsigned v = in_tag[tg];
                c[tg][0] += v | ((v & tgt) << 16);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const unsigned p = v & (pr >> t) & 1u;
                    c[tg][1 + t] += p | ((p & tgt) << 16);
                }
            }
        }
        // wave reduce, then one integer atomic per counter per workgroup
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
        for (int tg = 0; tg < kTags; ++tg)
#pragma unroll
            for (int t = 0; t <= NT; ++t) {
                if (t > T) continue;
                unsigned v = c[tg][t];
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) red[wave][tg * (kMaxThr + 1) + t] = v;
            }
        __syncthreads();
        if (threadIdx.x < 2 * kTags * (kMaxThr + 1)) {
            const int half = threadIdx.x & 1, j = threadIdx.x >> 1;
            const int tg = j / (kMaxThr + 1), t = j - tg * (kMaxThr + 1);
            if (t <= T && ((a.tag_mask >> tg) & 1)) {
                unsigned s = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) s += (red[w][j] >> (16 * half)) & 0xffffu;
                // word 0 -> valid (lo) / target (hi); word 1 + t -> pred[t] (lo) / inter[t] (hi)
                const int slot = t == 0 ? half : (half ? 2 + T + (t - 1) : 2 + (t - 1));
                if (s) atomicAdd(a.counts + (((size_t)b * kTags + tg) * a.P + d) * (2 + 2 * T) + slot, s);
            }
        }
        __syncthreads();
    }
}

// out[b, tag, d, t, {iou, iou_pos, iou_neg}]
__global__ void eval_iou_finalise_k(const unsigned *__restrict__ counts, int n_bd, int T, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_bd * T) return;
    const int bd = i / T, t = i - bd * T;
    const unsigned *c = counts + (size_t)bd * (2 + 2 * T);
    idh_metrics::iou_from_counts(c[0], c[1], c[2 + t], c[2 + T + t], out + (size_t)i * 3);
}

// ---- depth metrics over an upsampled prediction ---------------------------------------------------------------
template <bool BILINEAR>
__global__ __launch_bounds__(256) void eval_depth_partial_k(const float *__restrict__ gt, const float *__restrict__ pred, int h, int w,
                                                            int H, int W, float sy, float sx, float valid_above, int nchunks,
                                                            double *__restrict__ part) {
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int N = H * W;
    const int i0 = chunk * kDmChunk, i1 = min(N, i0 + kDmChunk);
    const float *g = gt + (size_t)b * N;
    const float *p = pred + (size_t)b * h * w;
    double s[kDM + 1];
    for (int k = 0; k <= kDM; ++k) s[k] = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const float gd = g[i];
        if (!(gd > valid_above)) continue;  // valid_mask_b = gt > thresh_to_check (test_bd.py:274-275, test_reg.py:196-197)
        const int y = i / W, x = i - y * W;
        float pv;
        if (BILINEAR) {
            const Lin ly = linear_src(y, sy, h), lx = linear_src(x, sx, w);
            const float v00 = p[(size_t)ly.i0 * w + lx.i0], v01 = p[(size_t)ly.i0 * w + lx.i1];
            const float v10 = p[(size_t)ly.i1 * w + lx.i0], v11 = p[(size_t)ly.i1 * w + lx.i1];
            pv = ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
        } else {
            pv = p[(size_t)nearest_src(y, sy, h) * w + nearest_src(x, sx, w)];
        }
        idh_metrics::depth_metric_terms(gd, pv, s);
    }
    idh_metrics::depth_metric_block_store(s, part + ((size_t)b * nchunks + chunk) * (kDM + 1));
}

__global__ void eval_depth_finalise_k(const double *__restrict__ part, int nchunks, int mult_a, float *__restrict__ out) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= kDM) return;
    out[(size_t)b * kDM + k] = idh_metrics::depth_metric_finalise(part, b, nchunks, k, mult_a);
}

// ---- host side ---------------------------------------------------------------------------------------------
size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

size_t counts_bytes(long long B, long long P, long long T) { return (size_t)(B * kTags * P * (2 + 2 * T)) * sizeof(unsigned); }

size_t depth_part_bytes(long long B, long long H, long long W) {
    return (size_t)(B * ((H * W + kDmChunk - 1) / kDmChunk) * (kDM + 1)) * sizeof(double);
}

bool shapes_ok(int B, int P, int h, int w, int H, int W) {
    return B >= 0 && P > 0 && h > 0 && w > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) && (long long)h * w < (1ll << 31);
}

int launch_masks(const float *depth, const float *rend, int B, int P, int h, int w, float thr, float *surf, float *bnd, unsigned char *code,
                 hipStream_t st) {
    MaskArgs m{depth, rend, P, h, w, idh_cdiv(w, kMTW), thr, surf, bnd, code};
    hipLaunchKernelGGL(eval_masks_k, dim3(m.tiles_x * idh_cdiv(h, kMTH), B * P), dim3(256), 0, st, m);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

}  // namespace

extern "C" size_t idh_sizeof_eval_args(void) { return sizeof(idh_eval_args); }

extern "C" size_t idh_eval_frame_workspace_bytes(int B, int P, int h, int w, int H, int W, int T) {
    if (!shapes_ok(B, P, h, w, H, W) || B == 0 || T <= 0 || T > kMaxThr) return 0;
    const size_t plane = align256(counts_bytes(B, P, T)) + align256((size_t)B * P * h * w * sizeof(float)) + align256((size_t)B * P * h * w);
    const size_t depth = align256(depth_part_bytes(B, H, W));
    return plane > depth ? plane : depth;
}

extern "C" int idh_eval_masks_fwd(const float *depth_b1hw, const float *rendered_bphw, int B, int P, int h, int w, float surface_threshold,
                                  float *surface_out, float *boundary_out, unsigned char *code_out, void *stream) {
    if (B < 0 || P <= 0 || h <= 0 || w <= 0 || (long long)h * w >= (1ll << 31)) return IDH_EINVAL;
    if (B == 0) return IDH_OK;
    if (!depth_b1hw || !rendered_bphw || !(surface_out || boundary_out || code_out)) return IDH_EINVAL;
    if ((long long)B * P > 65535) return IDH_EUNSUPPORTED;
    return launch_masks(depth_b1hw, rendered_bphw, B, P, h, w, surface_threshold, surface_out, boundary_out, code_out, idh_stream(stream));
}

extern "C" int idh_eval_plane_scores_fwd(const idh_eval_args *args, float *out, unsigned *counts_out, void *workspace, size_t workspace_bytes,
                                         void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_eval_args)) return IDH_EINVAL;
    const idh_eval_args &e = *args;
    if (!shapes_ok(e.B, e.P, e.h, e.w, e.H, e.W)) return IDH_EINVAL;
    const bool reg = e.pred_kind == IDH_EVAL_PRED_DEPTH;
    if (!reg && e.pred_kind != IDH_EVAL_PRED_LOGITS) return IDH_EINVAL;
    if (e.sampling != IDH_EVAL_BILINEAR && e.sampling != IDH_EVAL_NEAREST) return IDH_EINVAL;
    if (e.T <= 0 || e.T > kMaxThr || (reg && (e.T != 1 || e.bins))) return IDH_EINVAL;
    if (e.bins && (e.T != 1 || e.n_bins <= 0 || e.n_bins > kMaxThr)) return IDH_EINVAL;
    if (e.tag_mask <= 0 || e.tag_mask > 7) return IDH_EINVAL;
    const bool tagged = (e.tag_mask & (IDH_EVAL_TAG_SURFACE | IDH_EVAL_TAG_BOUNDARY)) != 0;
    if (e.B == 0) return IDH_OK;
    if (!e.prediction || !e.rendered_bphw || !e.gt_b1HW || !out || (!reg && !e.thresholds) || (tagged && !e.depth_b1hw)) return IDH_EINVAL;
    // workspace: [counts unless counts_out | sigmoid(m * logits) unless regressed | mask codes when tagged]
    const size_t cbytes = counts_out ? 0 : align256(counts_bytes(e.B, e.P, e.T));
    const size_t n_lo = (size_t)e.B * e.P * e.h * e.w;
    const size_t sbytes = reg ? 0 : align256(n_lo * sizeof(float));
    const size_t need = cbytes + sbytes + (tagged ? align256(n_lo) : 0);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7)) return IDH_EWORKSPACE;
    if ((long long)e.B * e.P > 65535) return IDH_EUNSUPPORTED;
    hipStream_t st = idh_stream(stream);
    unsigned *counts = counts_out ? counts_out : static_cast<unsigned *>(workspace);
    float *sig = reg ? nullptr : reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + cbytes);
    unsigned char *code = tagged ? static_cast<unsigned char *>(workspace) + cbytes + sbytes : nullptr;
    if (hipMemsetAsync(counts, 0, counts_bytes(e.B, e.P, e.T), st) != hipSuccess) return IDH_ELAUNCH;
    if (tagged) {
        const int r = launch_masks(e.depth_b1hw, e.rendered_bphw, e.B, e.P, e.h, e.w, e.surface_threshold, nullptr, nullptr, code, st);
        if (r != IDH_OK) return r;
    }
    if (!reg) {
        hipLaunchKernelGGL(eval_sigmoid_k, dim3((unsigned)std::min<size_t>((n_lo + 255) / 256, 4096)), dim3(256), 0, st, e.prediction,
                           e.sigmoid_multiplier, (long long)n_lo, sig);
        IDH_CHECK_LAUNCH();
    }
    Iou3Args a{reg ? e.prediction : sig, e.rendered_bphw, code, e.gt_b1HW, reg ? nullptr : e.thresholds, e.bins, e.bins ? e.n_bins : 0, e.T,
               e.tag_mask, e.P, e.h, e.w, e.H, e.W, (float)e.h / e.H, (float)e.w / e.W, counts};
    const dim3 grid(idh_cdiv((long long)e.H * e.W, kStrip), e.B);
    const bool nearest = e.sampling == IDH_EVAL_NEAREST, one = e.T == 1;
    if (reg)
        hipLaunchKernelGGL((nearest ? eval_iou3_k<kRegNearest, 1> : eval_iou3_k<kRegBilinear, 1>), grid, dim3(256), 0, st, a);
    else if (one)
        hipLaunchKernelGGL((nearest ? eval_iou3_k<kSigNearest, 1> : eval_iou3_k<kSigBilinear, 1>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((nearest ? eval_iou3_k<kSigNearest, kMaxThr> : eval_iou3_k<kSigBilinear, kMaxThr>), grid, dim3(256), 0, st, a);
    IDH_CHECK_LAUNCH();
    const long long n = (long long)e.B * kTags * e.P * e.T;
    hipLaunchKernelGGL(eval_iou_finalise_k, dim3(idh_cdiv(n, 128)), dim3(128), 0, st, counts, e.B * kTags * e.P, e.T, out);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_eval_depth_metrics_fwd(const float *gt_b1HW, const float *pred_b1hw, int B, int h, int w, int H, int W, int sampling,
                                          float valid_above, int mult_a, float *out_b12, void *workspace, size_t workspace_bytes,
                                          void *stream) {
    if (!shapes_ok(B, 1, h, w, H, W) || (sampling != IDH_EVAL_BILINEAR && sampling != IDH_EVAL_NEAREST)) return IDH_EINVAL;
    if (B == 0) return IDH_OK;
    if (!gt_b1HW || !pred_b1hw || !out_b12) return IDH_EINVAL;
    const int nchunks = idh_cdiv((long long)H * W, kDmChunk);
    if (!workspace || workspace_bytes < depth_part_bytes(B, H, W) || ((uintptr_t)workspace & 7)) return IDH_EWORKSPACE;
    if (B > 65535) return IDH_EUNSUPPORTED;
    hipStream_t st = idh_stream(stream);
    double *part = static_cast<double *>(workspace);
    const float sy = (float)h / H, sx = (float)w / W;
    if (sampling == IDH_EVAL_BILINEAR)
        hipLaunchKernelGGL(eval_depth_partial_k<true>, dim3(nchunks, B), dim3(256), 0, st, gt_b1HW, pred_b1hw, h, w, H, W, sy, sx, valid_above, nchunks, part);
    else
        hipLaunchKernelGGL(eval_depth_partial_k<false>, dim3(nchunks, B), dim3(256), 0, st, gt_b1HW, pred_b1hw, h, w, H, W, sy, sx, valid_above, nchunks, part);
    IDH_CHECK_LAUNCH();
    hipLaunchKernelGGL(eval_depth_finalise_k, dim3(B), dim3(64), 0, st, part, nchunks, mult_a, out_b12);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
