// Occlusion MLP at sparse rays, and the projection of world points to such rays (gfx950, fp32 MFMA).
//
// Fused form of the reference's ray path  BDModel.run_mlp_train (experiment_modules/bd_model.py:313-393):
//     sampled_rays (B,N,2) in pixel-centre units of the supervision grid -> (x / grid_w - 0.5) * 2            (:325-326)
//     for each scale s: rays[:, ::(s+1)], depths[:, ::(s+1)]                                                   (:352-353)
//         F.grid_sample(feature_s, rays, bilinear, zeros, align_corners=False) -> expand over the S samples    (:357-364)
//         cat([depth | feature | (prior)]) -> permute -> BinaryMLPNetwork                                      (:367-384)
// i.e. a (B, N, S, 1 + Cf) tensor per scale.  Here the feature row of a ray is blended from its four corner rows of the NHWC map
// straight into the MFMA B-operand registers, pre1 = W1f . feat + b1 is formed once per ray, and the S depth samples run through
// the same register-resident loop as the planes of binary_mlp_k (csrc/mlp.hip): one ray per column instead of one pixel.
//
// The exact fp32 expression of the gather is stated in include/idh.h (tests/ray_query_ref.py derives its bound from it).
//
// ray_search_k is the same text with the sample loop replaced by the binary depth search of binary_mlp_k (BDModel.forward(infer_depth=True),
// bd_model.py:273-292): lo / hi / query / flags of a ray live in the registers of its four quarter-lanes, which see the same reduced logit
// and so stay in step; the final query is back-projected to a camera- or world-space hit point (BackprojectDepth, geometry_utils.py:39,60-61).
//
// view_mlp_k is the same text again with the rays drawn from a depth map in another camera: a ray is one pixel (b, p, row, col) of
// rendered (B,P,h,w); it is back-projected with that view's invK / world_T_cam (BackprojectDepth, geometry_utils.py:55-63), projected into
// the keyframe's scale-0 map with the expression of project_points_k below (Project3D, :77-89) and asked at its keyframe z, S = 1, with the
// nearest sample of a prior prediction (bd_model.py:405-409) when there is one.  Rays, depth, valid and prior never reach HBM.
//
// view_search_k is the search of ray_search_k along the rays of another camera: the query is the z-depth in THAT camera, so the sample point
// moves across the keyframe's image from step to step and every step is one whole view_mlp_k pixel (back-projection, projection, validity,
// prior texel, gather, W1f . f, MLP) at rendered = q_n; an invalid probe's logit is `fill`.  The threshold is keyed by the probe's keyframe z.
//
// view_keys_k / view_keys_search_k are those two with the projection looped over M remembered keyframes (a ring of feature maps, cameras and
// priors, indexed by slot): the world point is projected into key_slots[0..M-1] in turn, the first key in which it is valid is selected, and
// the prior texel, the four corners and the MLP are those of the selected key alone - one MLP pass per pixel whatever M is.
//
// view_march_k / view_keys_march_k are view_search_k / view_keys_search_k with the bracket found instead of assumed: every ray probes the
// shared samples march_depths[0 .. n_march-1] in turn until the first probe that is behind the surface, then bisects `refine` steps inside
// [previous sample, that sample].  Rays of a tile finish at different steps: a finished ray rides along as an invalid probe with its state frozen.
#include <algorithm>
#include <cfloat>
#include <tuple>
#include <type_traits>

#include "idh_common.h"
#include "mlp_common.h"

namespace {

using namespace idh_mlp;

// (the host value-initialises an argument block and sets its fields by name - set_* in the host section: what a mode does not name is zero or null)
struct RayArgs {
    const float *feat;   // NHWC rows, B*H*W x cs
    const float *rays;   // B,N,2
    const float *depth;  // B,N,S
    const float *prior;  // B,N,S or null
    const float *w1f, *w2, *vecs;  // as BinArgs of csrc/mlp.hip
    float *out;          // B,Nq,S
    int M, Nq, N, S, ray_step;  // M = B * Nq rays of this launch
    int H, W, cs, Cf;
    float grid_w, grid_h;
    int has_prior;
    float prior_const;
    int feat_unaligned;  // 1: rows are not 16-byte aligned, dword loads
    int nchunk, s_chunk;  // the S samples of a ray tile are cut into nchunk runs of s_chunk: one work item (= one wave pass) each
    // ray_search_k only (S = 1, ray_step = 1, nchunk = 1; `prior` is (B,N), `out` the logits of the last evaluation):
    int iters;
    float lo, hi, thr_logit;
    const float *bins, *thr_logits;  // per-depth Thresholder: n_bins sorted edges, logit(threshold) per bin; n_bins = 0: thr_logit
    int n_bins;
    float *sdepth;         // B,N final queries
    unsigned char *flags;  // B,N or null: bit 0 = hi moved, bit 1 = lo moved
    float *points;         // B,N,3 or null
    const float *invK, *wTc;  // B,4,4; wTc may be null (camera-space points)
    // view_mlp_k only (S = 1, ray_step = 1, nchunk = 1, Nq = N = vP * vh * vw, grid = (H, W)): `depth` is rendered (B,vP,vh,vw), invK / wTc
    // the VIEW's (both required), `prior` a (B,1,H,W) map or null, `flags` valid or null, `sdepth` the keyframe z or null, `points` or null
    const float *key_cTw, *key_K;      // B,4,4: the keyframe's cam_T_world and K at H x W
    const float *prior_cTw, *prior_K;  // B,4,4, with a prior map
    int nb, vP, vh, vw;                // nb = B
    float fill;
    // view_search_k: view_mlp_k's cameras, prior and fill with ray_search_k's iters / lo / hi / thresholds and outputs; there is no `depth`;
    // `rays` (B,N,2) in pixel-centre units of the VIEW, or null: the vh x vw grid of its pixel centres (vP = 1, Nq = N = vh * vw);
    // `points` are world points; flags gain bit 2 = some probe was invalid
};

// view_keys_k / view_keys_search_k: `feat`, `key_cTw`, `key_K`, `prior`, `prior_cTw`, `prior_K` are rings indexed by slot - the features of
// slot s start at feat + s * key_stride, the matrices are (n_slots,B,4,4), the prior maps (n_slots,B,1,H,W).  A separate struct: the four
// single-key kernels keep their argument block as it is.  On the host keys_args checks and fills these fields; set_common reads key_stride.
constexpr int kMaxKeys = 16;
struct KeysArgs : RayArgs {
    long long key_stride;     // floats between the feature blocks of two slots
    int nkeys;                // M <= kMaxKeys keys, asked in this order
    int key_slots[kMaxKeys];  // their slots
    unsigned char *keyout;    // view_keys_search_k: the key of the last step (position in key_slots, 255 = none) or null; view_keys_k writes it to `flags`
};

// view_march_k / view_keys_march_k: view_search_k's / view_keys_search_k's arguments without iters / lo / hi, plus the march.  Derived structs:
// the six kernels above keep their argument blocks as they are.
template <class Base>
struct MarchArgsT : Base {
    const float *march_depths;  // n_march samples shared by all rays: finite, positive, strictly increasing (the caller's precondition)
    int n_march, refine;        // 1 <= n_march <= 255, refine >= 0
    unsigned char *hit_step;    // the first sample that is behind, 255 = none, or null
};
using MarchArgs = MarchArgsT<RayArgs>;
using KeysMarchArgs = MarchArgsT<KeysArgs>;

enum { kSamples = 0, kSearch = 1, kView = 2, kViewSearch = 3, kViewKeys = 4, kViewKeysSearch = 5, kViewMarch = 6, kViewKeysMarch = 7, kRayModes = 8 };
constexpr int kKeyCamFloats = 24;  // per (key, batch) in LDS: P = K cam_T_world (12), the prior camera's (12); then per batch rows 0-2 of the view's invK (12) and world_T_cam (12)
constexpr int kViewMaxBatch = 128;  // 24 KiB of cameras next to at most 96 KiB of weights
constexpr int kCamFloats = 48;  // per batch in LDS: P = K cam_T_world (12), the prior camera's (12), rows 0-2 of the view's invK (12) and world_T_cam (12)

constexpr int kRayMaxThreads = 768;  // 12 waves, as binary_mlp_k; small launches use 4 (ray_mlp_launch)
constexpr int kW1LdsMaxBlocks = 4;   // Cf <= 64 -> W1f in LDS, as binary_mlp_k
#ifndef IDH_VIEW_SEARCH_SKIP
#define IDH_VIEW_SEARCH_SKIP 1
#endif
constexpr bool kViewSearchSkip = IDH_VIEW_SEARCH_SKIP;  // view_search_k: skip gather and MLP of a step at which no ray of the tile has a valid probe

// kSamples: the S depth samples of `depth`; kSearch: `iters` dependent evaluations at the ray's current search depth; kView: one evaluation
// per pixel of a depth map seen from another camera; kViewSearch: `iters` dependent kView evaluations along a ray of that other camera;
// kViewMarch: at most n_march + refine dependent kView evaluations along such a ray, first the shared samples, then the bisection of the bracket
template <int kMode, class Args = RayArgs>
__device__ __forceinline__ void ray_body(const Args &a) {
    constexpr bool kKeys = kMode == kViewKeys || kMode == kViewKeysSearch || kMode == kViewKeysMarch;
    constexpr bool kMarch = kMode == kViewMarch || kMode == kViewKeysMarch;
    constexpr bool kDense = kMode == kView || kMode == kViewKeys;  // one evaluation per pixel of a depth map
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int nthreads = blockDim.x, nwaves = nthreads >> 6;
    f32x4 *sW2 = reinterpret_cast<f32x4 *>(smem_raw);
    const int cblocks = (a.Cf + 15) >> 4;
    const bool w1_lds = cblocks <= kW1LdsMaxBlocks;
    f32x4 *sW1 = sW2 + kNS * kNS * 64;
    float *s_vec = reinterpret_cast<float *>(sW1 + (w1_lds ? cblocks * kNS * 64 : 0));
    {
        const f32x4 *g2 = reinterpret_cast<const f32x4 *>(a.w2), *g1 = reinterpret_cast<const f32x4 *>(a.w1f);
        for (int i = threadIdx.x; i < kNS * kNS * 64; i += nthreads) sW2[i] = g2[i];
        if (w1_lds)
            for (int i = threadIdx.x; i < cblocks * kNS * 64; i += nthreads) sW1[i] = g1[i];
        for (int i = threadIdx.x; i < 6 * kHidden; i += nthreads) s_vec[i] = a.vecs[i];
    }
    float *s_cam = s_vec + 6 * kHidden;
    if constexpr (kKeys) {
        // P = K cam_T_world of every key (and of its prior camera), once per workgroup, key and batch: the fma loop of project_points_k
        for (int t = threadIdx.x; t < 2 * a.nkeys * a.nb; t += nthreads) {
            const int mb = t >> 1, pc = t & 1;
            if (pc && !a.prior) continue;
            const int m = mb / a.nb, b = mb - m * a.nb;
            const size_t cam_i = ((size_t)a.key_slots[m] * a.nb + b) * 16;
            const float *Kb = (pc ? a.prior_K : a.key_K) + cam_i, *T = (pc ? a.prior_cTw : a.key_cTw) + cam_i;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) {
                    float s = 0.f;
                    for (int k = 0; k < 4; ++k) s = fmaf(Kb[i * 4 + k], T[k * 4 + j], s);
                    s_cam[mb * kKeyCamFloats + 12 * pc + i * 4 + j] = s;
                }
        }
        float *s_view = s_cam + a.nkeys * a.nb * kKeyCamFloats;
        for (int t = threadIdx.x; t < 24 * a.nb; t += nthreads) {  // rows 0-2 of the view's invK and world_T_cam, as they are
            const int b = t / 24, e = t - b * 24;
            s_view[t] = (e < 12 ? a.invK : a.wTc)[(size_t)b * 16 + (e < 12 ? e : e - 12)];
        }
    } else if constexpr (kMode == kView || kMode == kViewSearch || kMode == kViewMarch) {
        // P = K cam_T_world of the keyframe (and of the prior camera), once per workgroup and batch: the fma loop of project_points_k
        for (int t = threadIdx.x; t < 2 * a.nb; t += nthreads) {
            const int b = t >> 1, pc = t & 1;
            if (pc && !a.prior) continue;
            const float *Kb = (pc ? a.prior_K : a.key_K) + (size_t)b * 16, *T = (pc ? a.prior_cTw : a.key_cTw) + (size_t)b * 16;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) {
                    float s = 0.f;
                    for (int m = 0; m < 4; ++m) s = fmaf(Kb[i * 4 + m], T[m * 4 + j], s);
                    s_cam[b * kCamFloats + 12 * pc + i * 4 + j] = s;
                }
        }
        for (int t = threadIdx.x; t < 24 * a.nb; t += nthreads) {  // rows 0-2 of the view's invK and world_T_cam, as they are
            const int b = t / 24, e = t - b * 24;
            s_cam[b * kCamFloats + 24 + e] = (e < 12 ? a.invK : a.wTc)[(size_t)b * 16 + (e < 12 ? e : e - 12)];
        }
    }
    __syncthreads();
    const float *s_b1 = s_vec, *s_wd = s_vec + kHidden, *s_wp = s_vec + 2 * kHidden, *s_b2 = s_vec + 3 * kHidden,
                *s_w3 = s_vec + 4 * kHidden;
    const float b3 = s_vec[5 * kHidden];

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ln = lane & 15, q = lane >> 4;
    const int tiles = (a.M + 15) >> 4;
    const int items = tiles * a.nchunk;
    const float Wf = (float)a.W, Hf = (float)a.H;

    for (int item = blockIdx.x * nwaves + wave; item < items; item += gridDim.x * nwaves) {
        const int tile = item / a.nchunk, ch = item - tile * a.nchunk;
        const int r = tile * 16 + ln;
        const bool rok = r < a.M;
        const int rr = rok ? r : a.M - 1;
        const int b = rr / a.Nq, j = rr - b * a.Nq;
        const size_t src = (size_t)b * a.N + (size_t)j * a.ray_step;  // ray j of the launch is rays[b, j * ray_step]
        float x, y;
        // view: the pixel's world point, its keyframe z, prior sample and validity
        float vX[3] = {0.f, 0.f, 0.f}, vz = 0.f, vprior = 0.f;
        bool vdok = false, vvalid = false;
        const float *cam = s_cam + b * kCamFloats;  // (kView / kViewSearch)
        // the view's invK rows (12) and world_T_cam rows (12) of batch b
        const float *vcam = cam + 24;
        int vkey = 255, vslot = 0;  // (keys) the selected key - its position in key_slots - and its slot
        if constexpr (kKeys) vcam = s_cam + (a.nkeys * a.nb + b) * kKeyCamFloats;
        // ---- one point Xc of the view camera's frame: world point, Project3D into the keyframe (project_points_k, verbatim), validity, nearest
        // prior sample; the expressions of include/idh.h.  Every quarter-lane of a ray computes the same values ----
        auto probe = [&](const float (&Xc)[3], const bool dok) {
            const float *T = vcam + 12;
#pragma unroll
            for (int i = 0; i < 3; ++i) vX[i] = fmaf(T[4 * i], Xc[0], fmaf(T[4 * i + 1], Xc[1], fmaf(T[4 * i + 2], Xc[2], T[4 * i + 3])));
            const float X0 = vX[0], X1 = vX[1], X2 = vX[2];
            if constexpr (kKeys) {
                // the projection and the validity rule below, once per key; the first valid key is kept in scalars (u, v, z, key, slot), key 0's z
                // stands in where none is valid.  The prior texel is the selected key's alone
                float bu = 0.f, bv = 0.f, bz = 0.f, z0 = 0.f;
                bool found = false;
                vkey = 255;
                vslot = 0;
#pragma unroll 1
                for (int m = 0; m < a.nkeys; ++m) {
                    const float *P = s_cam + (m * a.nb + b) * kKeyCamFloats;
                    const float cx = fmaf(P[0], X0, fmaf(P[1], X1, fmaf(P[2], X2, P[3])));
                    const float cy = fmaf(P[4], X0, fmaf(P[5], X1, fmaf(P[6], X2, P[7])));
                    const float cz = fmaf(P[8], X0, fmaf(P[9], X1, fmaf(P[10], X2, P[11])));
                    const float z = fmaxf(cz, 1e-5f);
                    const float u = cx / z, v = cy / z;
                    const bool ok = dok && cz > 0.f && u >= 0.f && u < Wf && v >= 0.f && v < Hf;
                    const bool take = ok && !found;
                    const int slot = a.key_slots[m];  // (m is wave-uniform)
                    if (m == 0) z0 = z;
                    bu = take ? u : bu;
                    bv = take ? v : bv;
                    bz = take ? z : bz;
                    vkey = take ? m : vkey;
                    vslot = take ? slot : vslot;
                    found = found || ok;
                }
                vvalid = found;
                vz = found ? bz : z0;
                vprior = a.prior_const;
                if (a.prior) {
                    const float *Q = s_cam + ((found ? vkey : 0) * a.nb + b) * kKeyCamFloats + 12;
                    const float qx = fmaf(Q[0], X0, fmaf(Q[1], X1, fmaf(Q[2], X2, Q[3])));
                    const float qy = fmaf(Q[4], X0, fmaf(Q[5], X1, fmaf(Q[6], X2, Q[7])));
                    const float pz = fmaf(Q[8], X0, fmaf(Q[9], X1, fmaf(Q[10], X2, Q[11])));
                    const float zz = fmaxf(pz, 1e-5f);
                    const float pu = qx / zz, pw = qy / zz;
                    const float gx = (pu / Wf - 0.5f) * 2.f, gy = (pw / Hf - 0.5f) * 2.f;
                    const float sx = ((gx + 1.f) * Wf - 1.f) * 0.5f, sy = ((gy + 1.f) * Hf - 1.f) * 0.5f;
                    const float xr = rintf(sx), yr = rintf(sy);  // round-half-even, as sample_prior_k
                    const bool in = vvalid && pz > 0.f && xr >= 0.f && xr <= Wf - 1.f && yr >= 0.f && yr <= Hf - 1.f;  // no valid key: no texel is read
                    // (texel 0 of the selected key's map - of the first key's where none is valid - exists: no branch)
                    const float texel = a.prior[((size_t)(found ? vslot : a.key_slots[0]) * a.nb + b) * a.H * a.W + (size_t)(in ? (int)yr * a.W + (int)xr : 0)];
                    vprior = in ? texel : -1.f;
                }
                x = bu;
                y = bv;
                return;
            }
            const float *P = cam;
            const float cx = fmaf(P[0], X0, fmaf(P[1], X1, fmaf(P[2], X2, P[3])));
            const float cy = fmaf(P[4], X0, fmaf(P[5], X1, fmaf(P[6], X2, P[7])));
            const float cz = fmaf(P[8], X0, fmaf(P[9], X1, fmaf(P[10], X2, P[11])));
            const float z = fmaxf(cz, 1e-5f);
            const float u = cx / z, v = cy / z;
            vvalid = dok && cz > 0.f && u >= 0.f && u < Wf && v >= 0.f && v < Hf;
            vz = z;
            vprior = a.prior_const;
            if (a.prior) {
                const float *Q = cam + 12;
                const float qx = fmaf(Q[0], X0, fmaf(Q[1], X1, fmaf(Q[2], X2, Q[3])));
                const float qy = fmaf(Q[4], X0, fmaf(Q[5], X1, fmaf(Q[6], X2, Q[7])));
                const float pz = fmaf(Q[8], X0, fmaf(Q[9], X1, fmaf(Q[10], X2, Q[11])));
                const float zz = fmaxf(pz, 1e-5f);
                const float pu = qx / zz, pw = qy / zz;
                const float gx = (pu / Wf - 0.5f) * 2.f, gy = (pw / Hf - 0.5f) * 2.f;
                const float sx = ((gx + 1.f) * Wf - 1.f) * 0.5f, sy = ((gy + 1.f) * Hf - 1.f) * 0.5f;
                const float xr = rintf(sx), yr = rintf(sy);  // round-half-even, as sample_prior_k
                const bool in = vvalid && pz > 0.f && xr >= 0.f && xr <= Wf - 1.f && yr >= 0.f && yr <= Hf - 1.f;  // an invalid pixel reads no texel
                const float texel = a.prior[(size_t)b * a.H * a.W + (size_t)(in ? (int)yr * a.W + (int)xr : 0)];  // texel 0 exists: no branch
                vprior = in ? texel : -1.f;
            }
            x = u;
            y = v;
        };
        float vc[3] = {0.f, 0.f, 0.f};  // kViewSearch / kViewMarch: the ray's direction invK (x, y, 1), once
        if constexpr (kMode == kSamples || kMode == kSearch) {
            x = a.rays[2 * src];
            y = a.rays[2 * src + 1];
        } else if constexpr (kDense) {
            const int pix = j % (a.vh * a.vw), row = pix / a.vw, col = pix - row * a.vw;
            const float dr = a.depth[src];
            vdok = dr > 0.f && dr <= 3.4028234663852886e38f;  // finite and positive (NaN fails both); anything else is asked as d = 0 and stores `fill`
            const float d = vdok ? dr : 0.f;
            const float px = (float)col + 0.5f, py = (float)row + 0.5f;  // BackprojectDepth's pixel centres (geometry_utils.py:39)
            const float *iK = vcam;
            float Xc[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) Xc[i] = d * fmaf(iK[4 * i], px, fmaf(iK[4 * i + 1], py, iK[4 * i + 2]));
            probe(Xc, vdok);
            if (!__any(vvalid)) {  // no valid ray in the tile (wave-uniform): no gather, no MLP
                if (q == 0 && rok) {
                    a.out[src] = a.fill;
                    if (a.flags) a.flags[src] = kKeys ? 255 : 0;
                    if (a.sdepth) a.sdepth[src] = vdok ? vz : 0.f;
                    if (a.points) {
#pragma unroll
                        for (int i = 0; i < 3; ++i) a.points[3 * src + i] = vdok ? vX[i] : 0.f;
                    }
                }
                continue;
            }
        } else {
            float px, py;
            if (a.rays) {
                px = a.rays[2 * src];
                py = a.rays[2 * src + 1];
            } else {
                const int row = j / a.vw, col = j - row * a.vw;
                px = (float)col + 0.5f;
                py = (float)row + 0.5f;
            }
            const float *iK = vcam;
#pragma unroll
            for (int i = 0; i < 3; ++i) vc[i] = fmaf(iK[4 * i], px, fmaf(iK[4 * i + 1], py, iK[4 * i + 2]));
        }
        f32x4 pre1[kNS][1];
        // gather + layer 1 of the row sampled at (x, y); `live` false: no corner is read (an invalid pixel of a view), f = 0
        auto gather = [&](const bool live) {
            // ---- gather: the expression of include/idh.h, one rounding per operation (-ffp-contract=off) ----
            const float gx = (x / a.grid_w - 0.5f) * 2.f, gy = (y / a.grid_h - 0.5f) * 2.f;              // bd_model.py:325-326
            const float ix = ((gx + 1.f) * Wf - 1.f) * 0.5f, iy = ((gy + 1.f) * Hf - 1.f) * 0.5f;        // grid_sample, align_corners=False
            const float x0 = floorf(ix), y0 = floorf(iy);
            const float wx0 = (x0 + 1.f) - ix, wx1 = ix - x0, wy0 = (y0 + 1.f) - iy, wy1 = iy - y0;
            const float wgt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};  // nw, ne, sw, se
            // validity in float first: a far or non-finite coordinate never reaches the integer conversion (NaN fails every comparison)
            const bool vx0 = x0 >= 0.f && x0 <= Wf - 1.f, vx1 = x0 >= -1.f && x0 <= Wf - 2.f;
            const bool vy0 = y0 >= 0.f && y0 <= Hf - 1.f, vy1 = y0 >= -1.f && y0 <= Hf - 2.f;
            const int xi = (vx0 || vx1) ? (int)x0 : 0, yi = (vy0 || vy1) ? (int)y0 : 0;
            const bool cv[4] = {live && vx0 && vy0, live && vx1 && vy0, live && vx0 && vy1, live && vx1 && vy1};
            const int base = b * a.H * a.W;
            const float *feat = a.feat;
            if constexpr (kKeys) feat += (size_t)vslot * a.key_stride;  // the selected key's block; no key selected: nothing is read
            const int crow[4] = {base + yi * a.W + xi, base + yi * a.W + xi + 1, base + (yi + 1) * a.W + xi, base + (yi + 1) * a.W + xi + 1};

            // ---- layer 1, sample-independent part: pre1^T = W1f . feat^T + b1 ----
#pragma unroll
            for (int i = 0; i < kNS; ++i) pre1[i][0] = *reinterpret_cast<const f32x4 *>(s_b1 + 16 * i + 4 * q);
#pragma unroll 1
            for (int c = 0; c < cblocks; ++c) {
                f32x4 Bf = (f32x4){0.f, 0.f, 0.f, 0.f};
                if ((16 * c + 4 * q) < a.Cf) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (cv[k]) {  // a corner outside the map is not read
                            const float *fp = feat + (size_t)crow[k] * a.cs + 16 * c + 4 * q;
                            f32x4 v;
                            if (a.feat_unaligned) v = (f32x4){fp[0], fp[1], fp[2], fp[3]};
                            else v = *reinterpret_cast<const f32x4 *>(fp);
#pragma unroll
                            for (int e = 0; e < 4; ++e) Bf[e] = Bf[e] + v[e] * wgt[k];
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < kNS; ++i) {
                    const f32x4 A = w1_lds ? sW1[(c * kNS + i) * 64 + lane]
                                           : *reinterpret_cast<const f32x4 *>(a.w1f + ((size_t)(c * kNS + i) * 64 + lane) * 4);
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) pre1[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[kk], Bf[kk], pre1[i][0], 0, 0, 0);
                }
            }
        };
        // ---- one evaluation at depth dv, prior pv: exactly the plane body of binary_mlp_k; every lane of a ray returns the same logit ----
        auto eval = [&](const float dv, const float pv) -> float {
            f32x4 h1[kNS][1], acc[kNS][1];
            auto layer1 = [&](auto with_prior) {
#pragma unroll
                for (int i = 0; i < kNS; ++i) {
                    const f32x4 wd = *reinterpret_cast<const f32x4 *>(s_wd + 16 * i + 4 * q);
                    f32x4 wp = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (decltype(with_prior)::value) wp = *reinterpret_cast<const f32x4 *>(s_wp + 16 * i + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v = fmaf(wd[e], dv, pre1[i][0][e]);
                        if (decltype(with_prior)::value) v = fmaf(wp[e], pv, v);
                        h1[i][0][e] = elu1(v);
                    }
                    acc[i][0] = *reinterpret_cast<const f32x4 *>(s_b2 + 16 * i + 4 * q);
                }
            };
            if (a.has_prior) layer1(std::true_type{});
            else layer1(std::false_type{});
            __builtin_amdgcn_s_setprio(0);
            dense128<1>(h1, sW2, lane, acc);
            __builtin_amdgcn_s_setprio(2);
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < kNS; ++i) {
                const f32x4 w3 = *reinterpret_cast<const f32x4 *>(s_w3 + 16 * i + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) t = fmaf(w3[e], elu1(acc[i][0][e]), t);
            }
            t += __shfl_xor(t, 16, 64);
            t += __shfl_xor(t, 32, 64);
            return t + b3;
        };
        if constexpr (kMode != kViewSearch && kMode != kViewKeysSearch && !kMarch) gather(!kDense || vvalid);  // an invalid pixel of a view reads no corner
        if constexpr (kDense) {
            const float logit = eval(vz, vprior);
            if (q == 0 && rok) {
                a.out[src] = vvalid ? logit : a.fill;
                if (a.flags) a.flags[src] = kKeys ? (unsigned char)vkey : (vvalid ? 1 : 0);
                if (a.sdepth) a.sdepth[src] = vdok ? vz : 0.f;
                if (a.points) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) a.points[3 * src + i] = vdok ? vX[i] : 0.f;
                }
            }
        } else if constexpr (kMode == kSamples) {
            const size_t doff = src * a.S, ooff = (size_t)rr * a.S;
            const int s_begin = ch * a.s_chunk, s_end = min(a.S, s_begin + a.s_chunk);
#pragma unroll 1
            for (int s = s_begin; s < s_end; ++s) {
                const float dv = a.depth[doff + s];
                const float pv = a.has_prior ? (a.prior ? a.prior[doff + s] : a.prior_const) : 0.f;
                const float logit = eval(dv, pv);
                if (q == 0 && rok) a.out[ooff + s] = logit;
            }
        } else if constexpr (kMode == kSearch) {
            // ---- the search rule of binary_mlp_k: first query (hi - lo) / 2 (the reference's, not the midpoint), "visible" = logit < thr moves hi ----
            const float pv = a.has_prior ? (a.prior ? a.prior[src] : a.prior_const) : 0.f;  // one value per ray, as plane 0 of the dense search's prior
            float lo = a.lo, hi = a.hi, sd = (a.hi - a.lo) * 0.5f, logit = 0.f;
            unsigned moved = 0;
#pragma unroll 1
            for (int p = 0; p < a.iters; ++p) {
                logit = eval(sd, pv);
                float thr = a.thr_logit;
                if (a.n_bins > 0) {  // torch.bucketize(depth, bins): number of edges strictly below the query depth
                    int idx = 0;
                    for (int e = 0; e < a.n_bins; ++e) idx += a.bins[e] < sd ? 1 : 0;
                    thr = a.thr_logits[idx < a.n_bins ? idx : a.n_bins - 1];
                }
                if (logit < thr) { hi = sd; moved |= 1u; }
                else { lo = sd; moved |= 2u; }
                sd = (hi + lo) * 0.5f;
            }
            if (q == 0 && rok) {  // ray rr = (b, j) with ray_step = 1: src == rr
                a.sdepth[src] = sd;
                a.out[src] = logit;
                if (a.flags) a.flags[src] = (unsigned char)moved;
                if (a.points) {  // the expression of include/idh.h: BackprojectDepth on the ray's own (x, y), then world_T_cam
                    const float *iK = a.invK + (size_t)b * 16;
                    float X[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) X[i] = sd * fmaf(iK[4 * i], x, fmaf(iK[4 * i + 1], y, iK[4 * i + 2]));
                    if (a.wTc) {
                        const float *T = a.wTc + (size_t)b * 16;
#pragma unroll
                        for (int i = 0; i < 3; ++i)
                            a.points[3 * src + i] = fmaf(T[4 * i], X[0], fmaf(T[4 * i + 1], X[1], fmaf(T[4 * i + 2], X[2], T[4 * i + 3])));
                    } else {
#pragma unroll
                        for (int i = 0; i < 3; ++i) a.points[3 * src + i] = X[i];
                    }
                }
            }
        } else if constexpr (kMarch) {
            // ---- first hit along a ray of the view (include/idh.h): the samples march_depths[s] in turn until the first probe that is behind
            // (logit < thr), then `refine` steps of the rule below inside [previous sample, that sample].  st: -1 marching, n > 0 refining with n steps
            // left, 0 done.  A marching ray's sample index is the loop counter, so the sample is one scalar load per step; while marching "in front
            // moves lo, behind moves hi" leaves exactly the bracket the refinement starts from.  A ray that is done rides along as an invalid probe:
            // it reads nothing and its state is frozen ----
            float lo = 0.f, hi = 0.f, sd = 0.f, logit = 0.f;
            unsigned moved = 0;
            int st = -1, hit = 255, lkey = 255;
            const int steps = a.n_march + a.refine;
            float Xc[3];
#pragma unroll 1
            for (int it = 0; it < steps; ++it) {
                const bool active = st != 0;
                if (!__any(active)) break;  // every ray of the tile is done (wave-uniform)
                const float qm = a.march_depths[it < a.n_march ? it : a.n_march - 1];  // (it is wave-uniform)
                sd = st < 0 ? qm : sd;
#pragma unroll
                for (int i = 0; i < 3; ++i) Xc[i] = sd * vc[i];
                probe(Xc, active);
                float l = a.fill;
                if (kViewSearchSkip ? __any(vvalid) : true) {  // no active ray of the tile has a valid probe at this step: no gather, no MLP (wave-uniform)
                    gather(vvalid);
                    const float e = eval(vz, vprior);
                    l = vvalid ? e : a.fill;
                }
                float thr = a.thr_logit;
                if (a.n_bins > 0) {
                    int idx = 0;
                    for (int e = 0; e < a.n_bins; ++e) idx += a.bins[e] < vz ? 1 : 0;
                    thr = a.thr_logits[idx < a.n_bins ? idx : a.n_bins - 1];
                }
                const bool behind = l < thr, marching = st < 0;
                // the state after this step, formed for every lane and taken by the active ones
                const float nhi = behind ? sd : hi, nlo = behind ? lo : sd;
                const bool bracket = marching && behind && it > 0;  // s* > 0: refine inside [march_depths[s* - 1], march_depths[s*]]
                const int nst = marching ? (behind ? (it > 0 ? a.refine : 0) : (it == a.n_march - 1 ? 0 : -1)) : st - 1;
                const float nsd = (bracket || !marching) ? (nhi + nlo) * 0.5f : sd;  // s* = 0 and "none" keep the sample itself
                if (active) {
                    logit = l;
                    moved |= (behind ? 1u : 2u) | (vvalid ? 0u : 4u);
                    hit = (marching && behind) ? it : hit;
                    hi = nhi;
                    lo = nlo;
                    sd = nsd;
                    st = nst;
                    if constexpr (kKeys) lkey = vkey;
                }
            }
            if (q == 0 && rok) {
                a.sdepth[src] = sd;
                a.out[src] = logit;
                if (a.flags) a.flags[src] = (unsigned char)moved;
                if (a.hit_step) a.hit_step[src] = (unsigned char)hit;
                if constexpr (kKeys) {
                    if (a.keyout) a.keyout[src] = (unsigned char)lkey;  // of the last evaluated probe
                }
                if (a.points) {  // the world point of the final depth, by the expressions of the probes
                    const float *T = vcam + 12;
#pragma unroll
                    for (int i = 0; i < 3; ++i) Xc[i] = sd * vc[i];
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        a.points[3 * src + i] = fmaf(T[4 * i], Xc[0], fmaf(T[4 * i + 1], Xc[1], fmaf(T[4 * i + 2], Xc[2], T[4 * i + 3])));
                }
            }
        } else {
            // ---- the same rule along a ray of the view: every step is a view_mlp_k pixel at rendered = sd; thr is keyed by the probe's keyframe z ----
            float lo = a.lo, hi = a.hi, sd = (a.hi - a.lo) * 0.5f, logit = 0.f;
            unsigned moved = 0;
            float Xc[3];
#pragma unroll 1
            for (int p = 0; p < a.iters; ++p) {
#pragma unroll
                for (int i = 0; i < 3; ++i) Xc[i] = sd * vc[i];
                probe(Xc, true);
                logit = a.fill;
                if (kViewSearchSkip ? __any(vvalid) : true) {  // a tile without a valid probe at this step: no gather, no MLP (wave-uniform); `fill` either way
                    gather(vvalid);
                    const float l = eval(vz, vprior);
                    logit = vvalid ? l : a.fill;
                }
                float thr = a.thr_logit;
                if (a.n_bins > 0) {
                    int idx = 0;
                    for (int e = 0; e < a.n_bins; ++e) idx += a.bins[e] < vz ? 1 : 0;
                    thr = a.thr_logits[idx < a.n_bins ? idx : a.n_bins - 1];
                }
                if (logit < thr) { hi = sd; moved |= 1u; }
                else { lo = sd; moved |= 2u; }
                if (!vvalid) moved |= 4u;
                sd = (hi + lo) * 0.5f;
            }
            if (q == 0 && rok) {
                a.sdepth[src] = sd;
                a.out[src] = logit;
                if (a.flags) a.flags[src] = (unsigned char)moved;
                if constexpr (kKeys) {
                    if (a.keyout) a.keyout[src] = (unsigned char)vkey;  // of the last step
                }
                if (a.points) {  // the world point of the final query, by the expressions of the probes
                    const float *T = vcam + 12;
#pragma unroll
                    for (int i = 0; i < 3; ++i) Xc[i] = sd * vc[i];
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        a.points[3 * src + i] = fmaf(T[4 * i], Xc[0], fmaf(T[4 * i + 1], Xc[1], fmaf(T[4 * i + 2], Xc[2], T[4 * i + 3])));
                }
            }
        }
    }
}

__global__ __launch_bounds__(kRayMaxThreads) void ray_mlp_k(const RayArgs a) { ray_body<kSamples>(a); }
__global__ __launch_bounds__(kRayMaxThreads) void ray_search_k(const RayArgs a) { ray_body<kSearch>(a); }
__global__ __launch_bounds__(kRayMaxThreads) void view_mlp_k(const RayArgs a) { ray_body<kView>(a); }
__global__ __launch_bounds__(kRayMaxThreads) void view_search_k(const RayArgs a) { ray_body<kViewSearch>(a); }
__global__ __launch_bounds__(kRayMaxThreads) void view_keys_k(const KeysArgs a) { ray_body<kViewKeys>(a); }
__global__ __launch_bounds__(kRayMaxThreads) void view_keys_search_k(const KeysArgs a) { ray_body<kViewKeysSearch>(a); }
__global__ __launch_bounds__(kRayMaxThreads) void view_march_k(const MarchArgs a) { ray_body<kViewMarch>(a); }
__global__ __launch_bounds__(kRayMaxThreads) void view_keys_march_k(const KeysMarchArgs a) { ray_body<kViewKeysMarch>(a); }

// ---- world points -> rays of the current view (+ the nearest sample of a prior prediction) ----
// Project3D (reference utils/geometry_utils.py:77-89): P = K cam_T_world, c = P[:3] X, depth = max(c_z, 1e-5), (u, v) = c_xy / depth.
// With a prior: the point goes through the prior camera's P' the same way and BDModel.sample_prior's nearest sample
// (bd_model.py:405-409) is taken at (u', v'), with sample_prior_k's rounding; -1 where the prior camera's z <= 0 or the texel is outside.
__global__ __launch_bounds__(256) void project_points_k(const float *__restrict__ pts, const float *__restrict__ cam_T_world,
                                                        const float *__restrict__ Kmat, int N, int H, int W, float *__restrict__ rays,
                                                        float *__restrict__ depth, unsigned char *__restrict__ valid,
                                                        const float *__restrict__ prior_pred, const float *__restrict__ prior_cam_T_world,
                                                        const float *__restrict__ prior_K, float *__restrict__ prior_out) {
    __shared__ float sP[2][12];
    const int b = blockIdx.y;
    if (threadIdx.x < 2 && (threadIdx.x == 0 || prior_pred)) {
        const float *Kb = (threadIdx.x ? prior_K : Kmat) + (size_t)b * 16, *T = (threadIdx.x ? prior_cam_T_world : cam_T_world) + (size_t)b * 16;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) {
                float s = 0.f;
                for (int m = 0; m < 4; ++m) s = fmaf(Kb[i * 4 + m], T[m * 4 + j], s);
                sP[threadIdx.x][i * 4 + j] = s;
            }
    }
    __syncthreads();
    const float Wf = (float)W, Hf = (float)H;
    for (int n = blockIdx.x * 256 + threadIdx.x; n < N; n += gridDim.x * 256) {
        const size_t o = (size_t)b * N + n;
        const float X0 = pts[3 * o], X1 = pts[3 * o + 1], X2 = pts[3 * o + 2];
        const float *P = sP[0];
        const float cx = fmaf(P[0], X0, fmaf(P[1], X1, fmaf(P[2], X2, P[3])));
        const float cy = fmaf(P[4], X0, fmaf(P[5], X1, fmaf(P[6], X2, P[7])));
        const float cz = fmaf(P[8], X0, fmaf(P[9], X1, fmaf(P[10], X2, P[11])));
        const float z = fmaxf(cz, 1e-5f);
        const float u = cx / z, v = cy / z;
        rays[2 * o] = u;
        rays[2 * o + 1] = v;
        depth[o] = z;
        valid[o] = (cz > 0.f && u >= 0.f && u < Wf && v >= 0.f && v < Hf) ? 1 : 0;
        if (prior_pred) {
            const float *Q = sP[1];
            const float px = fmaf(Q[0], X0, fmaf(Q[1], X1, fmaf(Q[2], X2, Q[3])));
            const float py = fmaf(Q[4], X0, fmaf(Q[5], X1, fmaf(Q[6], X2, Q[7])));
            const float pz = fmaf(Q[8], X0, fmaf(Q[9], X1, fmaf(Q[10], X2, Q[11])));
            const float zz = fmaxf(pz, 1e-5f);
            const float pu = px / zz, pw = py / zz;
            const float gx = (pu / Wf - 0.5f) * 2.f, gy = (pw / Hf - 0.5f) * 2.f;
            const float sx = ((gx + 1.f) * Wf - 1.f) * 0.5f, sy = ((gy + 1.f) * Hf - 1.f) * 0.5f;
            const float xr = rintf(sx), yr = rintf(sy);  // round-half-even, as sample_prior_k
            float val = -1.f;
            if (pz > 0.f && xr >= 0.f && xr <= Wf - 1.f && yr >= 0.f && yr <= Hf - 1.f)
                val = prior_pred[(size_t)b * H * W + (size_t)((int)yr * W + (int)xr)];
            prior_out[o] = val;
        }
    }
}

}  // namespace

// ---- host side ----
// An entry point is the rules that apply to it, in the order that decides which code wins - argument errors (IDH_EINVAL), the empty call
// (IDH_OK), missing and misaligned pointers (IDH_EINVAL), sizes (IDH_EUNSUPPORTED) -, then its argument block, value-initialised and filled by
// name, then ray_mlp_launch<mode>.  A rule is one helper for every entry point that has it; what one has on its own stands in its body.
constexpr bool mode_view(int m) { return m >= kView; }  // the rays come from another camera: cameras in LDS, grid = (W, H)
constexpr bool mode_keys(int m) { return m == kViewKeys || m == kViewKeysSearch || m == kViewKeysMarch; }  // (kKeys of ray_body)

// The kernels, in the order of the modes' enum; the argument struct of a mode is what its kernel takes
constexpr auto kRayKernels = std::make_tuple(ray_mlp_k, ray_search_k, view_mlp_k, view_search_k, view_keys_k, view_keys_search_k, view_march_k, view_keys_march_k);
static_assert(std::tuple_size<decltype(kRayKernels)>::value == kRayModes, "one kernel per mode");

// Work partition of one launch (also what tests/ray_query_ref.py restates for its persistent-loop case): an item is 16 rays x one run of
// samples.  While the ray tiles alone do not give every SIMD of the device (256 CUs x 4) a wave, the S samples of a tile are cut into runs
// of at least kMinChunk (a run repeats the gather and the W1f product: 128 - 512 MFMAs against 256 per sample), so N = 4096 rays x 64
// samples run on 1024 waves instead of 256.  Every mode but kSamples has S = 1 and so one item per tile: its evaluations are dependent,
// there is nothing to split.  The kernel and the cameras' share of LDS follow from the mode: B x 48 floats for one key, (M + 1) B x 24 for M.
template <int kMode, class Args>
static int ray_mlp_launch(Args a, void *stream) {
    constexpr int kSimds = 256 * 4, kMinChunk = 8;
    const long long tiles = ((long long)a.M + 15) / 16;
    int nchunk = 1;
    if (tiles < kSimds) {
        nchunk = (int)((kSimds + tiles - 1) / tiles);
        const int most = (a.S + kMinChunk - 1) / kMinChunk;
        if (nchunk > most) nchunk = most;
    }
    a.s_chunk = (a.S + nchunk - 1) / nchunk;
    a.nchunk = (a.S + a.s_chunk - 1) / a.s_chunk;
    const long long items = tiles * a.nchunk;
    // 4-wave workgroups, as many as there are items, while that leaves at most one workgroup per CU; beyond that the persistent 12-wave
    // form of binary_mlp_k (3 waves per SIMD share one copy of the weights)
    const int waves = items <= 256 * 4 ? 4 : kRayMaxThreads / 64;
    long long grid = (items + waves - 1) / waves;
    if (grid > 256) grid = 256;
    const int cblocks = (a.Cf + 15) >> 4;
    size_t lds = ((size_t)kNS * kNS * 64 + (cblocks <= kW1LdsMaxBlocks ? (size_t)cblocks * kNS * 64 : 0)) * sizeof(f32x4) + 6 * kHidden * sizeof(float);
    if constexpr (mode_keys(kMode)) lds += (size_t)(a.nkeys + 1) * a.nb * kKeyCamFloats * sizeof(float);
    else if constexpr (mode_view(kMode)) lds += (size_t)a.nb * kCamFloats * sizeof(float);
    constexpr void (*kernel)(const Args) = std::get<kMode>(kRayKernels);  // (RayArgs, KeysArgs, MarchArgs or KeysMarchArgs: no other compiles)
    static IdhDeviceOnce attr_set;
    if (attr_set.first()) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return IDH_ELAUNCH;
        attr_set.mark();
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(waves * 64), lds, idh_stream(stream), a);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

// ---- the rules ----
using Ptrs = std::initializer_list<const void *>;
static bool any_null(Ptrs ps) { return std::any_of(ps.begin(), ps.end(), [](const void *p) { return !p; }); }
static bool any_misaligned(Ptrs ps) { return std::any_of(ps.begin(), ps.end(), [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }); }
// the feature map and its shapes
static bool feat_bad(int B, int H, int W, int Cf, int feat_cs) { return B < 0 || H <= 0 || W <= 0 || Cf <= 0 || (Cf & 3) || feat_cs < Cf; }
// the constant threshold (n_bins = 0) or the tables of the per-depth Thresholder
static bool threshold_bad(float threshold, const float *bins, const float *thr_logits, int n_bins) {
    return n_bins < 0 || (n_bins == 0 ? !(threshold > 0.f) || !(threshold < 1.f) : !bins || !thr_logits);
}
// the bracket of a search in another camera: finite, 0 < lo < hi (NaN fails every comparison); idh_binary_mlp_rays_search_fwd asks hi > lo alone
static bool bracket_bad(float lo, float hi) { return !(lo > 0.f) || !(hi > lo) || !(lo <= FLT_MAX) || !(hi <= FLT_MAX); }
// the cameras of a view entry point (rings of them, with several keys); a prior map comes with its cameras and a prior-enabled network
struct ViewCams { const float *invK, *wTc, *key_cTw, *key_K, *prior_cTw, *prior_K; };
static bool prior_map_bad(const float *prior, int has_prior, const ViewCams &c) { return prior && (!has_prior || !c.prior_cTw || !c.prior_K); }
// the pointers every view entry point requires, and those it wants 4-byte aligned; `req` (required) and `opt` are the entry point's own
static bool view_ptrs_bad(const float *feat, const ViewCams &c, const float *prior, const float *w1f, const float *w2, const float *vecs, Ptrs req, Ptrs opt) {
    return any_null({feat, c.invK, c.wTc, c.key_cTw, c.key_K, w1f, w2, vecs}) || any_null(req) ||
           any_misaligned({feat, c.invK, c.wTc, c.key_cTw, c.key_K, prior, c.prior_cTw, c.prior_K}) || any_misaligned(req) || any_misaligned(opt);
}
// where the rays of a view come from: `rays` (B,N,2), or null - the pixel centres of its h x w grid; the dense modes have vP x vh x vw pixels
struct RaySource { long long Nq; int vP, vh, vw; bool bad, empty; };
static RaySource ray_source(const float *rays, int N, int h, int w) {
    if (rays) return {N, 1, 1, N, N < 0, N == 0};
    return {(long long)h * w, 1, h, w, h < 0 || w < 0, h == 0 || w == 0};
}
// rays (a tile rounds their number up to 16) and texels are indexed with ints (Nq first: B * Nq stays inside 64 bits; it can be large only
// with a grid, the dense modes bound P * h before they form it); the cameras of every batch element of a view sit in LDS
template <int kMode>
static int size_limits(int B, long long Nq, int H, int W) {
    if (Nq >= (1ll << 31) || (long long)B * Nq >= (1ll << 31) - 16 || (long long)B * H * W >= (1ll << 31)) return IDH_EUNSUPPORTED;
    return mode_view(kMode) && B > kViewMaxBatch ? IDH_EUNSUPPORTED : IDH_OK;
}
// the multi-key entry points, between the pointers and the sizes: the order of the keys and the ring's geometry.  IDH_OK: k's own fields are filled in
static int keys_args(KeysArgs &k, long long key_stride, int n_slots, const int *key_slots, int M, int B, int H, int W, int feat_cs) {
    if (!key_slots || M <= 0 || n_slots <= 0 || key_stride < 0) return IDH_EINVAL;
    if (M > kMaxKeys) return IDH_EUNSUPPORTED;
    for (int m = 0; m < M; ++m) {
        if (key_slots[m] < 0 || key_slots[m] >= n_slots) return IDH_EINVAL;
        for (int o = 0; o < m; ++o)
            if (key_slots[o] == key_slots[m]) return IDH_EINVAL;
    }
    if (n_slots > 1 && key_stride < (long long)B * H * W * feat_cs) return IDH_EINVAL;
    if ((long long)M * B > kViewMaxBatch || (long long)n_slots * B * H * W >= (1ll << 31)) return IDH_EUNSUPPORTED;
    k.key_stride = key_stride, k.nkeys = M;
    std::copy(key_slots, key_slots + M, k.key_slots);
    return IDH_OK;
}
// the march entry points, among their argument errors
static int march_args_ok(const float *march_depths, int n_march, int refine) {
    if (n_march <= 0 || n_march > 255 || refine < 0 || !march_depths || (reinterpret_cast<uintptr_t>(march_depths) & 3)) return IDH_EINVAL;
    return refine > (1 << 30) ? IDH_EUNSUPPORTED : IDH_OK;  // (n_march + refine stays an int)
}

// ---- the argument block: `Args a{}` leaves every field zero or null, these name what the modes share ----
// every mode: the feature map (rows of a ring's slots lie key_stride apart), the prior, the weights, and one sample per ray in one item
template <class Args>
static void set_common(Args &a, const float *feat, int feat_cs, int Cf, int H, int W, const float *prior, int has_prior, float prior_const,
                       const float *w1f, const float *w2, const float *vecs) {
    a.feat = feat, a.cs = feat_cs, a.Cf = Cf, a.H = H, a.W = W;
    a.prior = prior, a.has_prior = has_prior, a.prior_const = prior_const;
    a.w1f = w1f, a.w2 = w2, a.vecs = vecs;
    a.S = a.ray_step = a.nchunk = a.s_chunk = 1;
    long long key_stride = 0;
    if constexpr (std::is_base_of<KeysArgs, Args>::value) key_stride = a.key_stride;
    a.feat_unaligned = ((feat_cs & 3) || (key_stride & 3) || (reinterpret_cast<uintptr_t>(feat) & 15)) ? 1 : 0;
}
// the B x Nq rays of the launch, of N per batch element, in pixel-centre units of a grid_w x grid_h grid
static void set_rays(RayArgs &a, const float *rays, int B, long long Nq, int N, int grid_w, int grid_h) {
    a.rays = rays, a.M = (int)((long long)B * Nq), a.Nq = (int)Nq, a.N = N;
    a.grid_w = (float)grid_w, a.grid_h = (float)grid_h;
}
// the view modes (after set_common): rays from `src` on the keyframe's own grid, and the cameras
static void set_view(RayArgs &a, const float *rays, int B, const RaySource &src, const ViewCams &c, float fill) {
    set_rays(a, rays, B, src.Nq, (int)src.Nq, a.W, a.H);
    a.invK = c.invK, a.wTc = c.wTc, a.key_cTw = c.key_cTw, a.key_K = c.key_K, a.prior_cTw = c.prior_cTw, a.prior_K = c.prior_K;
    a.nb = B, a.vP = src.vP, a.vh = src.vh, a.vw = src.vw, a.fill = fill;
}
static void set_threshold(RayArgs &a, float threshold, const float *bins, const float *thr_logits, int n_bins) {
    a.thr_logit = n_bins == 0 ? logf(threshold / (1.f - threshold)) : 0.f;
    a.bins = bins, a.thr_logits = thr_logits, a.n_bins = n_bins;
}
// `out`: the logits; what the other three hold depends on the mode (RayArgs)
static void set_outputs(RayArgs &a, float *out, float *sdepth, unsigned char *flags, float *points) {
    a.out = out, a.sdepth = sdepth, a.flags = flags, a.points = points;
}

extern "C" int idh_binary_mlp_rays_fwd(const float *feat_nhwc, int feat_cs, int Cf, int B, int H, int W, const float *rays_bn2,
                                       const float *depth_bns, const float *prior_bns, int has_prior, float prior_const, int N, int S,
                                       int ray_step, int grid_w, int grid_h, const float *w1f_packed, const float *w2_packed,
                                       const float *vecs6x128, float *out_bqs, void *stream) {
    if (feat_bad(B, H, W, Cf, feat_cs) || N < 0 || S <= 0 || ray_step < 1 || grid_w <= 0 || grid_h <= 0) return IDH_EINVAL;
    if (B == 0 || N == 0) return IDH_OK;
    if (any_null({feat_nhwc, rays_bn2, depth_bns, w1f_packed, w2_packed, vecs6x128, out_bqs}) ||
        any_misaligned({feat_nhwc, rays_bn2, depth_bns, prior_bns, out_bqs}))  // (its data pointers alone)
        return IDH_EINVAL;
    const int Nq = (int)(((long long)N + ray_step - 1) / ray_step);
    if (const int rc = size_limits<kSamples>(B, Nq, H, W)) return rc;
    if (((long long)B * Nq + 15) / 16 * ((S + 7) / 8) >= (1ll << 30)) return IDH_EUNSUPPORTED;  // the items of the launch
    RayArgs a{};
    set_common(a, feat_nhwc, feat_cs, Cf, H, W, prior_bns, has_prior, prior_const, w1f_packed, w2_packed, vecs6x128);
    set_rays(a, rays_bn2, B, Nq, N, grid_w, grid_h);
    a.depth = depth_bns, a.S = S, a.ray_step = ray_step, a.out = out_bqs;
    return ray_mlp_launch<kSamples>(a, stream);
}

// Depth and hit point per ray by binary search (reference BDModel.forward(infer_depth=True), bd_model.py:273-292, at the rays of
// run_mlp_train): the gather of idh_binary_mlp_rays_fwd once, then `iters` dependent evaluations in one launch.  include/idh.h states the rule.
extern "C" int idh_binary_mlp_rays_search_fwd(const float *feat_nhwc, int feat_cs, int Cf, int B, int H, int W, const float *rays_bn2,
                                              const float *prior_bn, int has_prior, float prior_const, int N, int grid_w, int grid_h,
                                              const float *w1f_packed, const float *w2_packed, const float *vecs6x128, int iters, float lo, float hi,
                                              float threshold, const float *bins, const float *thr_logits, int n_bins, const float *invK_44,
                                              const float *world_T_cam_44, float *depth_bn, float *last_logits_bn, unsigned char *flags_bn,
                                              float *points_bn3, void *stream) {
    if (feat_bad(B, H, W, Cf, feat_cs) || N < 0 || grid_w <= 0 || grid_h <= 0 || iters <= 0 || !(hi > lo) ||
        threshold_bad(threshold, bins, thr_logits, n_bins) || (points_bn3 && !invK_44))
        return IDH_EINVAL;
    if (B == 0 || N == 0) return IDH_OK;
    if (any_null({feat_nhwc, rays_bn2, w1f_packed, w2_packed, vecs6x128, depth_bn, last_logits_bn}) ||
        any_misaligned({feat_nhwc, rays_bn2, prior_bn, bins, thr_logits, invK_44, world_T_cam_44, depth_bn, last_logits_bn, points_bn3}))
        return IDH_EINVAL;
    if (const int rc = size_limits<kSearch>(B, N, H, W)) return rc;
    RayArgs a{};
    set_common(a, feat_nhwc, feat_cs, Cf, H, W, prior_bn, has_prior, prior_const, w1f_packed, w2_packed, vecs6x128);
    set_rays(a, rays_bn2, B, N, N, grid_w, grid_h);
    a.iters = iters, a.lo = lo, a.hi = hi;
    set_threshold(a, threshold, bins, thr_logits, n_bins);
    a.invK = invK_44, a.wTc = world_T_cam_44;
    set_outputs(a, last_logits_bn, depth_bn, flags_bn, points_bn3);
    return ray_mlp_launch<kSearch>(a, stream);
}

// Dense occlusion in another camera: every pixel of rendered (B,P,h,w) is back-projected in its own view, projected into the keyframe's
// scale-0 map and asked there, in one launch (view_mlp_k).  include/idh.h states the expression and the validity rule.
extern "C" int idh_binary_mlp_view_fwd(const float *feat_nhwc, int feat_cs, int Cf, int B, int H, int W, const float *rendered_bphw, int P, int h,
                                       int w, const float *invK_44, const float *world_T_cam_44, const float *key_cam_T_world_44,
                                       const float *key_K_44, const float *prior_pred_b1hw, const float *prior_cam_T_world_44,
                                       const float *prior_K_44, int has_prior, float prior_const, const float *w1f_packed, const float *w2_packed,
                                       const float *vecs6x128, float fill, float *logits_bphw, unsigned char *valid_bphw, float *view_depth_bphw,
                                       float *view_points_bphw3, void *stream) {
    const ViewCams cams{invK_44, world_T_cam_44, key_cam_T_world_44, key_K_44, prior_cam_T_world_44, prior_K_44};
    if (feat_bad(B, H, W, Cf, feat_cs) || P < 0 || h < 0 || w < 0 || prior_map_bad(prior_pred_b1hw, has_prior, cams)) return IDH_EINVAL;
    if (B == 0 || P == 0 || h == 0 || w == 0) return IDH_OK;
    if (view_ptrs_bad(feat_nhwc, cams, prior_pred_b1hw, w1f_packed, w2_packed, vecs6x128, {rendered_bphw, logits_bphw},
                      {view_depth_bphw, view_points_bphw3}))
        return IDH_EINVAL;
    if ((long long)P * h >= (1ll << 31)) return IDH_EUNSUPPORTED;  // (the product below stays inside 64 bits)
    const RaySource src{(long long)P * h * w, P, h, w};
    if (const int rc = size_limits<kView>(B, src.Nq, H, W)) return rc;
    RayArgs a{};
    set_common(a, feat_nhwc, feat_cs, Cf, H, W, prior_pred_b1hw, has_prior, prior_const, w1f_packed, w2_packed, vecs6x128);
    set_view(a, nullptr, B, src, cams, fill);
    a.depth = rendered_bphw;
    set_outputs(a, logits_bphw, view_depth_bphw, valid_bphw, view_points_bphw3);
    return ray_mlp_launch<kView>(a, stream);
}

// Depth along the rays of another camera: the search of idh_binary_mlp_rays_search_fwd with every step one pixel of idh_binary_mlp_view_fwd at
// rendered = q_n, in one launch (view_search_k).  include/idh.h states the expressions and the invalid-probe rule.
extern "C" int idh_binary_mlp_view_search_fwd(const float *feat_nhwc, int feat_cs, int Cf, int B, int H, int W, int h, int w, const float *rays_bn2,
                                              int N, const float *invK_44, const float *world_T_cam_44, const float *key_cam_T_world_44,
                                              const float *key_K_44, const float *prior_pred_b1hw, const float *prior_cam_T_world_44,
                                              const float *prior_K_44, int has_prior, float prior_const, const float *w1f_packed,
                                              const float *w2_packed, const float *vecs6x128, int iters, float lo, float hi, float threshold,
                                              const float *bins, const float *thr_logits, int n_bins, float fill, float *depth, float *last_logits,
                                              unsigned char *flags, float *points, void *stream) {
    const ViewCams cams{invK_44, world_T_cam_44, key_cam_T_world_44, key_K_44, prior_cam_T_world_44, prior_K_44};
    const RaySource src = ray_source(rays_bn2, N, h, w);
    if (feat_bad(B, H, W, Cf, feat_cs) || src.bad || iters <= 0 || bracket_bad(lo, hi) || threshold_bad(threshold, bins, thr_logits, n_bins) ||
        prior_map_bad(prior_pred_b1hw, has_prior, cams))
        return IDH_EINVAL;
    if (B == 0 || src.empty) return IDH_OK;
    if (view_ptrs_bad(feat_nhwc, cams, prior_pred_b1hw, w1f_packed, w2_packed, vecs6x128, {depth, last_logits}, {rays_bn2, bins, thr_logits, points}))
        return IDH_EINVAL;
    if (const int rc = size_limits<kViewSearch>(B, src.Nq, H, W)) return rc;
    RayArgs a{};
    set_common(a, feat_nhwc, feat_cs, Cf, H, W, prior_pred_b1hw, has_prior, prior_const, w1f_packed, w2_packed, vecs6x128);
    set_view(a, rays_bn2, B, src, cams, fill);
    a.iters = iters, a.lo = lo, a.hi = hi;
    set_threshold(a, threshold, bins, thr_logits, n_bins);
    set_outputs(a, last_logits, depth, flags, points);
    return ray_mlp_launch<kViewSearch>(a, stream);
}

// Dense occlusion in another camera against M remembered keyframes: idh_binary_mlp_view_fwd with the projection looped over the keys and the
// first valid key selected per pixel, in one launch (view_keys_k).  include/idh.h states the expression.
extern "C" int idh_binary_mlp_view_keys_fwd(const float *feat_ring, int feat_cs, int Cf, int B, int H, int W, long long key_stride, int n_slots,
                                            const int *key_slots, int M, const float *rendered_bphw, int P, int h, int w, const float *invK_44,
                                            const float *world_T_cam_44, const float *key_cam_T_world_s44, const float *key_K_s44,
                                            const float *prior_pred_sb1hw, const float *prior_cam_T_world_s44, const float *prior_K_s44,
                                            int has_prior, float prior_const, const float *w1f_packed, const float *w2_packed,
                                            const float *vecs6x128, float fill, float *logits_bphw, unsigned char *key_bphw,
                                            float *view_depth_bphw, float *view_points_bphw3, void *stream) {
    const ViewCams cams{invK_44, world_T_cam_44, key_cam_T_world_s44, key_K_s44, prior_cam_T_world_s44, prior_K_s44};
    if (feat_bad(B, H, W, Cf, feat_cs) || P < 0 || h < 0 || w < 0 || prior_map_bad(prior_pred_sb1hw, has_prior, cams)) return IDH_EINVAL;
    if (B == 0 || P == 0 || h == 0 || w == 0) return IDH_OK;
    if (view_ptrs_bad(feat_ring, cams, prior_pred_sb1hw, w1f_packed, w2_packed, vecs6x128, {rendered_bphw, logits_bphw},
                      {view_depth_bphw, view_points_bphw3}))
        return IDH_EINVAL;
    KeysArgs a{};
    if (const int rc = keys_args(a, key_stride, n_slots, key_slots, M, B, H, W, feat_cs)) return rc;
    if ((long long)P * h >= (1ll << 31)) return IDH_EUNSUPPORTED;  // (the product below stays inside 64 bits)
    const RaySource src{(long long)P * h * w, P, h, w};
    if (const int rc = size_limits<kViewKeys>(B, src.Nq, H, W)) return rc;
    set_common(a, feat_ring, feat_cs, Cf, H, W, prior_pred_sb1hw, has_prior, prior_const, w1f_packed, w2_packed, vecs6x128);
    set_view(a, nullptr, B, src, cams, fill);
    a.depth = rendered_bphw;
    set_outputs(a, logits_bphw, view_depth_bphw, key_bphw, view_points_bphw3);  // (view_keys_k writes the key to `flags`)
    return ray_mlp_launch<kViewKeys>(a, stream);
}

// Depth along the rays of another camera against M remembered keyframes: idh_binary_mlp_view_search_fwd with every step one pixel of
// idh_binary_mlp_view_keys_fwd at rendered = q_n - every step selects its own key - in one launch (view_keys_search_k).
extern "C" int idh_binary_mlp_view_keys_search_fwd(const float *feat_ring, int feat_cs, int Cf, int B, int H, int W, long long key_stride,
                                                   int n_slots, const int *key_slots, int M, int h, int w, const float *rays_bn2, int N,
                                                   const float *invK_44, const float *world_T_cam_44, const float *key_cam_T_world_s44,
                                                   const float *key_K_s44, const float *prior_pred_sb1hw, const float *prior_cam_T_world_s44,
                                                   const float *prior_K_s44, int has_prior, float prior_const, const float *w1f_packed,
                                                   const float *w2_packed, const float *vecs6x128, int iters, float lo, float hi, float threshold,
                                                   const float *bins, const float *thr_logits, int n_bins, float fill, float *depth,
                                                   float *last_logits, unsigned char *flags, float *points, unsigned char *key, void *stream) {
    const ViewCams cams{invK_44, world_T_cam_44, key_cam_T_world_s44, key_K_s44, prior_cam_T_world_s44, prior_K_s44};
    const RaySource src = ray_source(rays_bn2, N, h, w);
    if (feat_bad(B, H, W, Cf, feat_cs) || src.bad || iters <= 0 || bracket_bad(lo, hi) || threshold_bad(threshold, bins, thr_logits, n_bins) ||
        prior_map_bad(prior_pred_sb1hw, has_prior, cams))
        return IDH_EINVAL;
    if (B == 0 || src.empty) return IDH_OK;
    if (view_ptrs_bad(feat_ring, cams, prior_pred_sb1hw, w1f_packed, w2_packed, vecs6x128, {depth, last_logits}, {rays_bn2, bins, thr_logits, points}))
        return IDH_EINVAL;
    KeysArgs a{};
    if (const int rc = keys_args(a, key_stride, n_slots, key_slots, M, B, H, W, feat_cs)) return rc;
    if (const int rc = size_limits<kViewKeysSearch>(B, src.Nq, H, W)) return rc;
    set_common(a, feat_ring, feat_cs, Cf, H, W, prior_pred_sb1hw, has_prior, prior_const, w1f_packed, w2_packed, vecs6x128);
    set_view(a, rays_bn2, B, src, cams, fill);
    a.iters = iters, a.lo = lo, a.hi = hi;
    set_threshold(a, threshold, bins, thr_logits, n_bins);
    set_outputs(a, last_logits, depth, flags, points);
    a.keyout = key;
    return ray_mlp_launch<kViewKeysSearch>(a, stream);
}

// First-hit depth along the rays of another camera: the samples march_depths[0 .. n_march-1] in turn until the first probe that is behind, then
// `refine` steps of idh_binary_mlp_view_search_fwd's rule inside the bracket, in one launch (view_march_k).  include/idh.h states the rule.
extern "C" int idh_binary_mlp_view_march_fwd(const float *feat_nhwc, int feat_cs, int Cf, int B, int H, int W, int h, int w, const float *rays_bn2,
                                             int N, const float *invK_44, const float *world_T_cam_44, const float *key_cam_T_world_44,
                                             const float *key_K_44, const float *prior_pred_b1hw, const float *prior_cam_T_world_44,
                                             const float *prior_K_44, int has_prior, float prior_const, const float *w1f_packed,
                                             const float *w2_packed, const float *vecs6x128, const float *march_depths, int n_march, int refine,
                                             float threshold, const float *bins, const float *thr_logits, int n_bins, float fill, float *depth,
                                             float *last_logits, unsigned char *flags, unsigned char *hit_step, float *points, void *stream) {
    const ViewCams cams{invK_44, world_T_cam_44, key_cam_T_world_44, key_K_44, prior_cam_T_world_44, prior_K_44};
    const RaySource src = ray_source(rays_bn2, N, h, w);
    if (feat_bad(B, H, W, Cf, feat_cs) || n_bins < 0 || src.bad) return IDH_EINVAL;
    if (const int rc = march_args_ok(march_depths, n_march, refine)) return rc;
    if (threshold_bad(threshold, bins, thr_logits, n_bins) || prior_map_bad(prior_pred_b1hw, has_prior, cams)) return IDH_EINVAL;
    if (B == 0 || src.empty) return IDH_OK;
    if (view_ptrs_bad(feat_nhwc, cams, prior_pred_b1hw, w1f_packed, w2_packed, vecs6x128, {depth, last_logits}, {rays_bn2, bins, thr_logits, points}))
        return IDH_EINVAL;
    if (const int rc = size_limits<kViewMarch>(B, src.Nq, H, W)) return rc;
    MarchArgs a{};
    set_common(a, feat_nhwc, feat_cs, Cf, H, W, prior_pred_b1hw, has_prior, prior_const, w1f_packed, w2_packed, vecs6x128);
    set_view(a, rays_bn2, B, src, cams, fill);
    set_threshold(a, threshold, bins, thr_logits, n_bins);
    a.march_depths = march_depths, a.n_march = n_march, a.refine = refine, a.hit_step = hit_step;
    set_outputs(a, last_logits, depth, flags, points);
    return ray_mlp_launch<kViewMarch>(a, stream);
}

// The same against M remembered keyframes: every probe selects its own key, as in idh_binary_mlp_view_keys_search_fwd (view_keys_march_k).
extern "C" int idh_binary_mlp_view_keys_march_fwd(const float *feat_ring, int feat_cs, int Cf, int B, int H, int W, long long key_stride,
                                                  int n_slots, const int *key_slots, int M, int h, int w, const float *rays_bn2, int N,
                                                  const float *invK_44, const float *world_T_cam_44, const float *key_cam_T_world_s44,
                                                  const float *key_K_s44, const float *prior_pred_sb1hw, const float *prior_cam_T_world_s44,
                                                  const float *prior_K_s44, int has_prior, float prior_const, const float *w1f_packed,
                                                  const float *w2_packed, const float *vecs6x128, const float *march_depths, int n_march,
                                                  int refine, float threshold, const float *bins, const float *thr_logits, int n_bins, float fill,
                                                  float *depth, float *last_logits, unsigned char *flags, unsigned char *hit_step, float *points,
                                                  unsigned char *key, void *stream) {
    const ViewCams cams{invK_44, world_T_cam_44, key_cam_T_world_s44, key_K_s44, prior_cam_T_world_s44, prior_K_s44};
    const RaySource src = ray_source(rays_bn2, N, h, w);
    if (feat_bad(B, H, W, Cf, feat_cs) || n_bins < 0 || src.bad) return IDH_EINVAL;
    if (const int rc = march_args_ok(march_depths, n_march, refine)) return rc;
    if (threshold_bad(threshold, bins, thr_logits, n_bins) || prior_map_bad(prior_pred_sb1hw, has_prior, cams)) return IDH_EINVAL;
    if (B == 0 || src.empty) return IDH_OK;
    if (view_ptrs_bad(feat_ring, cams, prior_pred_sb1hw, w1f_packed, w2_packed, vecs6x128, {depth, last_logits}, {rays_bn2, bins, thr_logits, points}))
        return IDH_EINVAL;
    KeysMarchArgs a{};
    if (const int rc = keys_args(a, key_stride, n_slots, key_slots, M, B, H, W, feat_cs)) return rc;
    if (const int rc = size_limits<kViewKeysMarch>(B, src.Nq, H, W)) return rc;
    set_common(a, feat_ring, feat_cs, Cf, H, W, prior_pred_sb1hw, has_prior, prior_const, w1f_packed, w2_packed, vecs6x128);
    set_view(a, rays_bn2, B, src, cams, fill);
    set_threshold(a, threshold, bins, thr_logits, n_bins);
    a.march_depths = march_depths, a.n_march = n_march, a.refine = refine, a.hit_step = hit_step;
    set_outputs(a, last_logits, depth, flags, points);
    a.keyout = key;
    return ray_mlp_launch<kViewKeysMarch>(a, stream);
}

extern "C" int idh_project_points_fwd(const float *points_bn3, const float *cam_T_world_44, const float *K_44, int B, int N, int H, int W,
                                      float *rays_bn2, float *depth_bn, unsigned char *valid_bn, const float *prior_pred_b1hw,
                                      const float *prior_cam_T_world_44, const float *prior_K_44, float *prior_bn, void *stream) {
    if (B < 0 || N < 0 || H <= 0 || W <= 0 || B > 65535) return IDH_EINVAL;
    if (B == 0 || N == 0) return IDH_OK;
    if (!points_bn3 || !cam_T_world_44 || !K_44 || !rays_bn2 || !depth_bn || !valid_bn) return IDH_EINVAL;
    if (prior_pred_b1hw && (!prior_cam_T_world_44 || !prior_K_44 || !prior_bn)) return IDH_EINVAL;
    if ((long long)B * H * W >= (1ll << 31)) return IDH_EUNSUPPORTED;
    int gx = idh_cdiv(N, 256);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(project_points_k, dim3(gx, B), dim3(256), 0, idh_stream(stream), points_bn3, cam_T_world_44, K_44, N, H, W, rays_bn2, depth_bn,
                       valid_bn, prior_pred_b1hw, prior_cam_T_world_44, prior_K_44, prior_bn);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
