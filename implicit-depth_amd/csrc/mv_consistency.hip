// Multi-view depth consistency (include/idh_geometry.h): a depth map against K source depth maps, the reference's
// MVDepthLoss arithmetic (losses.py:143-261) per pixel and source.  The header states the arithmetic; this file follows it expression
// by expression.
//
//   mv_consistency_k<GATE, LOSS>  one lane per pixel, a workgroup of 256 consecutive pixels of one map, a loop over the K sources.  The
//                     K projections P = K E are formed once per workgroup (one entry per thread) and read from LDS, where every lane
//                     reads the same word; the map's own matrices are wave-uniform (scalar loads).  Per source one gather of the
//                     source's depth.  GATE runs the chain a second time for the gate map.  LOSS reduces err per source: the wave
//                     by shuffles, the four waves through LDS, one {sum, count} partial per workgroup and source.  The err it sums
//                     is evaluated in fp64 (the tested map's chain and two logs per visible entry); masks and planes stay fp32.
//   mv_loss_finalise_k  one workgroup: per source the partials summed in a fixed order in fp64, then the mean of the K means.
// No atomics anywhere.
#include <math.h>

#include "../../include/idh_geometry.h"
#include "idh_common.h"

namespace {

__device__ __forceinline__ bool valid_depth(float d) { return d > 0.f && d < INFINITY; }  // false for NaN: the rule of tsdf.hip

struct MvArgs {
    const float *depth, *gate, *invK, *E, *sdepth, *sK, *sE;
    uint8_t *counts, *visible;
    float *weight, *filtered, *err;
    double *psum;      // (workgroups, K)
    long long *pcnt;   // (workgroups, K)
    float ratio, log_tol;
    int min_consistent, max_conflict, K, hw, w, h;
};

// a0 b0 + a1 b1 + a2 b2 + a3 b3, left to right, every further product fused into the running sum: the matrix products of the reference
// run on BLAS kernels built from fused multiply-adds, and where the terms cancel (a camera plane through the point) the unfused sum
// is several times further from the fp64 value than the reference's own fp32 run
__device__ __forceinline__ float dot4(float a0, float b0, float a1, float b1, float a2, float b2, float a3, float b3) {
    return fmaf(a3, b3, fmaf(a2, b2, fmaf(a1, b1, a0 * b0)));
}

// depth d at pixel direction q -> the point in the world, four components (the reference multiplies the homogeneous 4-vector through)
__device__ __forceinline__ void to_world(const float *__restrict__ E, float d, float qx, float qy, float qz, float X[4]) {
    const float cx = d * qx, cy = d * qy, cz = d * qz;
#pragma unroll
    for (int r = 0; r < 4; ++r) X[r] = dot4(E[r * 4 + 0], cx, E[r * 4 + 1], cy, E[r * 4 + 2], cz, E[r * 4 + 3], 1.f);
}

// torch.maximum(z, eps): a NaN stays a NaN (fmaxf would return the clamp)
__device__ __forceinline__ float clamp_z(float z) { return z < 1e-5f ? 1e-5f : z; }

__device__ __forceinline__ float row_dot(const float *P, const float X[4]) { return dot4(P[0], X[0], P[1], X[1], P[2], X[2], P[3], X[3]); }

template <bool GATE, bool LOSS>
__global__ __launch_bounds__(256) void mv_consistency_k(const MvArgs a) {
    __shared__ float sP[IDH_MV_MAX_SOURCES][12];
    __shared__ double sSum[IDH_MV_MAX_SOURCES][4];
    __shared__ double sPz[IDH_MV_MAX_SOURCES][4];  // LOSS: the z row of P in fp64
    __shared__ int sCnt[IDH_MV_MAX_SOURCES][4];
    const int b = blockIdx.y, K = a.K, t = threadIdx.x;
    if (t < K * 12) {
        const int k = t / 12, e = t - k * 12, r = e >> 2, c = e & 3;
        const float *Km = a.sK + ((size_t)b * K + k) * 16 + r * 4, *Em = a.sE + ((size_t)b * K + k) * 16 + c;
        sP[k][e] = dot4(Km[0], Em[0], Km[1], Em[4], Km[2], Em[8], Km[3], Em[12]);
    }
    if (LOSS && t >= 192 && t < 192 + K * 4) {
        const int k = (t - 192) >> 2, c = (t - 192) & 3;
        const float *Km = a.sK + ((size_t)b * K + k) * 16 + 8, *Em = a.sE + ((size_t)b * K + k) * 16 + c;
        sPz[k][c] = (((double)Km[0] * Em[0] + (double)Km[1] * Em[4]) + (double)Km[2] * Em[8]) + (double)Km[3] * Em[12];
    }
    __syncthreads();
    const int pix = blockIdx.x * 256 + t;
    const bool live = pix < a.hw;
    const int p = live ? pix : 0;  // a lane past the end works on pixel 0 and stores nothing
    const int i = p / a.w, j = p - i * a.w;
    const float *iK = a.invK + (size_t)b * 16, *E = a.E + (size_t)b * 16;  // wave-uniform
    const float u = (float)j + 0.5f, v = (float)i + 0.5f;
    const float qx = fmaf(iK[1], v, iK[0] * u) + iK[2], qy = fmaf(iK[5], v, iK[4] * u) + iK[6], qz = fmaf(iK[9], v, iK[8] * u) + iK[10];
    const float d = a.depth[(size_t)b * a.hw + p];
    float Xt[4], Xg[4];
    to_world(E, d, qx, qy, qz, Xt);
    if (GATE) to_world(E, a.gate[(size_t)b * a.hw + p], qx, qy, qz, Xg);
    const float *X = GATE ? Xg : Xt;  // the chain px, py, s and the gate's z come from
    const bool d_ok = valid_depth(d);
    // LOSS: the tested point once more in fp64.  The err the loss averages is evaluated in fp64 from the same fp32 inputs: the fp32
    // chain's rounding is not free of bias (a few 1e-8 relative in z per source, one sign over a whole map), which a mean over
    // thousands of pixels keeps and which is as large as the last bit of the float the loss is returned in.
    double Xd[4] = {0.0, 0.0, 0.0, 0.0};
    if (LOSS) {
        const double ud = (double)u, vd = (double)v, dd = (double)d;
        const double cx = dd * (((double)iK[0] * ud + (double)iK[1] * vd) + (double)iK[2]);
        const double cy = dd * (((double)iK[4] * ud + (double)iK[5] * vd) + (double)iK[6]);
        const double cz = dd * (((double)iK[8] * ud + (double)iK[9] * vd) + (double)iK[10]);
#pragma unroll
        for (int r = 0; r < 4; ++r) Xd[r] = (((double)E[r * 4] * cx + (double)E[r * 4 + 1] * cy) + (double)E[r * 4 + 2] * cz) + (double)E[r * 4 + 3];
    }
    const float fw = (float)a.w, fh = (float)a.h;
    int n_vis = 0, n_con = 0, n_conf = 0;
    for (int k = 0; k < K; ++k) {
        const float *P = sP[k];
        const float z_gate = clamp_z(row_dot(P + 8, X));
        const float px = row_dot(P, X) / z_gate, py = row_dot(P + 4, X) / z_gate;
        const float z_test = GATE ? clamp_z(row_dot(P + 8, Xt)) : z_gate;
        const float xr = rintf(px - 0.5f), yr = rintf(py - 0.5f);  // round-half-even (the rule of mlp.hip's sample_prior_k)
        const bool inside = xr >= 0.f && xr <= fw - 1.f && yr >= 0.f && yr <= fh - 1.f;  // false for NaN
        float s = 0.f;
        if (inside) s = a.sdepth[((size_t)b * K + k) * a.hw + (size_t)(int)yr * a.w + (int)xr];
        const bool vis = z_gate < a.ratio * s && z_gate > 0.f && s > 0.f;
        const float l = logf(s) - logf(z_test), err = fabsf(l);
        const bool counted = vis && d_ok && valid_depth(s) && inside;
        n_vis += vis, n_con += counted && err <= a.log_tol, n_conf += counted && l > a.log_tol;
        if (live) {
            const size_t o = ((size_t)b * K + k) * a.hw + p;
            if (a.visible) a.visible[o] = vis;
            if (a.err) a.err[o] = vis ? err : NAN;
        }
        if (LOSS) {
            const bool take = live && vis && err == err;  // nanmean skips the NaNs among the selected (the fp32 plane's, so counts match it)
            double sum = 0.0;
            if (take) {
                double zd = ((sPz[k][0] * Xd[0] + sPz[k][1] * Xd[1]) + sPz[k][2] * Xd[2]) + sPz[k][3] * Xd[3];
                zd = zd < (double)1e-5f ? (double)1e-5f : zd;
                sum = fabs(log((double)s) - log(zd));
            }
            int cnt = take;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64), cnt += __shfl_down(cnt, off, 64);
            if ((t & 63) == 0) sSum[k][t >> 6] = sum, sCnt[k][t >> 6] = cnt;
        }
    }
    if (live) {
        const bool kept = d_ok && n_con >= a.min_consistent && n_conf <= a.max_conflict;
        if (a.counts) {
            uint8_t *c = a.counts + (size_t)b * 3 * a.hw + p;
            c[0] = (uint8_t)n_vis, c[a.hw] = (uint8_t)n_con, c[2 * (size_t)a.hw] = (uint8_t)n_conf;
        }
        if (a.weight) a.weight[(size_t)b * a.hw + p] = kept ? 1.f + (float)n_con : 0.f;
        if (a.filtered) a.filtered[(size_t)b * a.hw + p] = kept ? d : 0.f;
    }
    if (LOSS) {
        __syncthreads();
        if (t < K) {
            const size_t o = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * K + t;
            a.psum[o] = ((sSum[t][0] + sSum[t][1]) + sSum[t][2]) + sSum[t][3];
            a.pcnt[o] = (long long)(((sCnt[t][0] + sCnt[t][1]) + sCnt[t][2]) + sCnt[t][3]);
        }
    }
}

// thread t adds partials t, t + 256, ...; the 256 sums are folded pairwise through LDS: one order, whatever the launch
__global__ __launch_bounds__(256) void mv_loss_finalise_k(const double *__restrict__ psum, const long long *__restrict__ pcnt, int n, int K,
                                                          float *__restrict__ loss, double *__restrict__ sum_k, long long *__restrict__ cnt_k) {
    __shared__ double sS[256];
    __shared__ long long sC[256];
    const int t = threadIdx.x;
    double total = 0.0;
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        long long c = 0;
        for (int i = t; i < n; i += 256) s += psum[(size_t)i * K + k], c += pcnt[(size_t)i * K + k];
        sS[t] = s, sC[t] = c;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (t < off) sS[t] += sS[t + off], sC[t] += sC[t + off];
            __syncthreads();
        }
        if (t == 0) {
            if (sum_k) sum_k[k] = sS[0];
            if (cnt_k) cnt_k[k] = sC[0];
            total += sS[0] / (double)sC[0];  // 0 / 0: NaN, the nanmean of an empty selection
        }
        __syncthreads();
    }
    if (t == 0) *loss = (float)(total / (double)K);
}

}  // namespace

extern "C" size_t idh_sizeof_mv_consistency_args(void) { return sizeof(idh_mv_consistency_args); }

extern "C" size_t idh_mv_consistency_workspace_bytes(int B, int K, int h, int w) {
    if (B <= 0 || K <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)16 * K * B * (size_t)(((long long)h * w + 255) / 256);
}

extern "C" int idh_mv_consistency_fwd(const idh_mv_consistency_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_mv_consistency_args)) return IDH_EINVAL;
    const idh_mv_consistency_args &e = *args;
    if (e.B < 0 || e.K <= 0 || e.h <= 0 || e.w <= 0 || e.src_h <= 0 || e.src_w <= 0) return IDH_EINVAL;
    if (!(e.ratio > 0.f && e.ratio < INFINITY) || !(e.log_tol > 0.f && e.log_tol < INFINITY)) return IDH_EINVAL;
    if (e.min_consistent < 0 || e.max_conflict < 0) return IDH_EINVAL;
    if (!e.depth_b1hw || !e.invK_b44 || !e.world_T_cam_b44 || !e.src_depth_bk1hw || !e.src_K_bk44 || !e.src_cam_T_world_bk44) return IDH_EINVAL;
    if (!e.loss && (e.loss_sum_k || e.loss_count_k)) return IDH_EINVAL;
    if (e.loss && ((uintptr_t)e.workspace & 7u)) return IDH_EINVAL;
    if (e.K > IDH_MV_MAX_SOURCES || e.B > IDH_MV_MAX_MAPS || e.src_h != e.h || e.src_w != e.w) return IDH_EUNSUPPORTED;
    if ((long long)e.B * e.K * e.h * e.w >= (1ll << 31) || (long long)e.h * e.w >= (1ll << 31)) return IDH_EUNSUPPORTED;
    if (e.B == 0) return IDH_OK;
    const int tiles = idh_cdiv((long long)e.h * e.w, 256);
    const long long n = (long long)tiles * e.B;
    if (e.loss && (!e.workspace || e.workspace_bytes < (int64_t)idh_mv_consistency_workspace_bytes(e.B, e.K, e.h, e.w))) return IDH_EWORKSPACE;
    MvArgs a;
    a.depth = e.depth_b1hw, a.gate = e.gate_depth_b1hw, a.invK = e.invK_b44, a.E = e.world_T_cam_b44;
    a.sdepth = e.src_depth_bk1hw, a.sK = e.src_K_bk44, a.sE = e.src_cam_T_world_bk44;
    a.counts = e.counts_b3hw, a.visible = e.visible_bkhw, a.weight = e.weight_b1hw, a.filtered = e.filtered_depth_b1hw, a.err = e.err_bkhw;
    a.psum = e.loss ? static_cast<double *>(e.workspace) : nullptr;
    a.pcnt = e.loss ? reinterpret_cast<long long *>(a.psum + n * e.K) : nullptr;
    a.ratio = e.ratio, a.log_tol = e.log_tol, a.min_consistent = e.min_consistent, a.max_conflict = e.max_conflict;
    a.K = e.K, a.hw = e.h * e.w, a.w = e.w, a.h = e.h;
    hipStream_t st = idh_stream(stream);
    const dim3 grid(tiles, e.B);
    if (e.gate_depth_b1hw) {
        if (e.loss) hipLaunchKernelGGL((mv_consistency_k<true, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((mv_consistency_k<true, false>), grid, dim3(256), 0, st, a);
    } else {
        if (e.loss) hipLaunchKernelGGL((mv_consistency_k<false, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((mv_consistency_k<false, false>), grid, dim3(256), 0, st, a);
    }
    IDH_CHECK_LAUNCH();
    if (e.loss) {
        hipLaunchKernelGGL(mv_loss_finalise_k, dim3(1), dim3(256), 0, st, a.psum, a.pcnt, (int)n, e.K, e.loss, e.loss_sum_k,
                           reinterpret_cast<long long *>(e.loss_count_k));
        IDH_CHECK_LAUNCH();
    }
    return IDH_OK;
}
