// Depth-only mesh rasterisation and the vertex bookkeeping of the temporal evaluation (include/idh_raster.h): what the reference does
// with pytorch3d's rasteriser in utils/binary_metrics_utils.py:283-388 and with torch in :273-280.
//
//   raster_vertex_k / raster_face_k / raster_large_k   the passes of raster_common.h, with the depth sink below.
//   raster_resolve_k                                   +inf -> -1.
// The output doubles as the z-buffer: z > 0, so the unsigned order of the bit pattern is the float order and an atomicMin on it picks the
// nearest hit whatever the order of arrival.  The geometry (camera-space ray test, edge rule, culls) is stated in raster_common.h.
#include <math.h>

#include <algorithm>

#include "../../include/idh_raster.h"
#include "idh_common.h"
#include "raster_common.h"

namespace {

// the z-buffer of the depth-only path: the float's bits, 32-bit atomic minimum
struct DepthSink {
    unsigned *zbuf;
    __device__ __forceinline__ DepthSink camera(size_t first_pixel) const { return {zbuf + first_pixel}; }
    __device__ __forceinline__ void hit(size_t pixel, float z, unsigned) const { atomicMin(zbuf + pixel, __float_as_uint(z)); }
};

__global__ __launch_bounds__(256) void raster_fill_k(unsigned *__restrict__ p, long long n, unsigned *__restrict__ qcount, int B) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i < n) p[i] = kInfBits;
    if (i < B) qcount[i] = 0u;
}

__global__ __launch_bounds__(256) void raster_resolve_k(float *__restrict__ p, long long n) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i < n && __float_as_uint(p[i]) == kInfBits) p[i] = -1.f;
}

// ---- vertex predictions (binary_metrics_utils.py:364-386) -----------------------------------------------------
// index of grid_sample's nearest tap for screen coordinate s (align_corners=False: s - 0.5, ties to even), -1 outside [0, n)
__device__ __forceinline__ int nearest_tap(float s, int n) {
    const float r = nearbyintf(s - 0.5f);
    return r >= 0.f && r < (float)n ? (int)r : -1;
}

__global__ __launch_bounds__(256) void vertex_predictions_k(const float *__restrict__ verts, int V, const float *__restrict__ cam_T_world,
                                                            const float *__restrict__ K, const float *__restrict__ pred,
                                                            const float *__restrict__ depth, int H, int W, float tol, float *__restrict__ out) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const Cam c = load_cam(cam_T_world, K);
    const V3 p = to_camera(c, verts + (size_t)v * 3);
    float r = -1.f;
    if (p.z > 0.f) {  // (:380); false for NaN
        const int ix = nearest_tap(c.fx * (p.x / p.z) + c.cx, W), iy = nearest_tap(c.fy * (p.y / p.z) + c.cy, H);
        if (ix >= 0 && iy >= 0) {  // zero padding: both samples 0 outside, which fails depth_s > 0
            const float ps = pred[(size_t)iy * W + ix], ds = depth[(size_t)iy * W + ix];
            if (ds > 0.f && fabsf(p.z - ds) < tol && ps > 0.f) r = ps;
        }
    }
    out[v] = r;
}

// ---- occlusion changes (binary_metrics_utils.py:273-280) -----------------------------------------------------
// class in units of 0.5: 0 (< 0.5), 1 (exactly 0.5, which the reference leaves as it is), 2 (> 0.5); -1 unknown (-1 or NaN)
__device__ __forceinline__ int occlusion_class(float p) {
    if (p == -1.f || p != p) return -1;
    return p > 0.5f ? 2 : (p < 0.5f ? 0 : 1);
}

__global__ __launch_bounds__(256) void occlusion_changes_k(const float *__restrict__ hist, int T, int V, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[4];
    unsigned long long s = 0;
    for (long long v = blockIdx.x * 256ll + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
        int prev = occlusion_class(hist[v]);
        for (int t = 1; t < T; ++t) {
            const int cur = occlusion_class(hist[(size_t)t * V + v]);
            if (prev >= 0 && cur >= 0) s += (unsigned)abs(cur - prev);
            prev = cur;
        }
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tot = red[0] + red[1] + red[2] + red[3];
        if (tot) atomicAdd(out, tot);
    }
}

}  // namespace

extern "C" size_t idh_raster_workspace_bytes(int B, int V, int F) {
    if (B < 0 || V < 0 || F < 0) return 0;
    return raster_scratch_bytes(B, V, F) + 256;
}

extern "C" int idh_raster_depth_fwd(const float *verts_v3, int V, const int32_t *faces_f3, int F, const float *cam_T_world_b44,
                                    const float *K_b44, int B, int H, int W, float *out_b1hw, void *workspace, size_t workspace_bytes,
                                    void *stream) {
    if (B < 0 || V < 0 || F < 0 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31)) return IDH_EINVAL;
    if (B == 0) return IDH_OK;
    if ((long long)B * H * W >= (1ll << 31)) return IDH_EUNSUPPORTED;  // one 32-bit grid of 256-lane workgroups fills / resolves the output
    if (!out_b1hw || !cam_T_world_b44 || !K_b44 || (V > 0 && !verts_v3) || (F > 0 && !faces_f3)) return IDH_EINVAL;
    if (!workspace || workspace_bytes < idh_raster_workspace_bytes(B, V, F) || ((uintptr_t)workspace & 255)) return IDH_EWORKSPACE;
    if (B > 65535) return IDH_EUNSUPPORTED;
    hipStream_t st = idh_stream(stream);
    const RasterScratch w = raster_scratch(workspace, B, V, F);
    const long long n = (long long)B * H * W;
    unsigned *zbuf = reinterpret_cast<unsigned *>(out_b1hw);
    hipLaunchKernelGGL(raster_fill_k, dim3(idh_cdiv(n > B ? n : B, 256)), dim3(256), 0, st, zbuf, n, w.qcount, B);
    IDH_CHECK_LAUNCH();
    if (V > 0 && F > 0) {
        hipLaunchKernelGGL(raster_vertex_k, dim3(idh_cdiv(V, 256), B), dim3(256), 0, st, verts_v3, V, cam_T_world_b44, K_b44, w.cam, w.scr);
        IDH_CHECK_LAUNCH();
        const RasterArgs<DepthSink> a{w.cam, w.scr, faces_f3, cam_T_world_b44, K_b44, V, F, H, W, DepthSink{zbuf}, w.queue, w.qcount};
        hipLaunchKernelGGL(raster_face_k<DepthSink>, dim3(idh_cdiv(F, 256), B), dim3(256), 0, st, a);
        IDH_CHECK_LAUNCH();
        hipLaunchKernelGGL(raster_large_k<DepthSink>, dim3(std::min(kLargeBlocks, idh_cdiv(F, 4)), B), dim3(256), 0, st, a);
        IDH_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(raster_resolve_k, dim3(idh_cdiv(n, 256)), dim3(256), 0, st, out_b1hw, n);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_vertex_predictions_fwd(const float *verts_v3, int V, const float *cam_T_world_44, const float *K_44, const float *pred_11hw,
                                          const float *depth_11hw, int H, int W, float depth_tolerance, float *out_v, void *stream) {
    if (V < 0 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31)) return IDH_EINVAL;
    if (V == 0) return IDH_OK;
    if (!verts_v3 || !cam_T_world_44 || !K_44 || !pred_11hw || !depth_11hw || !out_v) return IDH_EINVAL;
    hipLaunchKernelGGL(vertex_predictions_k, dim3(idh_cdiv(V, 256)), dim3(256), 0, idh_stream(stream), verts_v3, V, cam_T_world_44, K_44,
                       pred_11hw, depth_11hw, H, W, depth_tolerance, out_v);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_vertex_occlusion_changes_fwd(const float *hist_tv, int T, int V, long long *half_units_out, void *stream) {
    if (T < 0 || V < 0) return IDH_EINVAL;
    if (!half_units_out || (T > 0 && V > 0 && !hist_tv)) return IDH_EINVAL;
    hipStream_t st = idh_stream(stream);
    if (hipMemsetAsync(half_units_out, 0, sizeof(long long), st) != hipSuccess) return IDH_ELAUNCH;
    if (T < 2 || V == 0) return IDH_OK;
    hipLaunchKernelGGL(occlusion_changes_k, dim3(std::min(idh_cdiv(V, 256), 2048)), dim3(256), 0, st, hist_tv, T, V,
                       reinterpret_cast<unsigned long long *>(half_units_out));
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
