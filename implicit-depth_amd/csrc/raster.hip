// Depth-only mesh rasterisation and the vertex bookkeeping of the temporal evaluation (include/idh_raster.h): what the reference does
// with pytorch3d's rasteriser in utils/binary_metrics_utils.py:283-388 and with torch in :273-280.
//
//   raster_vertex_k   world -> camera -> screen, once per vertex and camera.
//   raster_face_k     one lane per face: culls (index out of range, non-finite, wholly at z <= 0, zero area, bounding box off screen) and
//                     resolves a face whose box holds at most kSmallBox pixel centres in place; larger and z = 0-straddling faces go
//                     to a queue.
//   raster_large_k    one wave per queued face, its 64 lanes striding over the 8 x 8-pixel tiles of the face's box (the whole image for a
//                     straddling face); a tile wholly outside one edge is skipped.
//   raster_resolve_k  +inf -> -1.
// The output doubles as the z-buffer: z > 0, so the unsigned order of the bit pattern is the float order and an atomicMin on it picks the
// nearest hit whatever the order of arrival.
//
// The ray test runs in camera space (no projection of the triangle, hence no clipping): with camera-space corners A, B, C and pixel ray
// d = ((u - cx) / fx, (v - cy) / fy, 1), the ray meets the triangle's plane at z = N.A / N.d, N = (B - A) x (C - A), inside when
// d.(B x C), d.(C x A), d.(A x B) all carry the sign of N.A.  P x Q is computed as L x (H - L) from the lower-numbered corner L of the
// edge (negated when that swaps the operands): the difference keeps full precision for the small far triangles whose P and Q are nearly
// parallel, and the two triangles of a shared edge get exactly negated normals.  Built with -ffp-contract=off.
#include <math.h>

#include <algorithm>

#include "../../include/idh_raster.h"
#include "idh_common.h"

namespace {

constexpr int kSmallBox = 64;      // pixel centres a single lane resolves itself (one wave's width); above: queued for a wave
constexpr float kBoxPad = 1.f / 64;  // px added round a projected box: far above the fp32 error of a projected on-screen coordinate (~3e-5 px)
constexpr unsigned kInfBits = 0x7f800000u;
constexpr int kLargeBlocks = 1024;  // persistent workgroups of raster_large_k (4 waves each)

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 scale(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

struct Cam {
    float r[12];  // rows of [R | t]
    float fx, fy, cx, cy;
};

__device__ __forceinline__ Cam load_cam(const float *cam_T_world, const float *K) {
    Cam c;
#pragma unroll
    for (int i = 0; i < 12; ++i) c.r[i] = cam_T_world[i];
    c.fx = K[0], c.cx = K[2], c.fy = K[5], c.cy = K[6];
    return c;
}

__device__ __forceinline__ V3 to_camera(const Cam &c, const float *v) {
    const float X = v[0], Y = v[1], Z = v[2];
    return {c.r[0] * X + c.r[1] * Y + c.r[2] * Z + c.r[3], c.r[4] * X + c.r[5] * Y + c.r[6] * Z + c.r[7],
            c.r[8] * X + c.r[9] * Y + c.r[10] * Z + c.r[11]};
}

// ---- vertex pass --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void raster_vertex_k(const float *__restrict__ verts, int V, const float *__restrict__ cam_T_world,
                                                       const float *__restrict__ K, float4 *__restrict__ cam, float2 *__restrict__ scr) {
    const int b = blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const Cam c = load_cam(cam_T_world + b * 16, K + b * 16);
    const V3 p = to_camera(c, verts + (size_t)v * 3);
    cam[(size_t)b * V + v] = make_float4(p.x, p.y, p.z, 0.f);
    // screen position; only read for vertices with z > 0 (a denormal z may give +-inf: the box is clamped to the image)
    scr[(size_t)b * V + v] = make_float2(c.fx * (p.x / p.z) + c.cx, c.fy * (p.y / p.z) + c.cy);
}

// ---- one triangle -------------------------------------------------------------------------------------------
struct Tri {
    V3 n0, n1, n2, N;  // edge normals B x C, C x A, A x B and the plane normal, all signed so that k > 0
    float k;           // N.A
    int x0, x1, y0, y1;  // inclusive box of pixel centres (empty when x1 < x0 or y1 < y0)
    bool straddles;
};

// P x Q from the lower-numbered corner of the edge
__device__ __forceinline__ V3 edge_normal(V3 P, int ip, V3 Q, int iq) {
    const bool swap = ip > iq;
    const V3 L = swap ? Q : P, Hi = swap ? P : Q;
    const V3 n = cross(L, sub(Hi, L));
    return swap ? V3{-n.x, -n.y, -n.z} : n;
}

// false: the face draws nothing
__device__ __forceinline__ bool tri_setup(const float4 *__restrict__ cam, const float2 *__restrict__ scr, const int *__restrict__ face, int V,
                                          int H, int W, Tri &t) {
    const int ia = face[0], ib = face[1], ic = face[2];
    if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) return false;
    const float4 a4 = cam[ia], b4 = cam[ib], c4 = cam[ic];
    const V3 A{a4.x, a4.y, a4.z}, B{b4.x, b4.y, b4.z}, C{c4.x, c4.y, c4.z};
    if (!(finite3(A) && finite3(B) && finite3(C))) return false;
    const int front = (A.z > 0.f) + (B.z > 0.f) + (C.z > 0.f);
    if (front == 0) return false;
    t.N = cross(sub(B, A), sub(C, A));
    t.k = dot(t.N, A);
    if (!(fabsf(t.k) > 0.f) || !isfinite(t.k)) return false;  // zero area, or a plane through the eye: no ray meets it at z > 0
    const float s = t.k > 0.f ? 1.f : -1.f;
    t.N = scale(t.N, s);
    t.k *= s;
    t.n0 = scale(edge_normal(B, ib, C, ic), s);
    t.n1 = scale(edge_normal(C, ic, A, ia), s);
    t.n2 = scale(edge_normal(A, ia, B, ib), s);
    t.straddles = front != 3;
    if (t.straddles) {  // its projection is not the triangle of its projected corners: test the whole image
        t.x0 = 0, t.x1 = W - 1, t.y0 = 0, t.y1 = H - 1;
        return true;
    }
    const float2 pa = scr[ia], pb = scr[ib], pc = scr[ic];
    const float u0 = fminf(pa.x, fminf(pb.x, pc.x)), u1 = fmaxf(pa.x, fmaxf(pb.x, pc.x));
    const float v0 = fminf(pa.y, fminf(pb.y, pc.y)), v1 = fmaxf(pa.y, fmaxf(pb.y, pc.y));
    // pixel centres j + 0.5 inside [u0 - pad, u1 + pad], clamped to the image in float (the ends may be infinite)
    t.x0 = (int)fminf(fmaxf(ceilf(u0 - 0.5f - kBoxPad), 0.f), (float)W);
    t.x1 = (int)fmaxf(fminf(floorf(u1 - 0.5f + kBoxPad), (float)(W - 1)), -1.f);
    t.y0 = (int)fminf(fmaxf(ceilf(v0 - 0.5f - kBoxPad), 0.f), (float)H);
    t.y1 = (int)fmaxf(fminf(floorf(v1 - 0.5f + kBoxPad), (float)(H - 1)), -1.f);
    return t.x1 >= t.x0 && t.y1 >= t.y0;
}

__device__ __forceinline__ void shade(const Tri &t, const Cam &c, int x, int y, int W, unsigned *__restrict__ zbuf) {
    const V3 d{((float)x + 0.5f - c.cx) / c.fx, ((float)y + 0.5f - c.cy) / c.fy, 1.f};
    const float e0 = dot(d, t.n0), e1 = dot(d, t.n1), e2 = dot(d, t.n2);
    if (e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) {
        const float den = dot(d, t.N);
        const float z = t.k / den;
        if (den > 0.f && z > 0.f && z < INFINITY) atomicMin(zbuf + (size_t)y * W + x, __float_as_uint(z));
    }
}

struct RasterArgs {
    const float4 *cam;  // (B,V)
    const float2 *scr;  // (B,V)
    const int *faces;   // (F,3)
    const float *cam_T_world, *K;
    int V, F, H, W;
    unsigned *zbuf;    // (B,H,W)
    unsigned *queue;   // (B,F)
    unsigned *qcount;  // (B)
};

// ---- face pass ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void raster_face_k(const RasterArgs a) {
    const int b = blockIdx.y;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= a.F) return;
    Tri t;
    if (!tri_setup(a.cam + (size_t)b * a.V, a.scr + (size_t)b * a.V, a.faces + (size_t)f * 3, a.V, a.H, a.W, t)) return;
    const int bw = t.x1 - t.x0 + 1, n = bw * (t.y1 - t.y0 + 1);
    if (t.straddles || n > kSmallBox) {
        const unsigned slot = atomicAdd(a.qcount + b, 1u);  // < F: every face is appended at most once
        a.queue[(size_t)b * a.F + slot] = (unsigned)f;
        return;
    }
    const Cam c = load_cam(a.cam_T_world + b * 16, a.K + b * 16);
    unsigned *zb = a.zbuf + (size_t)b * a.H * a.W;
    for (int y = t.y0; y <= t.y1; ++y)
        for (int x = t.x0; x <= t.x1; ++x) shade(t, c, x, y, a.W, zb);
}

// ---- queued faces: a wave each ------------------------------------------------------------------------------
// The lanes stride over the kTile x kTile-pixel tiles of the face's box.  A tile is skipped when one edge function is negative at the
// pixel centres of all four of its corners: fp32 multiplication by a constant and fp32 addition are monotone, so dot(d, n) as shade()
// evaluates it is monotone in the pixel's column and in its row, and its largest value over the tile is taken at a corner — the skipped
// pixels are exactly pixels shade() would reject, and the cost of a face (a straddling one, whose box is the image, above all) follows
// the area it covers rather than the area of its box.
constexpr int kTile = 8;

__device__ __forceinline__ bool tile_outside(const Tri &t, const Cam &c, int x0, int x1, int y0, int y1) {
    const float dx0 = ((float)x0 + 0.5f - c.cx) / c.fx, dx1 = ((float)x1 + 0.5f - c.cx) / c.fx;
    const float dy0 = ((float)y0 + 0.5f - c.cy) / c.fy, dy1 = ((float)y1 + 0.5f - c.cy) / c.fy;
    const V3 d00{dx0, dy0, 1.f}, d01{dx1, dy0, 1.f}, d10{dx0, dy1, 1.f}, d11{dx1, dy1, 1.f};
    const V3 *n[3] = {&t.n0, &t.n1, &t.n2};
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (dot(d00, *n[i]) < 0.f && dot(d01, *n[i]) < 0.f && dot(d10, *n[i]) < 0.f && dot(d11, *n[i]) < 0.f) return true;
    return false;
}

__global__ __launch_bounds__(256) void raster_large_k(const RasterArgs a) {
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    const unsigned count = min(a.qcount[b], (unsigned)a.F);
    const Cam c = load_cam(a.cam_T_world + b * 16, a.K + b * 16);
    unsigned *zb = a.zbuf + (size_t)b * a.H * a.W;
    for (unsigned q = wave; q < count; q += nwaves) {
        const unsigned f = a.queue[(size_t)b * a.F + q];
        if (f >= (unsigned)a.F) continue;
        Tri t;
        if (!tri_setup(a.cam + (size_t)b * a.V, a.scr + (size_t)b * a.V, a.faces + (size_t)f * 3, a.V, a.H, a.W, t)) continue;
        const int tw = (t.x1 - t.x0) / kTile + 1, nt = tw * ((t.y1 - t.y0) / kTile + 1);
        for (int i = lane; i < nt; i += 64) {
            const int ty = i / tw;
            const int x0 = t.x0 + (i - ty * tw) * kTile, y0 = t.y0 + ty * kTile;
            const int x1 = min(x0 + kTile - 1, t.x1), y1 = min(y0 + kTile - 1, t.y1);
            if (tile_outside(t, c, x0, x1, y0, y1)) continue;
            for (int y = y0; y <= y1; ++y)
                for (int x = x0; x <= x1; ++x) shade(t, c, x, y, a.W, zb);
        }
    }
}

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

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t idh_raster_workspace_bytes(int B, int V, int F) {
    if (B < 0 || V < 0 || F < 0) return 0;
    const size_t bv = (size_t)B * (size_t)V;
    return align256(bv * sizeof(float4)) + align256(bv * sizeof(float2)) + align256((size_t)B * (size_t)F * sizeof(unsigned)) +
           align256((size_t)B * sizeof(unsigned)) + 256;
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
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    const size_t bv = (size_t)B * (size_t)V;
    float4 *cam = reinterpret_cast<float4 *>(ws);
    ws += align256(bv * sizeof(float4));
    float2 *scr = reinterpret_cast<float2 *>(ws);
    ws += align256(bv * sizeof(float2));
    unsigned *queue = reinterpret_cast<unsigned *>(ws);
    ws += align256((size_t)B * (size_t)F * sizeof(unsigned));
    unsigned *qcount = reinterpret_cast<unsigned *>(ws);
    const long long n = (long long)B * H * W;
    unsigned *zbuf = reinterpret_cast<unsigned *>(out_b1hw);
    hipLaunchKernelGGL(raster_fill_k, dim3(idh_cdiv(n > B ? n : B, 256)), dim3(256), 0, st, zbuf, n, qcount, B);
    IDH_CHECK_LAUNCH();
    if (V > 0 && F > 0) {
        hipLaunchKernelGGL(raster_vertex_k, dim3(idh_cdiv(V, 256), B), dim3(256), 0, st, verts_v3, V, cam_T_world_b44, K_b44, cam, scr);
        IDH_CHECK_LAUNCH();
        const RasterArgs a{cam, scr, faces_f3, cam_T_world_b44, K_b44, V, F, H, W, zbuf, queue, qcount};
        hipLaunchKernelGGL(raster_face_k, dim3(idh_cdiv(F, 256), B), dim3(256), 0, st, a);
        IDH_CHECK_LAUNCH();
        hipLaunchKernelGGL(raster_large_k, dim3(std::min(kLargeBlocks, idh_cdiv(F, 4)), B), dim3(256), 0, st, a);
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
