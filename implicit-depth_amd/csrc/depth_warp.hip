// Depth reprojection (include/idh_raster.h): M keyframe depth maps drawn into B live cameras as triangulated surfaces,
// torn at depth discontinuities, all M sources of a target into one z-buffer.  The depth path of the reference's compositor
// (inference/composite.py:104-134 with depth_pred_s0_b1hw or lidar) takes a depth map in the camera it composites into; this moves a map
// predicted or measured at a keyframe into the camera of the frames between.
//
//   warp_fill_k     the key plane to "empty", the queue counters to 0.
//   warp_face_k     one lane per implicit face: validity and tear test on its three source depths, its three vertices (back-projection
//                   as BackprojectDepth, utils/geometry_utils.py:39,60-61, then cam_T_src and the projection), then the setup and ray
//                   test of raster_common.h; a box above kSmallBox pixel centres or a face across z = 0 is queued.
//   warp_large_k    one wave per queued face over 8 x 8-pixel tiles, tile_outside skipping those wholly outside an edge.
//   warp_resolve_k  +inf -> empty_depth, the key's lower word -> the source id.
//
// There is no face list and no vertex buffer: face f of a h x w map is quad q = f >> 1 = i * (w - 1) + j with
// corners v00 = (i, j), v01 = (i, j + 1), v10 = (i + 1, j), v11 = (i + 1, j + 1); the even face is (v00, v10, v01), the odd one
// (v01, v10, v11).  Vertex numbers i * w + j order the shared edges for edge_normal.  A form that stored the transformed vertices in
// a vertex pass (24 B written per vertex, 72 B gathered back per face) returned the same bits and measured 4 - 22 % slower; it was
// removed (profiles/warp/README.md).
#include <math.h>

#include <algorithm>

#include "../../include/idh_raster.h"
#include "idh_common.h"
#include "raster_common.h"

namespace {

struct WarpArgs {
    const float *depth;      // (M,h,w)
    const float *src_invK;   // (M,4,4)
    const float *cam_T_src;  // (B,M,4,4)
    const float *K;          // (B,4,4)
    unsigned long long *keys;  // (B,H,W)
    unsigned *queue;         // (B,M,F)
    unsigned *qcount;        // (B,M)
    float tear_ratio;
    int M, h, w, F, H, W;
};

struct SrcK {
    float k[9];  // rows of invK[:3,:3]
};

__device__ __forceinline__ SrcK load_src(const float *invK) {
    SrcK s;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) s.k[r * 3 + c] = invK[r * 4 + c];
    return s;
}

// vertex (i, j) of a source in the target camera: depth * invK (j + 0.5, i + 0.5, 1), then cam_T_src
__device__ __forceinline__ V3 warp_vertex(const Cam &c, const SrcK &s, int i, int j, float d) {
    const float u = (float)j + 0.5f, v = (float)i + 0.5f;
    const float p[3] = {d * (s.k[0] * u + s.k[1] * v + s.k[2]), d * (s.k[3] * u + s.k[4] * v + s.k[5]), d * (s.k[6] * u + s.k[7] * v + s.k[8])};
    return to_camera(c, p);
}

// screen position; only read for faces wholly at z > 0 (a denormal z may give +-inf: the box is clamped to the image)
__device__ __forceinline__ float2 warp_screen(const Cam &c, V3 p) { return make_float2(c.fx * (p.x / p.z) + c.cx, c.fy * (p.y / p.z) + c.cy); }

__device__ __forceinline__ bool valid_depth(float d) { return d > 0.f && d < INFINITY; }  // false for NaN

__global__ __launch_bounds__(256) void warp_fill_k(unsigned long long *__restrict__ keys, long long n, unsigned *__restrict__ qcount, int BM) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i < n) keys[i] = kEmptyKey;
    if (i < BM) qcount[i] = 0u;
}

// Face f of source m in target b.  false: the face draws nothing (an invalid corner, a tear, or one of raster_common.h's culls).
__device__ __forceinline__ bool warp_tri(const WarpArgs &a, int m, const Cam &c, const SrcK &s, unsigned f, Tri &t) {
    const int w = a.w, w1 = w - 1;
    const int q = (int)(f >> 1), i = q / w1, j = q - i * w1;
    const int up = (int)(f & 1u);
    // (row, column) of the three corners: even (v00, v10, v01), odd (v01, v10, v11)
    const int ra = i, ca = j + up, rb = i + 1, cb = j, rc = i + up, cc = j + 1;
    const int ia = ra * w + ca, ib = rb * w + cb, ic = rc * w + cc;
    const float *depth = a.depth + (size_t)m * a.h * w;
    const float da = depth[ia], db = depth[ib], dc = depth[ic];
    if (!(valid_depth(da) && valid_depth(db) && valid_depth(dc))) return false;
    const float zmin = fminf(da, fminf(db, dc)), zmax = fmaxf(da, fmaxf(db, dc));
    if (!(zmax <= zmin * a.tear_ratio)) return false;  // a depth discontinuity: no surface is known between these taps
    const V3 A = warp_vertex(c, s, ra, ca, da), B = warp_vertex(c, s, rb, cb, db), C = warp_vertex(c, s, rc, cc, dc);
    if (!tri_setup_corners(A, ia, B, ib, C, ic, a.H, a.W, t)) return false;
    if (t.straddles) return true;
    return tri_setup_box(warp_screen(c, A), warp_screen(c, B), warp_screen(c, C), a.H, a.W, t);
}

__global__ __launch_bounds__(256) void warp_face_k(const WarpArgs a) {
    const int bm = blockIdx.y, b = bm / a.M, m = bm - b * a.M;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= a.F) return;
    const Cam c = load_cam(a.cam_T_src + (size_t)bm * 16, a.K + b * 16);
    const SrcK s = load_src(a.src_invK + m * 16);
    Tri t;
    if (!warp_tri(a, m, c, s, (unsigned)f, t)) return;
    const int bw = t.x1 - t.x0 + 1, n = bw * (t.y1 - t.y0 + 1);
    if (t.straddles || n > kSmallBox) {
        const unsigned slot = atomicAdd(a.qcount + bm, 1u);  // < F: every face is appended at most once
        a.queue[(size_t)bm * a.F + slot] = (unsigned)f;
        return;
    }
    const KeySink zb = KeySink{a.keys}.camera((size_t)b * a.H * a.W);
    const unsigned id = (unsigned)m * (unsigned)a.F + (unsigned)f;  // M * F < 2^31: checked on the host
    for (int y = t.y0; y <= t.y1; ++y)
        for (int x = t.x0; x <= t.x1; ++x) shade(t, c, x, y, a.W, id, zb);
}

__global__ __launch_bounds__(256) void warp_large_k(const WarpArgs a) {
    const int bm = blockIdx.y, b = bm / a.M, m = bm - b * a.M;
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    const unsigned count = min(a.qcount[bm], (unsigned)a.F);
    if (count == 0) return;
    const Cam c = load_cam(a.cam_T_src + (size_t)bm * 16, a.K + b * 16);
    const SrcK s = load_src(a.src_invK + m * 16);
    const KeySink zb = KeySink{a.keys}.camera((size_t)b * a.H * a.W);
    for (unsigned q = wave; q < count; q += nwaves) {
        const unsigned f = a.queue[(size_t)bm * a.F + q];
        if (f >= (unsigned)a.F) continue;
        Tri t;
        if (!warp_tri(a, m, c, s, f, t)) continue;
        const unsigned id = (unsigned)m * (unsigned)a.F + f;
        const int tw = (t.x1 - t.x0) / kTile + 1, nt = tw * ((t.y1 - t.y0) / kTile + 1);
        for (int i = lane; i < nt; i += 64) {
            const int ty = i / tw;
            const int x0 = t.x0 + (i - ty * tw) * kTile, y0 = t.y0 + ty * kTile;
            const int x1 = min(x0 + kTile - 1, t.x1), y1 = min(y0 + kTile - 1, t.y1);
            if (tile_outside(t, c, x0, x1, y0, y1)) continue;
            for (int y = y0; y <= y1; ++y)
                for (int x = x0; x <= x1; ++x) shade(t, c, x, y, a.W, id, zb);
        }
    }
}

__global__ __launch_bounds__(256) void warp_resolve_k(const unsigned long long *__restrict__ keys, long long n, float empty_depth,
                                                      float *__restrict__ depth, int *__restrict__ source) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    const unsigned zbits = (unsigned)(key >> 32);
    const bool covered = zbits != kInfBits;
    depth[i] = covered ? __uint_as_float(zbits) : empty_depth;
    if (source) source[i] = covered ? (int)(unsigned)(key & 0xffffffffull) : -1;
}

struct WarpScratch {
    unsigned *queue, *qcount;
    unsigned long long *keys;
    size_t bytes;
};

// sizes are validated by the callers: all positive, h, w >= 2
WarpScratch warp_scratch(void *workspace, int B, int M, int h, int w, int H, int W) {
    const uintptr_t ws = reinterpret_cast<uintptr_t>(workspace);  // (also called with NULL, for the size alone)
    uintptr_t at = ws;
    const size_t bm = (size_t)B * (size_t)M, F = 2 * (size_t)(h - 1) * (size_t)(w - 1);
    WarpScratch s;
    s.queue = reinterpret_cast<unsigned *>(at);
    at += align256(bm * F * sizeof(unsigned));
    s.qcount = reinterpret_cast<unsigned *>(at);
    at += align256(bm * sizeof(unsigned));
    s.keys = reinterpret_cast<unsigned long long *>(at);
    at += align256((size_t)B * (size_t)H * (size_t)W * sizeof(unsigned long long));
    s.bytes = (size_t)(at - ws);
    return s;
}

bool warp_sizes_ok(int B, int M, int h, int w, int H, int W) { return B > 0 && M > 0 && h >= 2 && w >= 2 && H > 0 && W > 0; }

}  // namespace

extern "C" size_t idh_sizeof_depth_warp_args(void) { return sizeof(idh_depth_warp_args); }

extern "C" size_t idh_depth_warp_workspace_bytes(int B, int M, int h, int w, int H, int W) {
    if (!warp_sizes_ok(B, M, h, w, H, W)) return 0;
    return warp_scratch(nullptr, B, M, h, w, H, W).bytes;
}

extern "C" int idh_depth_warp_fwd(const idh_depth_warp_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_depth_warp_args)) return IDH_EINVAL;
    const idh_depth_warp_args &e = *args;
    const int B = e.B, M = e.M, h = e.h, w = e.w, H = e.H, W = e.W;
    if (!warp_sizes_ok(B, M, h, w, H, W)) return IDH_EINVAL;
    if (!(e.tear_ratio >= 1.f)) return IDH_EINVAL;  // also refuses NaN
    if (!e.depth_m1hw || !e.src_invK_m44 || !e.cam_T_src_bm44 || !e.K_b44 || !e.depth_b1hw) return IDH_EINVAL;
    const long long F = 2ll * (h - 1) * (w - 1);
    // the source id is an int32; one 32-bit grid of 256-lane workgroups fills / resolves the image; grid y holds B * M
    if ((long long)h * w >= (1ll << 30) || (long long)M * F >= (1ll << 31) || (long long)B * H * W >= (1ll << 31) || (long long)B * M > 65535)
        return IDH_EUNSUPPORTED;
    if (!e.workspace || e.workspace_bytes < 0 || (size_t)e.workspace_bytes < idh_depth_warp_workspace_bytes(B, M, h, w, H, W) ||
        ((uintptr_t)e.workspace & 255))
        return IDH_EWORKSPACE;
    hipStream_t st = idh_stream(stream);
    const WarpScratch s = warp_scratch(e.workspace, B, M, h, w, H, W);
    const WarpArgs a{e.depth_m1hw, e.src_invK_m44, e.cam_T_src_bm44, e.K_b44, s.keys, s.queue, s.qcount, e.tear_ratio,
                     M, h, w, (int)F, H, W};
    const long long n = (long long)B * H * W;
    const int BM = B * M;
    hipLaunchKernelGGL(warp_fill_k, dim3(idh_cdiv(n > BM ? n : BM, 256)), dim3(256), 0, st, s.keys, n, s.qcount, BM);
    IDH_CHECK_LAUNCH();
    hipLaunchKernelGGL(warp_face_k, dim3(idh_cdiv(F, 256), BM), dim3(256), 0, st, a);
    IDH_CHECK_LAUNCH();
    hipLaunchKernelGGL(warp_large_k, dim3(std::min(kLargeBlocks, idh_cdiv(F, 4)), BM), dim3(256), 0, st, a);
    IDH_CHECK_LAUNCH();
    hipLaunchKernelGGL(warp_resolve_k, dim3(idh_cdiv(n, 256)), dim3(256), 0, st, s.keys, n, e.empty_depth, e.depth_b1hw, e.source_bhw);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
