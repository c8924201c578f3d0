// Shaded mesh render (include/idh_raster.h): depth, the winning face, barycentrics, interpolated per-vertex attributes
// and lit RGBA of a mesh in B cameras.  The asset's depth and colour in a live camera, which the reference reads from files rendered
// off line (inference/inference.py:117, inference/composite.py).
//
//   raster_vertex_k / raster_face_k / raster_large_k   the passes of raster_common.h with the key sink below: the geometry, the culls
//                                                      and the fp32 expressions of the depth-only path (raster.hip), unchanged.
//   shaded_fill_k      the key plane to "empty", the queue counters to 0.
//   shaded_resolve_k   deferred shading, one lane per pixel: triangle setup of the winning face alone, barycentrics from the edge
//                      functions of the coverage test, then whichever outputs were requested.
//
// Key: (float_bits(z) << 32) | face, resolved by KeySink (raster_common.h): the nearest hit wins, the lowest face index among equal
// depths, whatever the order of arrival.  Nothing per-face is kept in memory: the shade pass recomputes what it needs from the
// transformed-vertex buffers of the vertex pass, which are still in the workspace.
#include <math.h>

#include <algorithm>

#include "../../include/idh_raster.h"
#include "idh_common.h"
#include "raster_common.h"

namespace {

constexpr int kMaxAttrs = 16;

__global__ __launch_bounds__(256) void shaded_fill_k(unsigned long long *__restrict__ keys, long long n, unsigned *__restrict__ qcount, int B) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i < n) keys[i] = kEmptyKey;
    if (i < B) qcount[i] = 0u;
}

struct ShadeArgs {
    const unsigned long long *keys;  // (B,H,W)
    const float4 *cam;               // (B,V)
    const float2 *scr;               // (B,V)
    const int *faces;                // (F,3)
    const float *cam_T_world, *K;
    const unsigned char *colors;  // (V,4) or NULL
    const float *attrs;           // (V,C) or NULL
    float *depth;                 // each output may be NULL
    int *pix_to_face;
    float *bary;
    float *attr_out;
    unsigned char *rgba;
    float ambient, empty_depth;
    int V, F, B, H, W, C;
};

__device__ __forceinline__ unsigned char to_u8(float v) { return (unsigned char)(fminf(fmaxf(v, 0.f), 255.f) + 0.5f); }

__global__ __launch_bounds__(256) void shaded_resolve_k(const ShadeArgs a) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    const long long hw = (long long)a.H * a.W;
    if (i >= (long long)a.B * hw) return;
    const int b = (int)(i / hw);
    const int pix = (int)(i - (long long)b * hw);
    const int y = pix / a.W, x = pix - y * a.W;
    const unsigned long long key = a.keys[i];
    const unsigned zbits = (unsigned)(key >> 32), f = (unsigned)(key & 0xffffffffull);
    Tri t;
    // an empty pixel; a face word outside [0, F) or a face that no longer sets up cannot come out of the face passes: drawn as empty
    const bool covered = zbits != kInfBits && f < (unsigned)a.F &&
                         tri_setup(a.cam + (size_t)b * a.V, a.scr + (size_t)b * a.V, a.faces + (size_t)f * 3, a.V, a.H, a.W, t);
    if (!covered) {
        if (a.depth) a.depth[i] = a.empty_depth;
        if (a.pix_to_face) a.pix_to_face[i] = -1;
        if (a.bary) a.bary[i * 3] = 0.f, a.bary[i * 3 + 1] = 0.f, a.bary[i * 3 + 2] = 0.f;
        if (a.attr_out)
            for (int c = 0; c < a.C; ++c) a.attr_out[i * a.C + c] = 0.f;
        if (a.rgba) *reinterpret_cast<uchar4 *>(a.rgba + i * 4) = make_uchar4(0, 0, 0, 0);
        return;
    }
    if (a.depth) a.depth[i] = __uint_as_float(zbits);
    if (a.pix_to_face) a.pix_to_face[i] = (int)f;
    if (!a.bary && !a.attr_out && !a.rgba) return;
    const Cam c = load_cam(a.cam_T_world + b * 16, a.K + b * 16);
    const V3 d = pixel_ray(c, x, y);
    const float e0 = dot(d, t.n0), e1 = dot(d, t.n1), e2 = dot(d, t.n2);
    const float s = e0 + e1 + e2;
    float w0 = 1.f / 3.f, w1 = 1.f / 3.f, w2 = 1.f / 3.f;
    if (s > 0.f) w0 = e0 / s, w1 = e1 / s, w2 = e2 / s;
    if (a.bary) a.bary[i * 3] = w0, a.bary[i * 3 + 1] = w1, a.bary[i * 3 + 2] = w2;
    const int *face = a.faces + (size_t)f * 3;
    const int ia = face[0], ib = face[1], ic = face[2];  // inside [0, V): tri_setup checked
    if (a.attr_out) {
        const float *pa = a.attrs + (size_t)ia * a.C, *pb = a.attrs + (size_t)ib * a.C, *pc = a.attrs + (size_t)ic * a.C;
        for (int ch = 0; ch < a.C; ++ch) a.attr_out[i * a.C + ch] = w0 * pa[ch] + w1 * pb[ch] + w2 * pc[ch];
    }
    if (a.rgba) {
        const uchar4 ca = *reinterpret_cast<const uchar4 *>(a.colors + (size_t)ia * 4), cb = *reinterpret_cast<const uchar4 *>(a.colors + (size_t)ib * 4),
                     cc = *reinterpret_cast<const uchar4 *>(a.colors + (size_t)ic * 4);
        const float lam = dot(d, t.N) / sqrtf(dot(t.N, t.N) * dot(d, d));
        const float light = a.ambient + (1.f - a.ambient) * lam;
        const float r = (w0 * (float)ca.x + w1 * (float)cb.x + w2 * (float)cc.x) * light;
        const float g = (w0 * (float)ca.y + w1 * (float)cb.y + w2 * (float)cc.y) * light;
        const float bl = (w0 * (float)ca.z + w1 * (float)cb.z + w2 * (float)cc.z) * light;
        const float al = w0 * (float)ca.w + w1 * (float)cb.w + w2 * (float)cc.w;
        *reinterpret_cast<uchar4 *>(a.rgba + i * 4) = make_uchar4(to_u8(r), to_u8(g), to_u8(bl), to_u8(al));
    }
}

}  // namespace

extern "C" size_t idh_sizeof_raster_shaded_args(void) { return sizeof(idh_raster_shaded_args); }

extern "C" size_t idh_raster_shaded_workspace_bytes(int B, int V, int F, int H, int W) {
    if (B < 0 || V < 0 || F < 0 || H <= 0 || W <= 0) return 0;
    return raster_scratch_bytes(B, V, F) + align256((size_t)B * (size_t)H * (size_t)W * sizeof(unsigned long long)) + 256;
}

extern "C" int idh_raster_shaded_fwd(const idh_raster_shaded_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_raster_shaded_args)) return IDH_EINVAL;
    const idh_raster_shaded_args &e = *args;
    const int B = e.B, V = e.V, F = e.F, H = e.H, W = e.W, C = e.C;
    if (B < 0 || V < 0 || F < 0 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31)) return IDH_EINVAL;
    if (C < 0 || C > kMaxAttrs || (e.attrs_vc && C == 0)) return IDH_EINVAL;
    if (!(e.ambient >= 0.f && e.ambient <= 1.f)) return IDH_EINVAL;  // also refuses NaN
    if (B == 0) return IDH_OK;
    if ((long long)B * H * W >= (1ll << 31)) return IDH_EUNSUPPORTED;  // one 32-bit grid of 256-lane workgroups fills / shades the image
    if (!e.cam_T_world_b44 || !e.K_b44 || (V > 0 && !e.verts_v3) || (F > 0 && !e.faces_f3)) return IDH_EINVAL;
    if (!e.depth_b1hw && !e.pix_to_face_bhw && !e.bary_bhw3 && !e.attr_out_bhwc && !e.rgba_bhw4) return IDH_EINVAL;
    if ((e.attr_out_bhwc && !e.attrs_vc) || (e.rgba_bhw4 && !e.colors_v4)) return IDH_EINVAL;
    if (!e.workspace || e.workspace_bytes < 0 || (size_t)e.workspace_bytes < idh_raster_shaded_workspace_bytes(B, V, F, H, W) ||
        ((uintptr_t)e.workspace & 255))
        return IDH_EWORKSPACE;
    if (B > 65535) return IDH_EUNSUPPORTED;
    hipStream_t st = idh_stream(stream);
    const RasterScratch w = raster_scratch(e.workspace, B, V, F);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(w.end);  // 256-byte aligned
    const long long n = (long long)B * H * W;
    hipLaunchKernelGGL(shaded_fill_k, dim3(idh_cdiv(n, 256)), dim3(256), 0, st, keys, n, w.qcount, B);  // n >= B: H, W >= 1
    IDH_CHECK_LAUNCH();
    if (V > 0 && F > 0) {
        hipLaunchKernelGGL(raster_vertex_k, dim3(idh_cdiv(V, 256), B), dim3(256), 0, st, e.verts_v3, V, e.cam_T_world_b44, e.K_b44, w.cam, w.scr);
        IDH_CHECK_LAUNCH();
        const RasterArgs<KeySink> a{w.cam, w.scr, e.faces_f3, e.cam_T_world_b44, e.K_b44, V, F, H, W, KeySink{keys}, w.queue, w.qcount};
        hipLaunchKernelGGL(raster_face_k<KeySink>, dim3(idh_cdiv(F, 256), B), dim3(256), 0, st, a);
        IDH_CHECK_LAUNCH();
        hipLaunchKernelGGL(raster_large_k<KeySink>, dim3(std::min(kLargeBlocks, idh_cdiv(F, 4)), B), dim3(256), 0, st, a);
        IDH_CHECK_LAUNCH();
    }
    // F == 0 or V == 0: every key is empty, and the shade pass reads neither the faces nor the vertex buffers
    const ShadeArgs s{keys, w.cam, w.scr, e.faces_f3, e.cam_T_world_b44, e.K_b44, e.colors_v4, e.attrs_vc, e.depth_b1hw, e.pix_to_face_bhw,
                      e.bary_bhw3, e.attr_out_bhwc, e.rgba_bhw4, e.ambient, e.empty_depth, V, (V > 0 ? F : 0), B, H, W, C};
    hipLaunchKernelGGL(shaded_resolve_k, dim3(idh_cdiv(n, 256)), dim3(256), 0, st, s);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
