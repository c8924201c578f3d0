// What the entry points of the mesh rasteriser share (raster.hip: depth only; raster_shade.hip: depth + winning face, then a
// deferred shade pass; depth_warp.hip: depth maps drawn as implicit meshes, with its own passes over the device functions here): the camera, the per-triangle setup, the edge tests and the two-level face pass.  The passes are templates over
// a per-pixel SINK, the one place where the two differ: what a hit (pixel, z, face) does to the z-buffer.
//
//   raster_vertex_k   world -> camera -> screen, once per vertex and camera.
//   raster_face_k     one lane per face: culls (index out of range, non-finite, wholly at z <= 0, zero area, bounding box off screen) and
//                     resolves a face whose box holds at most kSmallBox pixel centres in place; larger and z = 0-straddling faces go
//                     to a queue.
//   raster_large_k    one wave per queued face, its 64 lanes striding over the 8 x 8-pixel tiles of the face's box (the whole image for a
//                     straddling face); a tile wholly outside one edge is skipped.
//
// The ray test runs in camera space (no projection of the triangle, hence no clipping): with camera-space corners A, B, C and pixel ray
// d = ((u - cx) / fx, (v - cy) / fy, 1), the ray meets the triangle's plane at z = N.A / N.d, N = (B - A) x (C - A), inside when
// d.(B x C), d.(C x A), d.(A x B) all carry the sign of N.A.  P x Q is computed as L x (H - L) from the lower-numbered corner L of the
// edge (negated when that swaps the operands): the difference keeps full precision for the small far triangles whose P and Q are nearly
// parallel, and the two triangles of a shared edge get exactly negated normals.  Built with -ffp-contract=off.
//
// Everything sits in an anonymous namespace: each source that includes it gets its own copy, as every other kernel file of the library does.
#ifndef IDH_RASTER_COMMON_H_
#define IDH_RASTER_COMMON_H_

#include <math.h>

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

// the ray of pixel (row y, col x)
__device__ __forceinline__ V3 pixel_ray(const Cam &c, int x, int y) { return {((float)x + 0.5f - c.cx) / c.fx, ((float)y + 0.5f - c.cy) / c.fy, 1.f}; }

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

// The two halves of a triangle's setup, for callers that hold the corners in registers (depth_warp.hip: the faces of a depth map are
// implicit).  tri_setup_corners: camera-space corners A, B, C with vertex numbers ia, ib, ic (they only order the shared edges); false:
// the face draws nothing; a face that straddles z = 0 leaves with the whole image as its box.  tri_setup_box: the box of a face wholly
// in front of the camera from its corners' screen positions; false: no pixel centre inside.
__device__ __forceinline__ bool tri_setup_corners(V3 A, int ia, V3 B, int ib, V3 C, int ic, int H, int W, Tri &t) {
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
    if (t.straddles) t.x0 = 0, t.x1 = W - 1, t.y0 = 0, t.y1 = H - 1;  // its projection is not the triangle of its projected corners: test the whole image
    return true;
}

__device__ __forceinline__ bool tri_setup_box(float2 pa, float2 pb, float2 pc, int H, int W, Tri &t) {
    const float u0 = fminf(pa.x, fminf(pb.x, pc.x)), u1 = fmaxf(pa.x, fmaxf(pb.x, pc.x));
    const float v0 = fminf(pa.y, fminf(pb.y, pc.y)), v1 = fmaxf(pa.y, fmaxf(pb.y, pc.y));
    // pixel centres j + 0.5 inside [u0 - pad, u1 + pad], clamped to the image in float (the ends may be infinite)
    t.x0 = (int)fminf(fmaxf(ceilf(u0 - 0.5f - kBoxPad), 0.f), (float)W);
    t.x1 = (int)fmaxf(fminf(floorf(u1 - 0.5f + kBoxPad), (float)(W - 1)), -1.f);
    t.y0 = (int)fminf(fmaxf(ceilf(v0 - 0.5f - kBoxPad), 0.f), (float)H);
    t.y1 = (int)fmaxf(fminf(floorf(v1 - 0.5f + kBoxPad), (float)(H - 1)), -1.f);
    return t.x1 >= t.x0 && t.y1 >= t.y0;
}

// false: the face draws nothing
__device__ __forceinline__ bool tri_setup(const float4 *__restrict__ cam, const float2 *__restrict__ scr, const int *__restrict__ face, int V,
                                          int H, int W, Tri &t) {
    const int ia = face[0], ib = face[1], ic = face[2];
    if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) return false;
    const float4 a4 = cam[ia], b4 = cam[ib], c4 = cam[ic];
    if (!tri_setup_corners(V3{a4.x, a4.y, a4.z}, ia, V3{b4.x, b4.y, b4.z}, ib, V3{c4.x, c4.y, c4.z}, ic, H, W, t)) return false;
    if (t.straddles) return true;
    return tri_setup_box(scr[ia], scr[ib], scr[ic], H, W, t);
}

// The ray test of one pixel.  A Sink is a small value type with
//   Sink camera(size_t first_pixel) const      the same sink moved to the plane of one camera
//   void hit(size_t pixel, float z, unsigned face) const
// `pixel` is y * W + x inside that plane and z > 0 is finite.
template <class Sink>
__device__ __forceinline__ void shade(const Tri &t, const Cam &c, int x, int y, int W, unsigned face, const Sink &sink) {
    const V3 d = pixel_ray(c, x, y);
    const float e0 = dot(d, t.n0), e1 = dot(d, t.n1), e2 = dot(d, t.n2);
    if (e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) {
        const float den = dot(d, t.N);
        const float z = t.k / den;
        if (den > 0.f && z > 0.f && z < INFINITY) sink.hit((size_t)y * W + x, z, face);
    }
}

// The z-buffer that also names the winner (raster_shade.hip, depth_warp.hip): key = (float_bits(z) << 32) | id.  z > 0, so the unsigned
// order of the upper word is the float order; the lower word breaks ties towards the lowest id.  One 64-bit atomicMin per hit
// (global_atomic_umin_x2 on gfx950, no compare-and-swap loop) picks the same winner whatever the order of arrival.
constexpr unsigned long long kEmptyKey = ((unsigned long long)kInfBits << 32) | 0xffffffffull;

struct KeySink {
    unsigned long long *keys;
    __device__ __forceinline__ KeySink camera(size_t first_pixel) const { return {keys + first_pixel}; }
    __device__ __forceinline__ void hit(size_t pixel, float z, unsigned face) const {
        atomicMin(keys + pixel, ((unsigned long long)__float_as_uint(z) << 32) | face);
    }
};

template <class Sink>
struct RasterArgs {
    const float4 *cam;  // (B,V)
    const float2 *scr;  // (B,V)
    const int *faces;   // (F,3)
    const float *cam_T_world, *K;
    int V, F, H, W;
    Sink sink;         // the z-buffer, (B,H,W)
    unsigned *queue;   // (B,F)
    unsigned *qcount;  // (B)
};

// ---- face pass ----------------------------------------------------------------------------------------------
template <class Sink>
__global__ __launch_bounds__(256) void raster_face_k(const RasterArgs<Sink> a) {
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
    const Sink zb = a.sink.camera((size_t)b * a.H * a.W);
    for (int y = t.y0; y <= t.y1; ++y)
        for (int x = t.x0; x <= t.x1; ++x) shade(t, c, x, y, a.W, (unsigned)f, zb);
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

template <class Sink>
__global__ __launch_bounds__(256) void raster_large_k(const RasterArgs<Sink> a) {
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    const unsigned count = min(a.qcount[b], (unsigned)a.F);
    const Cam c = load_cam(a.cam_T_world + b * 16, a.K + b * 16);
    const Sink zb = a.sink.camera((size_t)b * a.H * a.W);
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
                for (int x = x0; x <= x1; ++x) shade(t, c, x, y, a.W, f, zb);
        }
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// The vertex buffers, the queue of large faces and its counters: the head of both entry points' workspaces.
struct RasterScratch {
    float4 *cam;
    float2 *scr;
    unsigned *queue, *qcount;
    unsigned char *end;  // first byte after them, 256-byte aligned
};

inline size_t raster_scratch_bytes(int B, int V, int F) {
    const size_t bv = (size_t)B * (size_t)V;
    return align256(bv * sizeof(float4)) + align256(bv * sizeof(float2)) + align256((size_t)B * (size_t)F * sizeof(unsigned)) +
           align256((size_t)B * sizeof(unsigned));
}

inline RasterScratch raster_scratch(void *workspace, int B, int V, int F) {
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    const size_t bv = (size_t)B * (size_t)V;
    RasterScratch s;
    s.cam = reinterpret_cast<float4 *>(ws);
    ws += align256(bv * sizeof(float4));
    s.scr = reinterpret_cast<float2 *>(ws);
    ws += align256(bv * sizeof(float2));
    s.queue = reinterpret_cast<unsigned *>(ws);
    ws += align256((size_t)B * (size_t)F * sizeof(unsigned));
    s.qcount = reinterpret_cast<unsigned *>(ws);
    s.end = ws + align256((size_t)B * sizeof(unsigned));
    return s;
}

}  // namespace

#endif  // IDH_RASTER_COMMON_H_
