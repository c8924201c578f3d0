// Surface normals from depth (include/idh_geometry.h): the reference's NormalGenerator (utils/geometry_utils.py:92-138) in one launch.
//
//   depth_normals_k<K, FLAGS>   :121-138 dense: gaussian_blur2d (reflect), BackprojectDepth (:55-63), spatial_gradient (Sobel, replicate),
//                               cross, normalize; optionally orientation towards the camera, a rotation into world space and a validity map
//   patch_normals_k             :129-138 at the centre of given 3x3 patches of points (the hit test's form); no padding involved
//
// Both end in normal_of_patch(), so on equal points they give equal bits.  Built with -ffp-contract=off: every product and sum below is
// rounded on its own, in the order written.
//
// depth_normals_k: one workgroup of 256 lanes owns a 64 x 8 output tile (a wave stores 256 contiguous bytes per plane and row: whole 128-byte
// lines wherever the row itself is aligned).  With R = K / 2, in LDS:
//   raw  (8 + 2 + 2R) x (64 + 2 + 2R)   depth at the UNCLAMPED positions tile - 1 - R .. tile + R + 1, loaded through the reflect map
//   hb   (8 + 2 + 2R) x 66              horizontal blur of every raw row
//   pts  3 x 10 x 66                    back-projected smoothed points of tile - 1 .. tile + 1
// (ok / hok / pok: the same three stages of "flags == need", as bytes, when FLAGS.)  The border rule: spatial_gradient pads the SMOOTHED image
// with `replicate`, and the blur pads the DEPTH with `reflect`; the halo of the smoothed map is therefore the smoothed border pixel, not the
// blur of a padded depth.  Here the stages are indexed by unclamped image position (reflect is applied where the depth is read, so a stage
// entry at an in-image position is exactly the library's value there), entries at positions outside the image are never read, and the final
// 3x3 gather clamps its positions into the image: that clamp is the replicate padding.
// Per pixel 4 B in and 12 B out (+ 1 B + 1 B with flags); halo re-reads hit L2.  No atomics, no scratch, no inline assembly.
#include "idh_common.h"

#include "../../include/idh_geometry.h"

#include <math.h>

namespace {

constexpr int kTW = 64, kTH = 8, kPW = kTW + 2, kPH = kTH + 2;

// Steps 3-4 for one 3x3 patch p[row * 3 + col][component] (+ the orientation rule): Sobel cross-correlation with all nine taps in row-major
// order (the zero taps are multiplied too: 0 * NaN = NaN, as the convolution the reference runs), cross product, F.normalize, and - with
// `orient` - negation where the normal points along `view` (from the camera to the surface).
__device__ __forceinline__ void normal_of_patch(const float (&p)[9][3], const float (&view)[3], bool orient, float (&n)[3]) {
    const float wx[9] = {-0.125f, 0.f, 0.125f, -0.25f, 0.f, 0.25f, -0.125f, 0.f, 0.125f};
    const float wy[9] = {-0.125f, -0.25f, -0.125f, 0.f, 0.f, 0.f, 0.125f, 0.25f, 0.125f};
    float gx[3], gy[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float ax = wx[0] * p[0][c], ay = wy[0] * p[0][c];
#pragma unroll
        for (int t = 1; t < 9; ++t) {
            ax = ax + wx[t] * p[t][c];
            ay = ay + wy[t] * p[t][c];
        }
        gx[c] = ax, gy[c] = ay;
    }
    n[0] = gx[1] * gy[2] - gx[2] * gy[1];  // torch.cross(gx, gy)
    n[1] = gx[2] * gy[0] - gx[0] * gy[2];
    n[2] = gx[0] * gy[1] - gx[1] * gy[0];
    const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const float den = len < 1e-12f ? 1e-12f : len;  // clamp_min(eps): a NaN norm stays NaN (fmaxf would drop it)
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = n[c] / den;
    if (orient) {
        const float d = (n[0] * view[0] + n[1] * view[1]) + n[2] * view[2];
        if (d > 0.f) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
    }
}

struct NormArgs {
    const float *depth;
    const float *invK;
    const float *rot;
    const unsigned char *flags;
    float *out;
    unsigned char *valid;
    float g[7];
    int H, W, tiles_x, tiles_y, orient, need;
};

__device__ __forceinline__ int reflect_clamped(int i, int n) {  // `reflect` for i in [-(n-1), 2(n-1)]; positions further out are never used
    i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
    return min(max(i, 0), n - 1);
}

template <int K, bool FLAGS>
__global__ __launch_bounds__(256) void depth_normals_k(const NormArgs a) {
    constexpr int R = K / 2, RH = kPH + 2 * R, RW = kPW + 2 * R;
    __shared__ float raw[RH][RW];
    __shared__ float hb[K > 1 ? RH : 1][kPW];
    __shared__ float pts[3][kPH][kPW];
    __shared__ unsigned char ok[FLAGS ? RH : 1][RW], hok[FLAGS && K > 1 ? RH : 1][kPW], pok[FLAGS ? kPH : 1][kPW];

    const int tid = threadIdx.x;
    unsigned t = blockIdx.x;
    const int tx = (int)(t % (unsigned)a.tiles_x);
    t /= (unsigned)a.tiles_x;
    const int ty = (int)(t % (unsigned)a.tiles_y), b = (int)(t / (unsigned)a.tiles_y);
    const int H = a.H, W = a.W, x0 = tx * kTW, y0 = ty * kTH;
    const size_t plane = (size_t)H * W;
    const float *depth = a.depth + (size_t)b * plane;

    for (int i = tid; i < RH * RW; i += 256) {
        const int r = i / RW, c = i - r * RW;
        const size_t src = (size_t)reflect_clamped(y0 - 1 - R + r, H) * W + reflect_clamped(x0 - 1 - R + c, W);
        raw[r][c] = depth[src];
        if constexpr (FLAGS) ok[r][c] = a.flags[(size_t)b * plane + src] == (unsigned char)a.need;
    }
    __syncthreads();
    if constexpr (K > 1) {  // the horizontal pass first, as the library's separable filter
        for (int i = tid; i < RH * kPW; i += 256) {
            const int r = i / kPW, c = i - r * kPW;
            float acc = a.g[0] * raw[r][c];
            unsigned char v = 1;
            if constexpr (FLAGS) v = ok[r][c];
#pragma unroll
            for (int j = 1; j < K; ++j) {
                acc = acc + a.g[j] * raw[r][c + j];
                if constexpr (FLAGS) v &= ok[r][c + j];
            }
            hb[r][c] = acc;
            if constexpr (FLAGS) hok[r][c] = v;
        }
        __syncthreads();
    }
    const float *ik = a.invK + (size_t)b * 16;  // the same for every lane of the workgroup
    const float k00 = ik[0], k01 = ik[1], k02 = ik[2], k10 = ik[4], k11 = ik[5], k12 = ik[6], k20 = ik[8], k21 = ik[9], k22 = ik[10];
    for (int i = tid; i < kPH * kPW; i += 256) {
        const int r = i / kPW, c = i - r * kPW;
        float d;
        unsigned char v = 1;
        if constexpr (K > 1) {
            d = a.g[0] * hb[r][c];
            if constexpr (FLAGS) v = hok[r][c];
#pragma unroll
            for (int j = 1; j < K; ++j) {
                d = d + a.g[j] * hb[r + j][c];
                if constexpr (FLAGS) v &= hok[r + j][c];
            }
        } else {
            d = raw[r][c];  // k = 1: the identity, no arithmetic
            if constexpr (FLAGS) v = ok[r][c];
        }
        const float px = (float)(x0 - 1 + c) + 0.5f, py = (float)(y0 - 1 + r) + 0.5f;  // (:60-61)
        pts[0][r][c] = d * ((k00 * px + k01 * py) + k02);
        pts[1][r][c] = d * ((k10 * px + k11 * py) + k12);
        pts[2][r][c] = d * ((k20 * px + k21 * py) + k22);
        if constexpr (FLAGS) pok[r][c] = v;
    }
    __syncthreads();

    const int lx = tid & 63, x = x0 + lx;
    if (x >= W) return;
    int cs[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) cs[dx] = min(max(x + dx - 1, 0), W - 1) - (x0 - 1);  // replicate padding of the smoothed points
    float m[9] = {};
    if (a.rot)
        for (int i = 0; i < 9; ++i) m[i] = a.rot[(size_t)b * 9 + i];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int y = y0 + (tid >> 6) + 4 * h;
        if (y >= H) break;
        float p[9][3];
        bool v = true;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int r = min(max(y + dy - 1, 0), H - 1) - (y0 - 1);
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
#pragma unroll
                for (int c = 0; c < 3; ++c) p[dy * 3 + dx][c] = pts[c][r][cs[dx]];
                if constexpr (FLAGS) v = v && pok[r][cs[dx]];
            }
        }
        float n[3];
        normal_of_patch(p, p[4], a.orient != 0, n);
        if (a.rot) {
            const float n0 = n[0], n1 = n[1], n2 = n[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) n[c] = (m[3 * c] * n0 + m[3 * c + 1] * n1) + m[3 * c + 2] * n2;
        }
        const size_t o = (size_t)y * W + x;
        if constexpr (FLAGS) {
            if (!v) n[0] = n[1] = n[2] = 0.f;
            a.valid[(size_t)b * plane + o] = v ? 1 : 0;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out[((size_t)b * 3 + c) * plane + o] = n[c];
    }
}

struct PatchArgs {
    const float *points;
    const float *centre;
    const unsigned char *flags;
    float *out;
    unsigned char *valid;
    unsigned total, N;
    int orient, need;
};

__global__ __launch_bounds__(256) void patch_normals_k(const PatchArgs a) {
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= a.total) return;
    const float *src = a.points + (size_t)q * 27;
    float p[9][3];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 3; ++c) p[t][c] = src[t * 3 + c];
    float view[3] = {0.f, 0.f, 0.f};
    if (a.orient) {
        const float *cc = a.centre + (size_t)(q / a.N) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) view[c] = p[4][c] - cc[c];
    }
    float n[3];
    normal_of_patch(p, view, a.orient != 0, n);
    if (a.flags) {
        bool v = true;
#pragma unroll
        for (int t = 0; t < 9; ++t) v = v && a.flags[(size_t)q * 9 + t] == (unsigned char)a.need;
        if (!v) n[0] = n[1] = n[2] = 0.f;
        a.valid[q] = v ? 1 : 0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out[(size_t)q * 3 + c] = n[c];
}

template <int K>
void launch_dense(bool flags, unsigned blocks, hipStream_t st, const NormArgs &a) {
    if (flags)
        hipLaunchKernelGGL((depth_normals_k<K, true>), dim3(blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((depth_normals_k<K, false>), dim3(blocks), dim3(256), 0, st, a);
}

}  // namespace

extern "C" size_t idh_sizeof_normals_args(void) { return sizeof(idh_normals_args); }
extern "C" size_t idh_sizeof_patch_normals_args(void) { return sizeof(idh_patch_normals_args); }

extern "C" int idh_depth_normals_fwd(const idh_normals_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_normals_args)) return IDH_EINVAL;
    const idh_normals_args &e = *args;
    if (!e.depth_b1hw || !e.invK_b44 || !e.normals_b3hw) return IDH_EINVAL;
    const int k = e.kernel_size;
    if (k != 1 && k != 3 && k != 5 && k != 7) return IDH_EINVAL;
    if (!(e.smoothing_std > 0.f)) return IDH_EINVAL;
    if (e.B < 0 || e.H <= k / 2 || e.W <= k / 2) return IDH_EINVAL;  // reflect padding needs more than k / 2 pixels
    if (e.flags_b1hw && !e.valid_b1hw) return IDH_EINVAL;
    const long long lim = 1ll << 31;
    const long long tiles_x = idh_cdiv(e.W, kTW), tiles_y = idh_cdiv(e.H, kTH);
    if ((long long)e.H * e.W >= lim || tiles_x * tiles_y * e.B >= lim) return IDH_EUNSUPPORTED;
    if (e.B == 0) return IDH_OK;
    NormArgs a{};
    a.depth = e.depth_b1hw, a.invK = e.invK_b44, a.rot = e.world_R_cam_b33, a.flags = e.flags_b1hw, a.out = e.normals_b3hw;
    a.valid = e.valid_b1hw;
    // kornia.filters.get_gaussian_kernel1d: exp(-x^2 / (2 s^2)) / sum, in fp32
    const float den = 2.f * e.smoothing_std * e.smoothing_std;
    float sum = 0.f;
    for (int i = 0; i < k; ++i) {
        const float x = (float)(i - k / 2);
        a.g[i] = expf(-(x * x) / den);
        sum += a.g[i];
    }
    for (int i = 0; i < k; ++i) a.g[i] /= sum;
    a.H = e.H, a.W = e.W, a.tiles_x = (int)tiles_x, a.tiles_y = (int)tiles_y, a.orient = e.orient != 0, a.need = e.need;
    const unsigned blocks = (unsigned)(tiles_x * tiles_y * e.B);
    hipStream_t st = idh_stream(stream);
    const bool flags = a.flags != nullptr;
    switch (k) {
        case 1: launch_dense<1>(flags, blocks, st, a); break;
        case 3: launch_dense<3>(flags, blocks, st, a); break;
        case 5: launch_dense<5>(flags, blocks, st, a); break;
        default: launch_dense<7>(flags, blocks, st, a);
    }
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_patch_normals_fwd(const idh_patch_normals_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_patch_normals_args)) return IDH_EINVAL;
    const idh_patch_normals_args &e = *args;
    if (!e.points_bn93 || !e.normals_bn3) return IDH_EINVAL;
    if (e.B < 0 || e.N < 0) return IDH_EINVAL;
    if (e.flags_bn9 && !e.valid_bn) return IDH_EINVAL;
    if (e.orient && !e.cam_centre_b3) return IDH_EINVAL;
    if ((long long)e.B * e.N >= (1ll << 31)) return IDH_EUNSUPPORTED;
    if (e.B == 0 || e.N == 0) return IDH_OK;
    PatchArgs a{};
    a.points = e.points_bn93, a.centre = e.cam_centre_b3, a.flags = e.flags_bn9, a.out = e.normals_bn3, a.valid = e.valid_bn;
    a.total = (unsigned)e.B * (unsigned)e.N, a.N = (unsigned)e.N, a.orient = e.orient != 0, a.need = e.need;
    hipLaunchKernelGGL(patch_normals_k, dim3(idh_cdiv(a.total, 256)), dim3(256), 0, idh_stream(stream), a);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
