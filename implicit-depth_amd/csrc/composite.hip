// AR compositing (include/idh_composite.h): what the reference does on the CPU between the model's outputs and the frame it shows.
//
//   prep_rendered_depth_k   inference/inference.py:117-128: F.max_pool2d(x, 7, 1, 3) copied into the pixels that are exactly 0, then
//                           torchvision resize(NEAREST), evaluated per OUTPUT pixel: only h * w windows, no full-resolution temporary.
//   composite_k             inference/inference.py:159 (sigmoid_custom) and inference/composite.py:19-24, :75-143 in one pass over the
//                           camera image: resize of the map, get_mask, valid pixels, fade, blend, truncation to uint8.
//
// composite_k's dtypes follow numpy's, statement by statement (built with -ffp-contract=off: only the explicit fmaf of the resize fuse):
//   :82-84   rgba.astype(np.float32) / 255.0                      fp32 division                       rgb, alpha
//   :86-90   np.zeros((h, w, 3)) colour, np.ones valid            fp64 colour; valid = 1
//   :92-94   valid *= fade                                        fp32 product (render) / fp32(1.0 * fade) (constant colour, after :102's astype)
//   :101     cv2.resize(raw_matte, INTER_LINEAR)                  fp32, half-pixel centres, rounded as torch's CPU upsample_bilinear2d (linear_src, blend4)
//   :102     1.0 - matte * valid                                  fp32
//   :123-126 (virtual > 0).astype(np.float32) * fade              fp32
//   :128-129 get_mask(depth, virtual map); 1.0 - mask * valid     fp32: 5.0f * ((pred - virtual) + 0.1f), clipped / pred > virtual
//   :131-134 get_mask(depth, np.ones((h, w)) * plane); 1.0 - mask fp64 (the plane is float64), rounded to fp32 by :137
//   :76      im = u8 / 255.0                                      fp64
//   :138     matte * im + (1 - matte) * virtual_rgb               fp64 product + (fp32 product with a render | fp64 product with the colour), fp64 sum
//   :142     (composited * 255.0).astype(np.uint8)                fp64 product, truncation toward zero
//
// Shape: the kernel is bound by the image (3 B), render (4 B) and output (3 B) streams; the map is L2-resident.  The B * H * W pixels are
// taken as one flat run and every lane owns four consecutive ones: 12 image bytes in and 12 out as three dwords, 16 render bytes as one
// load, four matte floats as one store.  A group of four starts at byte 12 g, so it is dword-aligned whatever W is (141-byte rows included);
// a group may straddle a row or a frame, its pixels carry their own (b, y, x).  Only the last partial group, or every group when a base
// pointer is not aligned, goes through the per-pixel byte path.  Mode, render / colour and resize / copy are template parameters.
#include "idh_common.h"

#include "../../include/idh_composite.h"

namespace {

struct Lin {
    int i0, i1;  // taps (i1 = i0 or i0 + 1)
    float l0, l1;
};

// area_pixel_compute_source_index / guard_index_and_lambda of upsample_bilinear2d with align_corners = False, rounded as torch's CPU
// kernel rounds it (the replay of composite.py:101 / :118 that tests/golden/g16_composite.npz pins runs on the CPU): the source index is
// one FMA there.  eval_frame.hip keeps the unfused form, which is torch's GPU kernel; the two differ by an ulp of the index in a few
// rows / columns per image.
__device__ __forceinline__ Lin linear_src(int dst, float scale, int in) {
    float src = fmaf(scale, (float)dst + 0.5f, -0.5f);
    if (src < 0.f) src = 0.f;
    Lin r;
    r.i0 = min((int)floorf(src), in - 1);
    r.l1 = fminf(fmaxf(src - (float)r.i0, 0.f), 1.f);
    r.l0 = 1.f - r.l1;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    return r;
}

// The four-tap blend, again as torch's CPU kernel rounds it.  torch has two CPU kernels for a contiguous one-channel map and picks by the
// OUTPUT size: H + W <= 128 takes its vectorised kernel (`small`: the four products of the weights, v01 first and the other three taps
// accumulated by FMA), anything larger its generic one (row-wise, fma(ly0, top, ly1 * bot) with top / bot = fma(lx0, v0, lx1 * v1)).  The
// rule is torch's dispatch condition, confirmed against F.interpolate on shapes either side of it (tests/test_composite_cpu.py); camera
// frames are always on the row-wise side.  The host decides once per launch (CompArgs::small).
__device__ __forceinline__ float blend4(const Lin &ly, const Lin &lx, float v00, float v01, float v10, float v11, bool small) {
    if (small) {
        float acc = (ly.l0 * lx.l1) * v01;
        acc = fmaf(ly.l0 * lx.l0, v00, acc);
        acc = fmaf(ly.l1 * lx.l0, v10, acc);
        return fmaf(ly.l1 * lx.l1, v11, acc);
    }
    const float top = fmaf(lx.l0, v00, lx.l1 * v01), bot = fmaf(lx.l0, v10, lx.l1 * v11);
    return fmaf(ly.l0, top, ly.l1 * bot);
}

__device__ __forceinline__ int nearest_src(int dst, float scale, int in) { return min((int)floorf((float)dst * scale), in - 1); }

// ---- asset depth preparation --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_rendered_depth_k(const float *__restrict__ in, int Hr, int Wr, int h, int w, float sy, float sx,
                                                             float *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= h * w) return;
    const int b = blockIdx.y;
    const int oy = i / w, ox = i - oy * w;
    const int y = nearest_src(oy, sy, Hr), x = nearest_src(ox, sx, Wr);
    const float *p = in + (size_t)b * Hr * Wr;
    float v = p[(size_t)y * Wr + x];
    if (v == 0.f) {  // (:121): only the pixels that are exactly 0 take the pooled value
        const int y0 = max(y - 3, 0), y1 = min(y + 3, Hr - 1), x0 = max(x - 3, 0), x1 = min(x + 3, Wr - 1);
        for (int yy = y0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) {
                const float t = p[(size_t)yy * Wr + xx];
                if (t > v || t != t) v = t;  // max_pool2d propagates NaN
            }
    }
    out[(size_t)b * h * w + i] = v;
}

// ---- compositing ----------------------------------------------------------------------------------------------------
struct CompArgs {
    const unsigned char *image;  // (B,H,W,3)
    const unsigned char *rgba;   // (B,H,W,4) or null
    const float *map;            // (B,1,h,w)
    const float *vdepth;         // (B,H,W) or null
    const float *fade;           // (B) or null
    unsigned char *out;          // (B,H,W,3)
    float *matte_out;            // (B,H,W) or null
    double plane;
    double colour[3];
    float mult, sy, sx;
    int h, w, H, W;
    unsigned HW, N;  // H * W, B * H * W
    int bgr, vec;    // vec: every pointer is aligned for the dword / 16-byte path
    int small;       // H + W <= 128: the rounding form of blend4
};

struct alignas(4) U3 {
    unsigned a, b, c;
};

enum Src { kLogits = 0, kProb = 1, kDepthSoftMap = 2, kDepthHardMap = 3, kDepthSoftPlane = 4, kDepthHardPlane = 5 };

__device__ __forceinline__ float sigmoid_custom(float x, float m) { return 1.f / (1.f + expf(-m * x)); }  // modules/layers.py:138-139

template <int SRC, bool RESIZE>
__device__ __forceinline__ float sample_map(const CompArgs &a, const float *__restrict__ m, int y, int x) {
    if (RESIZE) {
        const Lin ly = linear_src(y, a.sy, a.h), lx = linear_src(x, a.sx, a.w);
        float v00 = m[(size_t)ly.i0 * a.w + lx.i0], v01 = m[(size_t)ly.i0 * a.w + lx.i1];
        float v10 = m[(size_t)ly.i1 * a.w + lx.i0], v11 = m[(size_t)ly.i1 * a.w + lx.i1];
        if (SRC == kLogits) {  // the reference resizes the probabilities (inference.py:159, composite.py:101)
            v00 = sigmoid_custom(v00, a.mult), v01 = sigmoid_custom(v01, a.mult);
            v10 = sigmoid_custom(v10, a.mult), v11 = sigmoid_custom(v11, a.mult);
        }
        return blend4(ly, lx, v00, v01, v10, v11, a.small != 0);
    }
    const float v = m[(size_t)y * a.w + x];
    return SRC == kLogits ? sigmoid_custom(v, a.mult) : v;
}

__device__ __forceinline__ float clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }
__device__ __forceinline__ double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

__device__ __forceinline__ unsigned to_u8(double c) {  // .astype(np.uint8) of a value in [0, 255]: truncation; kept in range, NaN -> 0
    c = !(c >= 0.0) ? 0.0 : (c > 255.0 ? 255.0 : c);
    return (unsigned)(int)c;
}

template <int SRC, bool RGBA, bool RESIZE>
__global__ __launch_bounds__(256) void composite_k(const CompArgs a) {
    constexpr bool kMask = SRC == kLogits || SRC == kProb, kPlane = SRC == kDepthSoftPlane || SRC == kDepthHardPlane;
    constexpr bool kSoft = SRC == kDepthSoftMap || SRC == kDepthSoftPlane;
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    const unsigned p0 = g * 4u;
    if (p0 >= a.N) return;
    const int n = (int)min(4u, a.N - p0);
    const bool vec = a.vec && n == 4;

    alignas(16) unsigned char im[12], va[16];
    alignas(16) float vd[4];
    if (vec) {
        *reinterpret_cast<U3 *>(im) = *reinterpret_cast<const U3 *>(a.image + (size_t)p0 * 3);
        if (RGBA) *reinterpret_cast<uint4 *>(va) = *reinterpret_cast<const uint4 *>(a.rgba + (size_t)p0 * 4);
        if (!kMask && !kPlane) *reinterpret_cast<float4 *>(vd) = *reinterpret_cast<const float4 *>(a.vdepth + p0);
    } else {
        for (int k = 0; k < 4; ++k) {
            const size_t p = p0 + min(k, n - 1);  // past the end: the last pixel again (read only)
            for (int c = 0; c < 3; ++c) im[3 * k + c] = a.image[p * 3 + c];
            if (RGBA)
                for (int c = 0; c < 4; ++c) va[4 * k + c] = a.rgba[p * 4 + c];
            if (!kMask && !kPlane) vd[k] = a.vdepth[p];
        }
    }

    unsigned b = p0 / a.HW;
    const unsigned r = p0 - b * a.HW;
    int y = (int)(r / (unsigned)a.W), x = (int)(r - (unsigned)y * a.W);
    const size_t plane = (size_t)a.h * a.w;
    alignas(4) unsigned char o[12];
    float mt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float fade = a.fade ? a.fade[b] : 1.f;
        const float pv = sample_map<SRC, RESIZE>(a, a.map + b * plane, y, x);
        float rgb[3] = {0.f, 0.f, 0.f}, alpha = 1.f;
        if (RGBA) {
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c] = (float)va[4 * k + c] / 255.f;
            alpha = (float)va[4 * k + 3] / 255.f;
        }
        float matte;
        if (kMask) {
            matte = 1.f - pv * (alpha * fade);  // (:92-94, :102); constant colour: alpha = 1, fp32(1.0 * fade) = fade
        } else if (!kPlane) {
            const float valid = (vd[k] > 0.f ? 1.f : 0.f) * fade;  // (:123-126)
            const float mask = kSoft ? clip01(5.f * ((pv - vd[k]) + 0.1f)) : (pv > vd[k] ? 1.f : 0.f);
            matte = 1.f - mask * valid;  // (:129)
        } else if (kSoft) {
            matte = (float)(1.0 - clip01(5.0 * (((double)pv - a.plane) + 0.1)));  // (:131-134, :137)
        } else {
            matte = 1.f - ((double)pv > a.plane ? 1.f : 0.f);
        }
        mt[k] = matte;
        const float inv = 1.f - matte;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double imd = (double)im[3 * k + c] / 255.0;
            const double vir = RGBA ? (double)(inv * rgb[c]) : (double)inv * a.colour[c];
            const double comp = (double)matte * imd + vir;  // (:138)
            o[3 * k + (a.bgr ? 2 - c : c)] = (unsigned char)to_u8(comp * 255.0);
        }
        if (++x == a.W) {
            x = 0;
            if (++y == a.H) y = 0, ++b;
        }
        if (k + 1 >= n) b = min(b, (a.N - 1) / a.HW);  // a partial last group stays inside the last frame
    }

    if (vec) {
        *reinterpret_cast<U3 *>(a.out + (size_t)p0 * 3) = *reinterpret_cast<const U3 *>(o);
        if (a.matte_out) *reinterpret_cast<float4 *>(a.matte_out + p0) = make_float4(mt[0], mt[1], mt[2], mt[3]);
    } else {
        for (int k = 0; k < n; ++k) {
            for (int c = 0; c < 3; ++c) a.out[(size_t)(p0 + k) * 3 + c] = o[3 * k + c];
            if (a.matte_out) a.matte_out[p0 + k] = mt[k];
        }
    }
}

template <int SRC, bool RGBA>
void launch2(bool resize, dim3 grid, hipStream_t st, const CompArgs &a) {
    if (resize)
        hipLaunchKernelGGL((composite_k<SRC, RGBA, true>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((composite_k<SRC, RGBA, false>), grid, dim3(256), 0, st, a);
}

template <int SRC>
void launch1(bool rgba, bool resize, dim3 grid, hipStream_t st, const CompArgs &a) {
    if (rgba)
        launch2<SRC, true>(resize, grid, st, a);
    else
        launch2<SRC, false>(resize, grid, st, a);
}

bool aligned(const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace

extern "C" size_t idh_sizeof_composite_args(void) { return sizeof(idh_composite_args); }

extern "C" int idh_prep_rendered_depth_fwd(const float *rendered_b1HW, int B, int Hr, int Wr, int h, int w, float *out_b1hw, void *stream) {
    if (B < 0 || Hr <= 0 || Wr <= 0 || h <= 0 || w <= 0 || (long long)Hr * Wr >= (1ll << 31) || (long long)h * w >= (1ll << 31)) return IDH_EINVAL;
    if (!rendered_b1HW || !out_b1hw) return IDH_EINVAL;
    if (B > 65535) return IDH_EUNSUPPORTED;
    if (B == 0) return IDH_OK;
    hipLaunchKernelGGL(prep_rendered_depth_k, dim3(idh_cdiv((long long)h * w, 256), B), dim3(256), 0, idh_stream(stream), rendered_b1HW, Hr, Wr,
                       h, w, (float)Hr / h, (float)Wr / w, out_b1hw);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_composite_fwd(const idh_composite_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_composite_args)) return IDH_EINVAL;
    const idh_composite_args &e = *args;
    if (e.B < 0 || e.h <= 0 || e.w <= 0 || e.H <= 0 || e.W <= 0) return IDH_EINVAL;
    if (e.mode < IDH_COMPOSITE_MASK_LOGITS || e.mode > IDH_COMPOSITE_DEPTH_HARD) return IDH_EINVAL;
    if (!e.image_bHW3 || !e.map_b1hw || !e.out_bHW3) return IDH_EINVAL;
    if ((e.virtual_rgba_bHW4 != nullptr) == (e.has_colour != 0)) return IDH_EINVAL;  // neither or both
    const bool depth = e.mode >= IDH_COMPOSITE_DEPTH_SOFT;
    if (depth ? (e.virtual_depth_bHW != nullptr) == (e.has_plane != 0) : (e.virtual_depth_bHW || e.has_plane)) return IDH_EINVAL;
    const long long lim = (1ll << 31) - 4;
    if ((long long)e.B * e.H * e.W >= lim || (long long)e.B * e.h * e.w >= lim) return IDH_EUNSUPPORTED;
    if (e.B == 0) return IDH_OK;
    CompArgs a{};
    a.image = e.image_bHW3, a.rgba = e.virtual_rgba_bHW4, a.map = e.map_b1hw, a.vdepth = e.virtual_depth_bHW, a.fade = e.fade_b;
    a.out = e.out_bHW3, a.matte_out = e.matte_out_bHW, a.plane = 1.0 * e.plane_distance;
    for (int c = 0; c < 3; ++c) a.colour[c] = e.colour[c];
    a.mult = e.sigmoid_multiplier, a.sy = (float)e.h / e.H, a.sx = (float)e.w / e.W;
    a.h = e.h, a.w = e.w, a.H = e.H, a.W = e.W;
    a.HW = (unsigned)e.H * e.W, a.N = a.HW * (unsigned)e.B;
    a.bgr = e.bgr != 0;
    a.small = (long long)e.H + e.W <= 128;
    a.vec = aligned(a.image, 4) && aligned(a.out, 4) && aligned(a.rgba, 16) && aligned(a.vdepth, 16) && aligned(a.matte_out, 16);
    const bool resize = e.h != e.H || e.w != e.W;  // (:117): a map of the image's size is used as it is
    const dim3 grid(idh_cdiv(idh_cdiv(a.N, 4), 256));
    hipStream_t st = idh_stream(stream);
    const bool rgba = a.rgba != nullptr;
    switch (e.mode) {
        case IDH_COMPOSITE_MASK_LOGITS: launch1<kLogits>(rgba, resize, grid, st, a); break;
        case IDH_COMPOSITE_MASK_PROB: launch1<kProb>(rgba, resize, grid, st, a); break;
        case IDH_COMPOSITE_DEPTH_SOFT:
            if (e.has_plane)
                launch1<kDepthSoftPlane>(rgba, resize, grid, st, a);
            else
                launch1<kDepthSoftMap>(rgba, resize, grid, st, a);
            break;
        default:
            if (e.has_plane)
                launch1<kDepthHardPlane>(rgba, resize, grid, st, a);
            else
                launch1<kDepthHardMap>(rgba, resize, grid, st, a);
    }
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
