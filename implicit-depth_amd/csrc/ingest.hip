// Frame ingest (include/idh_ingest.h): what the reference's dataset code does on the CPU between a camera frame and the model's inputs.
//
//   resize coefficients     Pillow's per-dimension bounds and fixed-point taps, computed on the host in doubles (no GPU call)
//   ingest_color_k          utils/generic_utils.py:210-212 + :149-152: Image.resize (BILINEAR / BICUBIC, antialiased), to_tensor and the
//                           ImageNet normalisation in one launch; the horizontal pass's image exists only in LDS
//   ingest_depth_k          datasets/scannet_dataset.py:515-530, :550-561: NEAREST resize of the uint16 depth, * value_scale, validity masks,
//                           NaN where invalid; the target-size and the full-resolution triple from one launch
//
// ingest_color_k: a workgroup owns an 8 x 64 output tile of one frame.  It copies the tile's rows of the two tap tables into LDS
// (x taps at a row length of 33 ints: odd, so lanes over x fall on different banks), takes the source rows the tile's first and last output
// rows reach, runs the horizontal pass for them into LDS AS uint8 (Pillow rounds and clips after the first pass, and the second pass sees
// that), runs the vertical pass out of LDS into the tile's interleaved bytes, and stores those bytes (16 B per lane) and the planar floats
// (float4 per lane); sizes or pointers that do not allow the wide stores take the per-element path.  Taps and sums are int32:
// sum |taps| < 2^23 and a sample is at most 255.  The LDS image holds 92 source rows: 7 * 8 + 2 * 16 + 2 = 90 is the most a tile can reach at the
// supported ratio of 8 with bicubic taps, whatever the image size.  Tables come from the caller, so every index read from them is
// clamped to the source before it is used.
// The source is read straight from global memory, one byte per tap and channel; neighbouring lanes overlap in the lines they read.
#include <math.h>

#include "idh_common.h"

#include "../../include/idh_ingest.h"

namespace {

constexpr int kPrecisionBits = 22;  // Pillow: 32 - 8 - 2
constexpr int TH = 8, TW = 64;      // output tile
constexpr int MAXK = 33;            // 2 * ceil(2 * 8) + 1: bicubic at ratio 8
constexpr int MAXROWS = 92;         // source rows a tile's vertical pass can reach (see above)
constexpr int ROWB = TW * 3;        // bytes of one tile row, interleaved RGB

// ---- coefficients (host) ----------------------------------------------------------------------------------------------------------
double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

int coeffs_check(int in, int out, int filter) {
    if (in <= 0 || out <= 0 || (filter != IDH_RESIZE_BILINEAR && filter != IDH_RESIZE_BICUBIC)) return IDH_EINVAL;
    if ((long long)in > (long long)IDH_INGEST_MAX_RATIO * out) return IDH_EUNSUPPORTED;
    return IDH_OK;
}

double filter_support(int filter) { return filter == IDH_RESIZE_BICUBIC ? 2.0 : 1.0; }

int coeffs_ksize(int in, int out, int filter) {
    double filterscale = (double)in / out;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(filter_support(filter) * filterscale) * 2 + 1;
}

__device__ __forceinline__ unsigned char clip8(int acc) {
    const int v = acc >> kPrecisionBits;  // arithmetic shift: a negative sum stays negative
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- colour -------------------------------------------------------------------------------------------------------------------------
struct ColorArgs {
    const unsigned char *src;  // (B,Hs,Ws,3)
    const int *xb, *xt;        // horizontal bounds / taps, or null: pass skipped
    const int *yb, *yt;
    float *img;                // (B,3,h,w) or null
    unsigned char *u8;         // (B,h,w,3) or null
    int Hs, Ws, h, w, kx, ky;
    int normalize;
    int vec_img, vec_u8;  // the wide store paths are allowed (size and alignment)
};

// to_tensor (u8.float().div(255)) and normalize (.sub_(mean).div_(std)): IEEE fp32, `/` is correctly rounded, nothing contracts
__device__ __forceinline__ float to_model(unsigned v, int c, bool normalize) {
    float f = (float)v / 255.f;
    if (normalize) {
        const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f), stdv = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
        f = (f - mean) / stdv;
    }
    return f;
}

__global__ __launch_bounds__(256) void ingest_color_k(const ColorArgs a) {
    __shared__ int s_xt[TW * MAXK], s_yt[TH * MAXK];
    __shared__ int s_xb[TW * 2], s_yb[TH * 2];
    __shared__ __attribute__((aligned(16))) unsigned char s_mid[MAXROWS * ROWB];  // horizontal pass of the source rows the tile reaches
    __shared__ __attribute__((aligned(16))) unsigned char s_out[TH * ROWB];       // the tile's resized bytes
    const int tid = threadIdx.x, b = blockIdx.z, ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
    const int tw = min(TW, a.w - ox0), th = min(TH, a.h - oy0);
    const bool hp = a.xb != nullptr, vp = a.yb != nullptr;

    if (hp) {
        for (int i = tid; i < tw; i += 256) {
            const int first = clampi(a.xb[2 * (ox0 + i)], 0, a.Ws - 1);
            s_xb[2 * i] = first, s_xb[2 * i + 1] = clampi(a.xb[2 * (ox0 + i) + 1], 0, min(a.kx, a.Ws - first));
        }
        for (int i = tid; i < tw * a.kx; i += 256) {
            const int x = i / a.kx, k = i - x * a.kx;
            s_xt[x * MAXK + k] = a.xt[(size_t)ox0 * a.kx + i];
        }
    }
    if (vp) {
        for (int i = tid; i < th; i += 256) {
            const int first = clampi(a.yb[2 * (oy0 + i)], 0, a.Hs - 1);
            s_yb[2 * i] = first, s_yb[2 * i + 1] = clampi(a.yb[2 * (oy0 + i) + 1], 0, min(a.ky, a.Hs - first));
        }
        for (int i = tid; i < th * a.ky; i += 256) {
            const int y = i / a.ky, k = i - y * a.ky;
            s_yt[y * MAXK + k] = a.yt[(size_t)oy0 * a.ky + i];
        }
    }
    __syncthreads();

    int r0 = oy0, nrows = th;  // source rows [r0, r0 + nrows) feed the tile
    if (vp) {
        int r1 = 0;
        r0 = a.Hs;
        for (int j = 0; j < th; ++j) r0 = min(r0, s_yb[2 * j]), r1 = max(r1, s_yb[2 * j] + s_yb[2 * j + 1]);
        nrows = min(r1 - r0, MAXROWS);
    }

    // horizontal pass (or a copy), one (row, x) with its three channels per step
    const unsigned char *frame = a.src + (size_t)b * a.Hs * a.Ws * 3;
    for (int it = tid; it < nrows * tw; it += 256) {
        const int r = it / tw, x = it - r * tw;
        const unsigned char *row = frame + (size_t)(r0 + r) * a.Ws * 3;
        unsigned char *m = s_mid + r * ROWB + x * 3;
        if (hp) {
            const unsigned char *p = row + (size_t)s_xb[2 * x] * 3;
            const int n = s_xb[2 * x + 1];
            const int *t = s_xt + x * MAXK;
            int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
            for (int k = 0; k < n; ++k) {
                const int c = t[k];
                a0 += (int)p[3 * k] * c, a1 += (int)p[3 * k + 1] * c, a2 += (int)p[3 * k + 2] * c;
            }
            m[0] = clip8(a0), m[1] = clip8(a1), m[2] = clip8(a2);
        } else {
            const unsigned char *p = row + (size_t)(ox0 + x) * 3;
            m[0] = p[0], m[1] = p[1], m[2] = p[2];
        }
    }
    __syncthreads();

    // vertical pass (or a copy) over the tile's interleaved bytes
    const int rowb = tw * 3;
    for (int it = tid; it < th * rowb; it += 256) {
        const int y = it / rowb, j = it - y * rowb;
        unsigned char v;
        if (vp) {
            const int first = s_yb[2 * y] - r0, n = s_yb[2 * y + 1];
            const int *t = s_yt + y * MAXK;
            int acc = 1 << (kPrecisionBits - 1);
            for (int k = 0; k < n; ++k) acc += (int)s_mid[min(first + k, MAXROWS - 1) * ROWB + j] * t[k];
            v = clip8(acc);
        } else {
            v = s_mid[y * ROWB + j];
        }
        s_out[y * ROWB + j] = v;
    }
    __syncthreads();

    if (a.u8) {
        unsigned char *dst = a.u8 + (((size_t)b * a.h + oy0) * a.w + ox0) * 3;
        const size_t stride = (size_t)a.w * 3;
        if (a.vec_u8) {  // w % 16 == 0: a tile row is a whole number of 16-byte pieces, each aligned
            const int q = rowb / 16;
            for (int it = tid; it < th * q; it += 256) {
                const int y = it / q, j = it - y * q;
                *reinterpret_cast<uint4 *>(dst + y * stride + 16 * j) = *reinterpret_cast<const uint4 *>(s_out + y * ROWB + 16 * j);
            }
        } else {
            for (int it = tid; it < th * rowb; it += 256) {
                const int y = it / rowb, j = it - y * rowb;
                dst[y * stride + j] = s_out[y * ROWB + j];
            }
        }
    }
    if (a.img) {
        const bool norm = a.normalize != 0;
        const size_t plane = (size_t)a.h * a.w;
        float *dst = a.img + (size_t)b * 3 * plane + (size_t)oy0 * a.w + ox0;
        if (a.vec_img) {  // w % 4 == 0
            const int q = tw / 4;
            for (int it = tid; it < 3 * th * q; it += 256) {
                const int c = it / (th * q), rem = it - c * (th * q), y = rem / q, x = 4 * (rem - y * q);
                const unsigned char *s = s_out + y * ROWB + 3 * x + c;
                *reinterpret_cast<float4 *>(dst + c * plane + (size_t)y * a.w + x) =
                    make_float4(to_model(s[0], c, norm), to_model(s[3], c, norm), to_model(s[6], c, norm), to_model(s[9], c, norm));
            }
        } else {
            for (int it = tid; it < 3 * th * tw; it += 256) {
                const int c = it / (th * tw), rem = it - c * (th * tw), y = rem / tw, x = rem - y * tw;
                dst[c * plane + (size_t)y * a.w + x] = to_model(s_out[y * ROWB + 3 * x + c], c, norm);
            }
        }
    }
}

// ---- depth --------------------------------------------------------------------------------------------------------------------------
struct DepthOut {
    float *depth, *mask;
    unsigned char *mask_b;
    int H, W;
    unsigned N;        // B * H * W
    double sy, sx;     // Hs / H, Ws / W
    int resize, vec;
};

struct DepthArgs {
    const unsigned short *src;  // (B,Hs,Ws)
    DepthOut target, full;
    float scale, lo, hi;
    int Hs, Ws;
};

// Four consecutive pixels of the flat (B,H,W) run per lane: 16-byte stores for the two float maps, one dword for the four bools.
__device__ __forceinline__ void depth_group(const DepthArgs &a, const DepthOut &o, unsigned g) {
    const unsigned p0 = g * 4u;
    if (!o.depth || p0 >= o.N) return;
    const int n = (int)min(4u, o.N - p0);
    const unsigned HW = (unsigned)o.H * o.W;
    float d[4], m[4];
    alignas(4) unsigned char mb[4];
    for (int k = 0; k < n; ++k) {
        const unsigned p = p0 + k, b = p / HW, r = p - b * HW;
        int y = (int)(r / (unsigned)o.W), x = (int)(r - (unsigned)y * o.W);
        if (o.resize) {  // Pillow's NEAREST: the step is a double, rounded before it is multiplied
            y = min((int)(((double)y + 0.5) * o.sy), a.Hs - 1);
            x = min((int)(((double)x + 0.5) * o.sx), a.Ws - 1);
        }
        const float f = (float)a.src[((size_t)b * a.Hs + y) * a.Ws + x] * a.scale;
        const bool ok = f > a.lo && f < a.hi;
        d[k] = ok ? f : __builtin_nanf(""), m[k] = ok ? 1.f : 0.f, mb[k] = ok ? 1 : 0;
    }
    if (o.vec && n == 4) {
        *reinterpret_cast<float4 *>(o.depth + p0) = make_float4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<float4 *>(o.mask + p0) = make_float4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<unsigned *>(o.mask_b + p0) = *reinterpret_cast<const unsigned *>(mb);
    } else {
        for (int k = 0; k < n; ++k) o.depth[p0 + k] = d[k], o.mask[p0 + k] = m[k], o.mask_b[p0 + k] = mb[k];
    }
}

__global__ __launch_bounds__(256) void ingest_depth_k(const DepthArgs a) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    depth_group(a, a.target, g);
    depth_group(a, a.full, g);
}

bool aligned(const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace

extern "C" size_t idh_sizeof_ingest_color_args(void) { return sizeof(idh_ingest_color_args); }
extern "C" size_t idh_sizeof_ingest_depth_args(void) { return sizeof(idh_ingest_depth_args); }

extern "C" int idh_resize_coeffs_sizes(int in, int out, int filter, int64_t *n_bounds, int64_t *n_taps) {
    if (const int e = coeffs_check(in, out, filter)) return e;
    if (!n_bounds || !n_taps) return IDH_EINVAL;
    *n_bounds = 2ll * out;
    *n_taps = (int64_t)out * coeffs_ksize(in, out, filter);
    return IDH_OK;
}

extern "C" int idh_resize_coeffs_pack(int in, int out, int filter, int32_t *bounds_out, int32_t *taps_out) {
    if (const int e = coeffs_check(in, out, filter)) return e;
    if (!bounds_out || !taps_out) return IDH_EINVAL;
    double (*const f)(double) = filter == IDH_RESIZE_BICUBIC ? bicubic_filter : bilinear_filter;
    const double scale = (double)in / out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support(filter) * filterscale;
    const int ksize = coeffs_ksize(in, out, filter);
    double w[MAXK];
    for (int i = 0; i < out; ++i) {
        const double center = (i + 0.5) * scale;
        int first = (int)(center - support + 0.5);
        if (first < 0) first = 0;
        int last = (int)(center + support + 0.5);
        if (last > in) last = in;
        const int n = last - first;  // <= ksize <= MAXK by the ratio check
        double sum = 0.0;
        for (int k = 0; k < n; ++k) {
            w[k] = f((k + first - center + 0.5) / filterscale);
            sum += w[k];
        }
        bounds_out[2 * i] = first, bounds_out[2 * i + 1] = n;
        int32_t *t = taps_out + (size_t)i * ksize;
        for (int k = 0; k < ksize; ++k) {
            if (k >= n) {
                t[k] = 0;
                continue;
            }
            const double v = sum != 0.0 ? w[k] / sum : w[k];
            t[k] = (int32_t)((v < 0 ? -0.5 : 0.5) + v * (double)(1 << kPrecisionBits));
        }
    }
    return IDH_OK;
}

extern "C" int idh_ingest_color_fwd(const idh_ingest_color_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_ingest_color_args)) return IDH_EINVAL;
    const idh_ingest_color_args &e = *args;
    if (e.B < 0 || e.Hs <= 0 || e.Ws <= 0 || e.h <= 0 || e.w <= 0) return IDH_EINVAL;
    if (e.filter != IDH_RESIZE_BILINEAR && e.filter != IDH_RESIZE_BICUBIC) return IDH_EINVAL;
    if (!e.frames_bHW3 || (!e.image_b3hw && !e.resized_bhw3)) return IDH_EINVAL;
    const bool hp = e.Ws != e.w, vp = e.Hs != e.h;
    if ((e.x_bounds != nullptr) != hp || (e.x_taps != nullptr) != hp || (e.y_bounds != nullptr) != vp || (e.y_taps != nullptr) != vp) return IDH_EINVAL;
    if ((long long)e.Hs > (long long)IDH_INGEST_MAX_RATIO * e.h || (long long)e.Ws > (long long)IDH_INGEST_MAX_RATIO * e.w) return IDH_EUNSUPPORTED;
    if (e.B > 65535 || e.h > TH * 65535 || (long long)e.Hs * e.Ws >= (1ll << 29) || (long long)e.h * e.w >= (1ll << 29)) return IDH_EUNSUPPORTED;
    if (e.B == 0) return IDH_OK;
    ColorArgs a{};
    a.src = e.frames_bHW3, a.xb = e.x_bounds, a.xt = e.x_taps, a.yb = e.y_bounds, a.yt = e.y_taps, a.img = e.image_b3hw, a.u8 = e.resized_bhw3;
    a.Hs = e.Hs, a.Ws = e.Ws, a.h = e.h, a.w = e.w;
    a.kx = hp ? coeffs_ksize(e.Ws, e.w, e.filter) : 0, a.ky = vp ? coeffs_ksize(e.Hs, e.h, e.filter) : 0;  // <= MAXK by the ratio check
    a.normalize = e.normalize != 0;
    a.vec_img = e.w % 4 == 0 && aligned(a.img, 16);
    a.vec_u8 = e.w % 16 == 0 && aligned(a.u8, 16);
    hipLaunchKernelGGL(ingest_color_k, dim3(idh_cdiv(e.w, TW), idh_cdiv(e.h, TH), e.B), dim3(256), 0, idh_stream(stream), a);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_ingest_depth_fwd(const idh_ingest_depth_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_ingest_depth_args)) return IDH_EINVAL;
    const idh_ingest_depth_args &e = *args;
    const bool target = e.depth_b1hw || e.mask_b1hw || e.mask_b_b1hw, full = e.full_depth_b1HW || e.full_mask_b1HW || e.full_mask_b_b1HW;
    if (e.B < 0 || e.Hs <= 0 || e.Ws <= 0 || (target && (e.h <= 0 || e.w <= 0))) return IDH_EINVAL;
    if (!e.depth_bHW || (!target && !full)) return IDH_EINVAL;
    if (target && !(e.depth_b1hw && e.mask_b1hw && e.mask_b_b1hw)) return IDH_EINVAL;
    if (full && !(e.full_depth_b1HW && e.full_mask_b1HW && e.full_mask_b_b1HW)) return IDH_EINVAL;
    const long long lim = (1ll << 31) - 4;
    if ((long long)e.B * e.Hs * e.Ws >= lim || (target && (long long)e.B * e.h * e.w >= lim)) return IDH_EUNSUPPORTED;
    if (e.B == 0) return IDH_OK;
    DepthArgs a{};
    a.src = e.depth_bHW, a.scale = e.value_scale, a.lo = e.min_valid, a.hi = e.max_valid, a.Hs = e.Hs, a.Ws = e.Ws;
    unsigned groups = 0;
    if (target) {
        DepthOut &o = a.target;
        o.depth = e.depth_b1hw, o.mask = e.mask_b1hw, o.mask_b = e.mask_b_b1hw, o.H = e.h, o.W = e.w, o.N = (unsigned)e.B * e.h * e.w;
        o.sy = (double)e.Hs / e.h, o.sx = (double)e.Ws / e.w, o.resize = e.h != e.Hs || e.w != e.Ws;
        o.vec = aligned(o.depth, 16) && aligned(o.mask, 16) && aligned(o.mask_b, 4);
        groups = (unsigned)idh_cdiv(o.N, 4);
    }
    if (full) {
        DepthOut &o = a.full;
        o.depth = e.full_depth_b1HW, o.mask = e.full_mask_b1HW, o.mask_b = e.full_mask_b_b1HW, o.H = e.Hs, o.W = e.Ws, o.N = (unsigned)e.B * e.Hs * e.Ws;
        o.sy = o.sx = 1.0, o.resize = 0;
        o.vec = aligned(o.depth, 16) && aligned(o.mask, 16) && aligned(o.mask_b, 4);
        groups = max(groups, (unsigned)idh_cdiv(o.N, 4));
    }
    hipLaunchKernelGGL(ingest_depth_k, dim3(idh_cdiv(groups, 256)), dim3(256), 0, idh_stream(stream), a);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
