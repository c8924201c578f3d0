// The ResNet18 stem of the matching encoder up to the max-pool (IDH_OP_STEM, include/idh_ops.h): conv1 7x7/2 3->64 with the
// eval-mode BatchNorm folded into weights and bias, ReLU, MaxPool2d(2, 1) and the anti-aliasing BlurPool (ReflectionPad2d((1, 2, 1, 2))
// + depthwise 4x4 binomial, stride 2) of antialiased_cnns.resnet18(filter_size=4, pool_only=True) (implicit-depth_amd/backbone.py) in
// ONE pass: the (H/2 x W/2 x 64) conv1 map never reaches HBM.
//
// Geometry (Hc = ceil(H/2) conv1 rows, Hm = Hc - 1 max-pooled rows, Ho = floor(Hc/2) output rows; the same for columns):
//   output row oy reads max-pooled rows 2oy-1 .. 2oy+2, reflected (-1 -> 1, Hm -> Hm-2, Hm+1 -> Hm-3);
//   max-pooled row r reads conv1 rows r, r+1; conv1 pads its input with zeros (pad 3).
// A workgroup owns an 8 x 16 output tile of one image; all the max-pooled rows it reads lie in conv1 rows 2oy0-2 .. 2oy0+17 (20 rows,
// the first one only for a reflected bottom edge) and columns 2ox0-2 .. 2ox0+33 (36): a 720-pixel conv1 tile, 1.41x the 512 conv1 pixels the
// tile owns.  64 channels of that tile would take 184 KB of LDS, so the channels go in four 16-channel quarters that share one staged input
// patch (3 x 45 x 78 floats, 41 KB):
//   1. conv1 as an implicit GEMM on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate): M = 16 conv1 pixels, N = 16 channels, K = 3 x 7 x 8
//      taps (kx padded 7 -> 8 with a zero weight, 42 K-steps instead of 37): lane quarter q of K-step (ci, ky, kx/4) reads tap kx = 4 (kx/4) + q,
//      so every A operand is one LDS read at a compile-time offset from the lane's pixel.  The 42 B fragments (this quarter's folded weights)
//      live in registers.  + bias, ReLU -> LDS conv tile;
//   2. max-pool + the horizontal blur pass (taps [1, 3, 3, 1] / 8) -> LDS (18 rows x 16 columns x 16 channels);
//   3. vertical blur pass -> HBM (NHWC, 64-byte channel runs of a channel-strided output).
// Error against fp64: the conv1 sum is an fmaf chain of 147 products (~1e-7 of the output scale); max-pool and blur add a few roundings.
#include <math.h>

#include "idh_common.h"
#include "../../include/idh_ops.h"

namespace idh_stem {

constexpr int kTY = 8, kTX = 16;                       // output tile
constexpr int kCR = 2 * kTY + 4, kCC = 2 * kTX + 4;    // conv1 tile (20 x 36)
constexpr int kNPix = kCR * kCC;                       // 720 = 45 MFMA row groups
constexpr int kGroups = kNPix / 16;
constexpr int kPR = 2 * (kCR - 1) + 7;                 // input patch rows (45)
constexpr int kPW = 2 * (kCC - 1) + 8;                 // input patch columns (78: kx up to 7)
constexpr int kPHW = kPR * kPW;
constexpr int kPatch = 3 * kPHW;                       // 10530 floats
constexpr int kConvCs = 17;                            // floats per conv1-tile pixel (16 channels + 1: bank spread of the accumulator stores)
constexpr int kConv = kNPix * kConvCs;                 // 12240
constexpr int kHR = 2 * kTY + 2;                       // max-pooled rows of the tile (18)
constexpr int kHoriz = kHR * kTX * 16;                 // 4608
constexpr int kSteps = 3 * 7 * 2;                      // 42 K-steps of 4 taps
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
static_assert(kNPix % 16 == 0, "conv1 tile must be whole MFMA row groups");
static_assert((kPatch + kConv + kHoriz) * 4 <= 160 * 1024, "LDS budget");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct StemArgs {
    const float *in;      // image 0, NCHW fp32
    const float *blob;    // idh_pack_stem_weight output: [quarter 4][step 42][lane 64] then bias[64]
    float *out;           // NHWC, 64 channels at channel offset 0 of each pixel, out_cs floats per pixel
    long long img_stride; // floats between consecutive images of a group
    long long grp_stride; // floats between groups
    int group;            // images per group
    int H, W, Hm, Wm, Ho, Wo, out_cs;
    int tiles_x, tiles_per_img;
};

// reflection of ReflectionPad2d((1, 2, 1, 2)) about [0, n) (only -1, n, n+1 occur for the rows an output row reads); clamped for the rows of
// a partial tile's unused outputs
__device__ __forceinline__ int refl(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(kThreads) void stem_conv7_pool_k(const StemArgs a) {
    __shared__ __attribute__((aligned(16))) float s_patch[kPatch];
    __shared__ __attribute__((aligned(16))) float s_conv[kConv];
    __shared__ __attribute__((aligned(16))) float s_h[kHoriz];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long b = blockIdx.x;
    const long long n = b / a.tiles_per_img;
    const int t = (int)(b - n * a.tiles_per_img);
    const int oy0 = (t / a.tiles_x) * kTY, ox0 = (t % a.tiles_x) * kTX;
    const int base_r = 2 * oy0 - 2, base_c = 2 * ox0 - 2;   // conv1 row / column of conv-tile (0, 0)
    const long long grp = n / a.group;
    const float *img = a.in + grp * a.grp_stride + (n - grp * a.group) * a.img_stride;
    const long long HW = (long long)a.H * a.W;

    // ---- 0. input patch: rows 2 base_r - 3 .., columns 2 base_c - 3 .., zeros outside the image (conv1's zero padding)
    const int iy0 = 2 * base_r - 3, ix0 = 2 * base_c - 3;
    for (int i = tid; i < kPatch; i += kThreads) {
        const int ci = i / kPHW, rem = i - ci * kPHW;
        const int r = rem / kPW, c = rem - r * kPW;
        const int iy = iy0 + r, ix = ix0 + c;
        float v = 0.f;
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = img[ci * HW + (long long)iy * a.W + ix];
        s_patch[i] = v;
    }

    const int ln = lane & 15, q = lane >> 4;
    float *outp = a.out + ((long long)n * a.Ho * a.Wo) * a.out_cs;
    for (int Q = 0; Q < 4; ++Q) {
        // ---- B fragments of this channel quarter (lane: channel 16 Q + ln, tap quarter q) and its bias
        float wreg[kSteps];
        const float *wq = a.blob + (size_t)Q * kSteps * 64 + lane;
#pragma unroll
        for (int s = 0; s < kSteps; ++s) wreg[s] = wq[s * 64];
        const float bias = a.blob[4 * kSteps * 64 + 16 * Q + ln];
        __syncthreads();  // patch staged (Q = 0) / previous quarter's conv tile and max-pool reads done

        // ---- 1. conv1 tile: 45 groups of 16 pixels over the waves
        for (int g = wave; g < kGroups; g += kWaves) {
            const int m = 16 * g + ln;
            const int cy = m / kCC, cx = m - cy * kCC;
            const float *pa = s_patch + (2 * cy) * kPW + 2 * cx + q;
            float av[kSteps];
#pragma unroll
            for (int ci = 0; ci < 3; ++ci)
#pragma unroll
                for (int ky = 0; ky < 7; ++ky)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) av[(ci * 7 + ky) * 2 + kb] = pa[ci * kPHW + ky * kPW + 4 * kb];
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < kSteps; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], wreg[s], acc, 0, 0, 0);
            // D[row = pixel 4 q + r][col = channel ln]
#pragma unroll
            for (int r = 0; r < 4; ++r) s_conv[(16 * g + 4 * q + r) * kConvCs + ln] = fmaxf(acc[r] + bias, 0.f);
        }
        __syncthreads();

        // ---- 2. max-pool + horizontal blur: s_h[j][x][c] = sum_k a_k / 8 * mp(row 2 oy0 - 1 + j, column 2 (ox0 + x) - 1 + k)
        for (int i = tid; i < kHoriz; i += kThreads) {
            const int c = i & 15, x = (i >> 4) & 15, j = i >> 8;
            // (clamped into the tile: only the unused rows / columns of a partial tile's outputs leave it)
            const int lr = min(max(refl(2 * oy0 - 1 + j, a.Hm) - base_r, 0), kCR - 2);
            const float *r0 = s_conv + lr * kCC * kConvCs + c;
            const float *r1 = r0 + kCC * kConvCs;
            float hsum = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int lc = min(max(refl(2 * (ox0 + x) - 1 + k, a.Wm) - base_c, 0), kCC - 2);
                const float mp = fmaxf(fmaxf(r0[lc * kConvCs], r0[(lc + 1) * kConvCs]), fmaxf(r1[lc * kConvCs], r1[(lc + 1) * kConvCs]));
                hsum = fmaf((k == 0 || k == 3) ? 0.125f : 0.375f, mp, hsum);
            }
            s_h[i] = hsum;
        }
        __syncthreads();

        // ---- 3. vertical blur -> out (16 channels = 64 contiguous bytes per pixel)
        for (int i = tid; i < kTY * kTX * 16; i += kThreads) {
            const int c = i & 15, x = (i >> 4) & 15, y = i >> 8;
            const int oy = oy0 + y, ox = ox0 + x;
            if (oy >= a.Ho || ox >= a.Wo) continue;
            const float *hp = s_h + ((2 * y) * kTX + x) * 16 + c;
            float v = 0.125f * hp[0];
            v = fmaf(0.375f, hp[kTX * 16], v);
            v = fmaf(0.375f, hp[2 * kTX * 16], v);
            v = fmaf(0.125f, hp[3 * kTX * 16], v);
            outp[((long long)oy * a.Wo + ox) * a.out_cs + 16 * Q + c] = v;
        }
        // (the next quarter's first barrier orders these s_h reads before its max-pool pass rewrites s_h)
    }
}

// folded conv1 weights in MFMA B-fragment order: dst[Q][s][lane] = w[16 Q + (lane & 15)][ci][ky][4 kb + (lane >> 4)] * g / sqrt(var + eps),
// s = (ci * 7 + ky) * 2 + kb, 0 for kx = 7; then the 64 folded biases beta - mean * g / sqrt(var + eps)
__global__ __launch_bounds__(256) void stem_pack_k(const float *__restrict__ w, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                   const float *__restrict__ mean, const float *__restrict__ var, float eps, float *__restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int nw = 4 * kSteps * 64;
    if (i < nw) {
        const int lane = i & 63, s = (i >> 6) % kSteps, Q = i / (64 * kSteps);
        const int co = 16 * Q + (lane & 15), kx = 4 * (s & 1) + (lane >> 4), ky = (s >> 1) % 7, ci = (s >> 1) / 7;
        const float sc = gamma[co] / sqrtf(var[co] + eps);
        dst[i] = kx < 7 ? w[((co * 3 + ci) * 7 + ky) * 7 + kx] * sc : 0.f;
    } else if (i < nw + 64) {
        const int co = i - nw;
        const float sc = gamma[co] / sqrtf(var[co] + eps);
        dst[i] = beta[co] - mean[co] * sc;
    }
}

__global__ __launch_bounds__(256) void fold_conv_bn_k(const float *__restrict__ w, int cout, int per_out, const float *__restrict__ gamma,
                                                      const float *__restrict__ beta, const float *__restrict__ mean, const float *__restrict__ var, float eps,
                                                      float *__restrict__ w_out, float *__restrict__ b_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nw = (long long)cout * per_out;
    if (i < nw) {
        const int co = (int)(i / per_out);
        w_out[i] = w[i] * (gamma[co] / sqrtf(var[co] + eps));
    } else if (i < nw + cout) {
        const int co = (int)(i - nw);
        b_out[co] = beta[co] - mean[co] * (gamma[co] / sqrtf(var[co] + eps));
    }
}

}  // namespace idh_stem

using namespace idh_stem;

// validation + launch of one IDH_OP_STEM (called by idh_run_ops, csrc/conv.hip; `launch` false: validate only, for idh_count_launches)
int idh_stem_op(const idh_op &op, hipStream_t st, bool launch) {
    const idh_conv_src &s = op.src[0];
    if (!s.in || !s.w || !op.out || op.N <= 0 || s.Cin != 3 || op.Cout != 64 || op.out_cs < 64 || (op.out_cs & 3) || ((uintptr_t)op.out & 15))
        return IDH_EINVAL;
    if (s.H < 8 || s.W < 8) return IDH_EINVAL;  // the reflection needs Hm, Wm >= 3
    const int Hc = (s.H + 1) / 2, Wc = (s.W + 1) / 2;
    if (op.Ho != Hc / 2 || op.Wo != Wc / 2) return IDH_EINVAL;
    const int group = s.up_C > 0 ? s.up_C : op.N;
    if (op.N % group || s.up_cs[0] < 0 || s.up_cs[1] < 0) return IDH_EINVAL;
    StemArgs a{};
    a.in = s.in; a.blob = s.w; a.out = op.out;
    a.img_stride = s.up_cs[0] ? s.up_cs[0] : 3ll * s.H * s.W;
    a.grp_stride = s.up_cs[1] ? s.up_cs[1] : a.img_stride * group;
    a.group = group;
    a.H = s.H; a.W = s.W; a.Hm = Hc - 1; a.Wm = Wc - 1; a.Ho = op.Ho; a.Wo = op.Wo; a.out_cs = op.out_cs;
    a.tiles_x = idh_cdiv(op.Wo, kTX);
    a.tiles_per_img = idh_cdiv(op.Ho, kTY) * a.tiles_x;
    const long long blocks = (long long)op.N * a.tiles_per_img;
    if (blocks >= (1ll << 31)) return IDH_EUNSUPPORTED;
    if (!launch) return IDH_OK;
    hipLaunchKernelGGL(stem_conv7_pool_k, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    return hipGetLastError() == hipSuccess ? IDH_OK : IDH_ELAUNCH;
}

extern "C" size_t idh_stem_weight_floats(void) { return 4 * kSteps * 64 + 64; }

extern "C" int idh_pack_stem_weight(const float *w_oihw, const float *bn_weight, const float *bn_bias, const float *bn_mean, const float *bn_var, float eps,
                                    float *dst, void *stream) {
    if (!w_oihw || !bn_weight || !bn_bias || !bn_mean || !bn_var || !dst || !(eps >= 0.f)) return IDH_EINVAL;
    const int total = (int)idh_stem_weight_floats();
    hipLaunchKernelGGL(stem_pack_k, dim3(idh_cdiv(total, 256)), dim3(256), 0, idh_stream(stream), w_oihw, bn_weight, bn_bias, bn_mean, bn_var, eps, dst);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_fold_conv_bn(const float *w, int cout, int per_out, const float *bn_weight, const float *bn_bias, const float *bn_mean,
                                const float *bn_var, float eps, float *w_out, float *b_out, void *stream) {
    if (!w || !bn_weight || !bn_bias || !bn_mean || !bn_var || !w_out || !b_out || cout <= 0 || per_out <= 0 || !(eps >= 0.f)) return IDH_EINVAL;
    const long long total = (long long)cout * per_out + cout;
    if (total >= (1ll << 31)) return IDH_EUNSUPPORTED;
    hipLaunchKernelGGL(fold_conv_bn_k, dim3(idh_cdiv(total, 256)), dim3(256), 0, idh_stream(stream), w, cout, per_out, bn_weight, bn_bias, bn_mean,
                       bn_var, eps, w_out, b_out);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
