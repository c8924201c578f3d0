// Edge mask of a depth map and the validation losses that read it (include/idh_geometry.h).
//
//   edge_sobel_k      S = sobel(1 / depth): kornia.filters.sobel(normalized=True, eps=1e-6) as utils/generic_utils.py:287 calls it
//   edge_select_k     per image the exact nanquantile of S (torch.nanquantile, linear interpolation): one workgroup per image, a radix
//                     select over order-preserving 32-bit keys, four 8-bit digits, integer histograms in LDS
//   edge_mask_k       S > threshold and the 5x5 max-pool of :291 as an OR over the in-image window
//   bd_val_partial_k  the phase != "train" branch of BDModel.compute_binary_losses (bd_model.py:451-495): per chunk of 2048 elements one
//   bd_val_finalise_k partial in the workspace, then one workgroup that adds the partials in a fixed order
//
// Built with -ffp-contract=off and without any fast-math flag: 1 / depth and sqrt are the correctly rounded IEEE operations, every product
// and sum of the Sobel taps is rounded on its own and the zero taps are multiplied too (0 * inf = NaN, as in the convolution the
// reference runs), so the NaN and inf sets of S are the composition's.  No floating-point atomics anywhere; no workgroup waits on another
// (the three stages are three launches); two runs give the same bits.
#include "idh_common.h"

#include "../../include/idh_geometry.h"

#include <math.h>

namespace {

constexpr int kTW = 64, kTH = 8;

// ---- Sobel magnitude of the disparity ---------------------------------------------------------------------------------------------------
// One workgroup of 256 lanes owns a 64 x 8 tile; the 66 x 10 disparities 1 / depth it reads (replicate border: positions clamped into the
// image) are divided once and kept in LDS.
__global__ __launch_bounds__(256) void edge_sobel_k(const float *__restrict__ depth, float *__restrict__ S, int H, int W, int tiles_x,
                                                    int tiles_y) {
    __shared__ float inv[kTH + 2][kTW + 2];
    const int tid = threadIdx.x;
    unsigned t = blockIdx.x;
    const int tx = (int)(t % (unsigned)tiles_x);
    t /= (unsigned)tiles_x;
    const int ty = (int)(t % (unsigned)tiles_y), b = (int)(t / (unsigned)tiles_y);
    const int x0 = tx * kTW, y0 = ty * kTH;
    const size_t plane = (size_t)H * W;
    const float *d = depth + (size_t)b * plane;
    for (int i = tid; i < (kTH + 2) * (kTW + 2); i += 256) {
        const int r = i / (kTW + 2), c = i - r * (kTW + 2);
        const int y = min(max(y0 - 1 + r, 0), H - 1), x = min(max(x0 - 1 + c, 0), W - 1);
        inv[r][c] = 1.f / d[(size_t)y * W + x];  // depth 0 -> +inf
    }
    __syncthreads();
    const float wx[9] = {-0.125f, 0.f, 0.125f, -0.25f, 0.f, 0.25f, -0.125f, 0.f, 0.125f};
    const float wy[9] = {-0.125f, -0.25f, -0.125f, 0.f, 0.f, 0.f, 0.125f, 0.25f, 0.125f};
    const int lx = tid & 63, x = x0 + lx;
    if (x >= W) return;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ly = (tid >> 6) + 4 * h, y = y0 + ly;
        if (y >= H) break;
        float gx = 0.f, gy = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float p = inv[ly + k / 3][lx + k % 3];
            if (k == 0) {
                gx = wx[0] * p, gy = wy[0] * p;
            } else {
                gx = gx + wx[k] * p, gy = gy + wy[k] * p;
            }
        }
        S[(size_t)b * plane + (size_t)y * W + x] = sqrtf((gx * gx + gy * gy) + 1e-6f);
    }
}

// ---- exact nanquantile ------------------------------------------------------------------------------------------------------------------
// Order-preserving key of a non-NaN float: negative values bit-flipped, the others with the sign bit set; +inf is the largest key.
__device__ __forceinline__ unsigned key_of(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// at::lerp (aten/src/ATen/native/Lerp.h) as torch.nanquantile applies it to the two order statistics
__device__ __forceinline__ float torch_lerp(float a, float b, float w) {
    const float diff = b - a;
    return w < 0.5f ? a + w * diff : b - diff * (1.f - w);
}

constexpr int kSelThreads = 1024, kSelUnroll = 8;

// One workgroup per image.  Pass p (p = 0 .. 3) histograms digit p (most significant first) of the keys that agree with the digits already
// fixed; the bin that holds rank k_lo fixes the next digit.  After four passes the key of rank k_lo is known together with the number of
// keys <= it; the order statistic k_hi = k_lo + 1 is the same key when that number exceeds k_hi, the smallest larger key otherwise (one more
// pass, an integer min).  Most values of a Sobel map share their leading digit: within a wave the lanes that agree with the first live lane
// are counted with a ballot and added by one lane (twice), the rest use one LDS integer atomic each.
__global__ __launch_bounds__(kSelThreads) void edge_select_k(const float *__restrict__ S, float *__restrict__ thr, int n_px, float q) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_k, s_dup, s_next, s_min;
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63;
    const float *s = S + (size_t)blockIdx.x * n_px;
    const int rounds = (n_px + kSelThreads * kSelUnroll - 1) / (kSelThreads * kSelUnroll);
    unsigned k_lo = 0, k_hi = 0;
    float weight = 0.f;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = pass ? s_prefix : 0u, fixed = pass ? 0xffffffffu << (shift + 8) : 0u;
        for (int r = 0; r < rounds; ++r) {
            float v[kSelUnroll];
#pragma unroll
            for (int u = 0; u < kSelUnroll; ++u) {
                const int i = (r * kSelUnroll + u) * kSelThreads + tid;
                v[u] = i < n_px ? s[i] : NAN;
            }
#pragma unroll
            for (int u = 0; u < kSelUnroll; ++u) {
                const unsigned key = key_of(v[u]);
                bool live = v[u] == v[u] && (key & fixed) == prefix;
                const unsigned d = (key >> shift) & 255u;
                unsigned long long todo = __ballot(live);
                for (int peel = 0; peel < 2 && todo; ++peel) {  // `todo` is the same in every lane of the wave
                    const int first = __ffsll((long long)todo) - 1;
                    const unsigned df = __shfl(d, first, 64);
                    const unsigned long long same = __ballot(live && d == df);
                    if (lane == first) atomicAdd(&hist[df], (unsigned)__popcll(same));
                    if (d == df) live = false;
                    todo &= ~same;
                }
                if (live) atomicAdd(&hist[d], 1u);
            }
        }
        __syncthreads();
        if (tid < 64) {  // wave 0: lane l owns bins 4 l .. 4 l + 3
            unsigned c[4], tot = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = hist[4 * lane + j], tot += c[j];
            unsigned inc = tot;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned up = __shfl_up(inc, off, 64);
                if (lane >= off) inc += up;
            }
            unsigned k;
            if (pass == 0) {
                // torch.nanquantile: rank = q * (n - 1) in fp32, clamped at 0; below = trunc, above = ceil, weight = rank - below
                const int n = (int)__shfl(inc, 63, 64);
                float rank = q * (float)(n - 1);
                rank = rank < 0.f ? 0.f : rank;
                unsigned lo = (unsigned)rank, hi = (unsigned)ceilf(rank);
                const unsigned last = n > 0 ? (unsigned)(n - 1) : 0u;
                lo = lo < last ? lo : last, hi = hi < last ? hi : last;
                if (lane == 0) s_n = n;
                k_lo = lo, k_hi = hi, weight = rank - (float)lo;
                k = lo;
            } else {
                k = s_k;
            }
            const unsigned exc = inc - tot;
            if (k >= exc && k < inc) {  // one lane (none when n == 0)
                unsigned r = k - exc;
                int j = 0;
                while (j < 3 && r >= c[j]) r -= c[j], ++j;
                s_prefix = prefix | ((unsigned)(4 * lane + j) << shift);
                s_k = r;
                s_dup = c[j];
            }
        }
        __syncthreads();
        if (s_n == 0) {  // nothing but NaN: sorted[0] is a NaN
            if (tid == 0) thr[blockIdx.x] = NAN;
            return;
        }
    }
    // wave 0 still holds k_lo, k_hi and weight; s_prefix is the key of rank k_lo, s_k its index among the s_dup equal keys, so k_lo - s_k keys
    // are smaller
    const unsigned key_lo = s_prefix;
    if (tid == 0) {
        const unsigned count_le = (k_lo - s_k) + s_dup;
        s_next = k_hi >= count_le;
        s_min = 0xffffffffu;
    }
    __syncthreads();
    const bool need_next = s_next != 0;
    if (need_next) {  // the smallest key above key_lo: it exists, because k_hi <= n - 1
        unsigned m = 0xffffffffu;
#pragma unroll 8
        for (int i = tid; i < n_px; i += kSelThreads) {
            const float v = s[i];
            const unsigned key = key_of(v);
            if (v == v && key > key_lo && key < m) m = key;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned o = __shfl_down(m, off, 64);
            m = o < m ? o : m;
        }
        if (lane == 0) atomicMin(&s_min, m);
        __syncthreads();
    }
    if (tid == 0) {
        const float v_lo = value_of(key_lo), v_hi = need_next ? value_of(s_min) : v_lo;
        thr[blockIdx.x] = torch_lerp(v_lo, v_hi, weight);
    }
}

// ---- S > threshold, 5x5 OR --------------------------------------------------------------------------------------------------------------
template <bool DILATE, typename T>
__global__ __launch_bounds__(256) void edge_mask_k(const float *__restrict__ S, const float *__restrict__ thr, T *__restrict__ mask, int H, int W,
                                                   int tiles_x, int tiles_y) {
    constexpr int R = DILATE ? 2 : 0, PH = kTH + 2 * R, PW = kTW + 2 * R;
    __shared__ unsigned char edge[PH][PW];
    const int tid = threadIdx.x;
    unsigned t = blockIdx.x;
    const int tx = (int)(t % (unsigned)tiles_x);
    t /= (unsigned)tiles_x;
    const int ty = (int)(t % (unsigned)tiles_y), b = (int)(t / (unsigned)tiles_y);
    const int x0 = tx * kTW, y0 = ty * kTH;
    const size_t plane = (size_t)H * W;
    const float *s = S + (size_t)b * plane;
    const float th = thr[b];
    for (int i = tid; i < PH * PW; i += 256) {
        const int r = i / PW, c = i - r * PW;
        const int y = y0 - R + r, x = x0 - R + c;
        unsigned char e = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) e = s[(size_t)y * W + x] > th;  // a NaN on either side: 0
        edge[r][c] = e;
    }
    __syncthreads();
    const int lx = tid & 63, x = x0 + lx;
    if (x >= W) return;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ly = (tid >> 6) + 4 * h, y = y0 + ly;
        if (y >= H) break;
        unsigned e = 0;
#pragma unroll
        for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
            for (int dx = 0; dx <= 2 * R; ++dx) e |= edge[ly + dy][lx + dx];
        mask[(size_t)b * plane + (size_t)y * W + x] = (T)e;
    }
}

// ---- validation losses ------------------------------------------------------------------------------------------------------------------
constexpr int kChunk = 2048;  // elements per partial: 8 per lane.  The partials depend on the problem alone, never on the grid

struct LossArgs {
    const float *pred, *rendered, *depth, *edge;
    double *part;  // (chunks, 4): sum bce, sum reg, count mask, count reg_mask
    unsigned total, per_map, hw;  // B * D * hw, D * hw, h * w
    int chunks;
    float pos_weight;
};

// Which elements count is decided on the fp32 inputs; the two terms are evaluated in fp64 from the fp32 logit, so that the value returned is
// the fp64 mean rounded once.  With e = exp(-|x|): BCEWithLogits = (1 - t) x + (1 + (pos_weight - 1) t) (log1p(e) + max(-x, 0)), and
// 2 (0.5 - |sigmoid(x) - 0.5|) = 2 e / (1 + e).
__global__ __launch_bounds__(256) void bd_val_partial_k(const LossArgs a) {
    __shared__ double sh[4][4];
    const int t = threadIdx.x;
    for (int chunk = blockIdx.x; chunk < a.chunks; chunk += gridDim.x) {
        double bce = 0.0, reg = 0.0;
        int nm = 0, nr = 0;
#pragma unroll
        for (int u = 0; u < kChunk / 256; ++u) {
            const long long i = (long long)chunk * kChunk + u * 256 + t;
            if (i < (long long)a.total) {
                const unsigned b = (unsigned)i / a.per_map;
                const size_t px = (size_t)b * a.hw + ((unsigned)i - b * a.per_map) % a.hw;
                const float x = a.pred[i], r = a.rendered[i], d = a.depth[px];
                const bool m = d > 0.f && r > 0.f;
                bool rm = m;
                if (a.edge) rm = m && a.edge[px] != 0.f;
                if (m) {
                    const double xd = (double)x, e = exp(-fabs(xd));
                    const double soft = log1p(e) + (xd < 0.0 ? -xd : 0.0);
                    const bool tgt = r < d;
                    bce += tgt ? (double)a.pos_weight * soft : xd + soft;
                    ++nm;
                    if (rm) reg += 2.0 * e / (1.0 + e), ++nr;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            bce += __shfl_down(bce, off, 64), reg += __shfl_down(reg, off, 64);
            nm += __shfl_down(nm, off, 64), nr += __shfl_down(nr, off, 64);
        }
        if ((t & 63) == 0) sh[0][t >> 6] = bce, sh[1][t >> 6] = reg, sh[2][t >> 6] = (double)nm, sh[3][t >> 6] = (double)nr;
        __syncthreads();
        if (t < 4) a.part[(size_t)chunk * 4 + t] = ((sh[t][0] + sh[t][1]) + sh[t][2]) + sh[t][3];
        __syncthreads();
    }
}

// thread t adds partials t, t + 256, ...; the 256 sums are folded pairwise through LDS: one order, whatever the launch.
// out: count(mask), count(reg_mask), binary_loss/0, reg_loss/0, the total (bd_model.py:484-494 in fp32 on the two fp32 means).
__global__ __launch_bounds__(256) void bd_val_finalise_k(const double *__restrict__ part, int chunks, float reg_weight, double *__restrict__ out) {
    __shared__ double sS[4][256];
    const int t = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = t; i < chunks; i += 256)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += part[(size_t)i * 4 + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) sS[j][t] = s[j];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off)
#pragma unroll
            for (int j = 0; j < 4; ++j) sS[j][t] += sS[j][t + off];
        __syncthreads();
    }
    if (t == 0) {
        const double nm = sS[2][0], nr = sS[3][0];
        const float bl = (float)(sS[0][0] / nm), rl = (float)(sS[1][0] / nr);  // 0 / 0: NaN, the mean of nothing
        float total = 0.f;  // an empty mask: the reference's edge case, |pred - pred|.mean() = 0
        if (nm > 0.0) {
            total = bl;
            if (reg_weight > 0.f) total = total + rl * reg_weight;
        }
        out[0] = nm, out[1] = nr, out[2] = (double)bl, out[3] = (double)rl, out[4] = (double)total;
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t idh_sizeof_edge_mask_args(void) { return sizeof(idh_edge_mask_args); }
extern "C" size_t idh_sizeof_bd_val_losses_args(void) { return sizeof(idh_bd_val_losses_args); }

extern "C" size_t idh_edge_mask_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return align256((size_t)4 * B * H * W) + align256((size_t)4 * B);
}

extern "C" int idh_edge_mask_fwd(const idh_edge_mask_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_edge_mask_args)) return IDH_EINVAL;
    const idh_edge_mask_args &e = *args;
    if (!e.depth_b1hw || !e.mask_b1hw) return IDH_EINVAL;
    if (e.B < 0 || e.H < 1 || e.W < 1) return IDH_EINVAL;
    if (!(e.q >= 0.f && e.q <= 1.f)) return IDH_EINVAL;  // (a NaN fails both)
    if ((uintptr_t)e.workspace & 3u) return IDH_EINVAL;
    const long long n_px = (long long)e.H * e.W;
    const long long tiles_x = idh_cdiv(e.W, kTW), tiles_y = idh_cdiv(e.H, kTH);
    // q * (n - 1) is formed in fp32: the ranks are exact up to 2^24 pixels per image
    if (n_px > (1ll << 24) || tiles_x * tiles_y * e.B >= (1ll << 31)) return IDH_EUNSUPPORTED;
    if (e.B == 0) return IDH_OK;
    if (!e.workspace || e.workspace_bytes < (int64_t)idh_edge_mask_workspace_bytes(e.B, e.H, e.W)) return IDH_EWORKSPACE;
    float *S = e.sobel_b1hw ? e.sobel_b1hw : static_cast<float *>(e.workspace);
    float *thr = e.threshold_b ? e.threshold_b
                               : reinterpret_cast<float *>(static_cast<char *>(e.workspace) + align256((size_t)4 * e.B * e.H * e.W));
    hipStream_t st = idh_stream(stream);
    const unsigned blocks = (unsigned)(tiles_x * tiles_y * e.B);
    hipLaunchKernelGGL(edge_sobel_k, dim3(blocks), dim3(256), 0, st, e.depth_b1hw, S, e.H, e.W, (int)tiles_x, (int)tiles_y);
    IDH_CHECK_LAUNCH();
    hipLaunchKernelGGL(edge_select_k, dim3(e.B), dim3(kSelThreads), 0, st, S, thr, (int)n_px, e.q);
    IDH_CHECK_LAUNCH();
    const int tx = (int)tiles_x, ty = (int)tiles_y;
    if (e.mask_u8) {
        uint8_t *m = static_cast<uint8_t *>(e.mask_b1hw);
        if (e.dilate) hipLaunchKernelGGL((edge_mask_k<true, uint8_t>), dim3(blocks), dim3(256), 0, st, S, thr, m, e.H, e.W, tx, ty);
        else hipLaunchKernelGGL((edge_mask_k<false, uint8_t>), dim3(blocks), dim3(256), 0, st, S, thr, m, e.H, e.W, tx, ty);
    } else {
        float *m = static_cast<float *>(e.mask_b1hw);
        if (e.dilate) hipLaunchKernelGGL((edge_mask_k<true, float>), dim3(blocks), dim3(256), 0, st, S, thr, m, e.H, e.W, tx, ty);
        else hipLaunchKernelGGL((edge_mask_k<false, float>), dim3(blocks), dim3(256), 0, st, S, thr, m, e.H, e.W, tx, ty);
    }
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" size_t idh_bd_val_losses_workspace_bytes(int B, int D, int h, int w) {
    if (B <= 0 || D <= 0 || h <= 0 || w <= 0) return 0;
    const long long total = (long long)B * D * h * w;
    return (size_t)32 * (size_t)((total + kChunk - 1) / kChunk);
}

extern "C" int idh_bd_val_losses_fwd(const idh_bd_val_losses_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_bd_val_losses_args)) return IDH_EINVAL;
    const idh_bd_val_losses_args &e = *args;
    if (!e.pred_bdhw || !e.rendered_bdhw || !e.depth_b1hw || !e.out5) return IDH_EINVAL;
    if (e.B < 1 || e.D < 1 || e.h < 1 || e.w < 1 || e.max_workgroups < 0) return IDH_EINVAL;
    if (!(e.bd_regularisation_weight == e.bd_regularisation_weight) || !(e.positive_weight == e.positive_weight)) return IDH_EINVAL;
    if (((uintptr_t)e.workspace & 7u) || ((uintptr_t)e.out5 & 7u)) return IDH_EINVAL;
    const long long total = (long long)e.B * e.D * e.h * e.w, chunks = (total + kChunk - 1) / kChunk;
    if (total >= (1ll << 31)) return IDH_EUNSUPPORTED;
    if (!e.workspace || e.workspace_bytes < (int64_t)idh_bd_val_losses_workspace_bytes(e.B, e.D, e.h, e.w)) return IDH_EWORKSPACE;
    LossArgs a;
    a.pred = e.pred_bdhw, a.rendered = e.rendered_bdhw, a.depth = e.depth_b1hw, a.edge = e.edge_mask_b1hw;
    a.part = static_cast<double *>(e.workspace);
    a.total = (unsigned)total, a.per_map = (unsigned)((long long)e.D * e.h * e.w), a.hw = (unsigned)(e.h * e.w), a.chunks = (int)chunks;
    a.pos_weight = e.positive_weight;
    const long long cap = e.max_workgroups > 0 ? e.max_workgroups : 2048;
    hipStream_t st = idh_stream(stream);
    hipLaunchKernelGGL(bd_val_partial_k, dim3((unsigned)(chunks < cap ? chunks : cap)), dim3(256), 0, st, a);
    IDH_CHECK_LAUNCH();
    hipLaunchKernelGGL(bd_val_finalise_k, dim3(1), dim3(256), 0, st, a.part, a.chunks, e.bd_regularisation_weight, e.out5);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
