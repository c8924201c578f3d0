// DepthModel's validation losses (include/idh_geometry.h): the forward value of DepthModel.compute_losses
// (experiment_modules/depth_model.py:442-540).
//
//   reg_level_k<T>   one launch per pyramid level of MSGradientLoss (losses.py:77-101): a workgroup owns 32 x 32 tiles of the level of one
//                    image, stages both maps with a one-pixel halo in LDS, accumulates sum |g_pred - g_gt| and the element count of the
//                    tile and writes its 16 x 16 tile of blur_pool2d of both maps, the next level.  T = float at level 0 (the caller's
//                    maps), double afterwards (the workspace).  Level 0's launch also evaluates the point-wise terms and the normals.
//   reg_finalise_k   one workgroup that adds the tile records in tile order and writes the sixteen outputs.
//
// Built with -ffp-contract=off and without any fast-math flag.  Which elements count is decided as the header says; the values are
// evaluated in fp64 from the fp32 inputs.  One record per tile, not per workgroup; a tile's 256 lane sums are folded through LDS, sixteen
// neighbours at a time, in a fixed order; no floating-point atomics: the same bits for every grid and every run.
#include "idh_common.h"

#include "../../include/idh_geometry.h"

#include <math.h>

namespace {

constexpr int kT = 32;      // tile edge at the level that is read; the tile of the next level is kT / 2
constexpr int kRec0 = 16;   // doubles of workspace per tile of level 0 (kNV used), 2 at the levels above
constexpr int kNV = 14;
// fields of a level-0 record
enum { F_GRAD = 0, F_GRAD_N, F_MS0, F_MS1, F_MS2, F_MS3, F_ABS, F_D, F_D2, F_MASK_N, F_INV, F_LIMIT_N, F_NRM, F_NRM_N };
constexpr int kSums = kNV + 2 * 3;  // what the finalise adds: a level-0 record and (sum, count) of levels 1 .. 3

struct LevelArgs {
    const void *gt, *pred;     // (B,H,W) of this level: float at level 0, double above
    double *gt_out, *pred_out; // (B,ceil(H/2),ceil(W/2)) the next level, or NULL
    double *part;              // (nv, ntiles): field-major, so that the finalise reads along tiles
    const uint8_t *mask;       // point-wise terms (level 0)
    const float *logp[4];
    const float *n_gt, *n_pred;
    int ry[4], rx[4], sw[4];   // per present scale: h / scale_h, w / scale_w, scale_w
    int H, W, tiles_x, tiles_y, ntiles, nv;
    int grad, point, normals;
    int vec;                   // rows and bases are 16-byte aligned: a lane's four pixels are one vector load per map
};

constexpr int kRedRow = 256 + 16;
constexpr int kLS = kT + 3;  // LDS row stride in doubles: with 35 the four rows a half-wave reads start 6 banks apart (34: rows 0 and 2 collide)

template <typename T>
struct Vec4;
template <>
struct Vec4<float> {
    static __device__ __forceinline__ void load(const float *p, float v[4]) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    }
};
template <>
struct Vec4<double> {
    static __device__ __forceinline__ void load(const double *p, double v[4]) {
        const double2 q0 = *reinterpret_cast<const double2 *>(p), q1 = *reinterpret_cast<const double2 *>(p + 2);
        v[0] = q0.x, v[1] = q0.y, v[2] = q1.x, v[3] = q1.y;
    }
};

// four pixels of one row: a vector load where the caller says so, else positions clamped into the image (the replicate border)
template <typename T>
__device__ __forceinline__ void load4(const T *m, int y, int x, int H, int W, bool vec, T v[4]) {
    if (vec) {
        Vec4<T>::load(m + (size_t)y * W + x, v);
    } else {
        const T *row = m + (size_t)min(y, H - 1) * W;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = row[min(x + j, W - 1)];
    }
}

// the Sobel pair at four neighbouring pixels from their 3 x 6 window in LDS; every tap, the zero ones too: 0 * NaN = 0 * inf = NaN
__device__ __forceinline__ void sobel4(const double (*m)[kLS], int ly, int lx0, double gx[4], double gy[4]) {
    const double wx[9] = {-0.125, 0.0, 0.125, -0.25, 0.0, 0.25, -0.125, 0.0, 0.125};
    const double wy[9] = {-0.125, -0.25, -0.125, 0.0, 0.0, 0.0, 0.125, 0.25, 0.125};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        double c[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] = m[ly + dy][lx0 + k];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int k = dy * 3 + dx;
                if (k == 0) {
                    gx[j] = wx[0] * c[j], gy[j] = wy[0] * c[j];
                } else {
                    gx[j] = gx[j] + wx[k] * c[j + dx], gy[j] = gy[j] + wy[k] * c[j + dx];
                }
            }
    }
}

// A lane owns four neighbouring pixels of one row of the tile: lane t row t / 8, columns 4 (t % 8) .. + 3.
template <typename T>
__global__ __launch_bounds__(256) void reg_level_k(const LevelArgs a) {
    // the staged maps, and after the tile has been consumed the lanes' sums in the same memory: lane i of field j at red[j][i + i / 16],
    // so that 16 lanes adding 16 neighbours each, and 256 lanes storing, touch every bank once
    __shared__ double smem[kNV * kRedRow + kNV * 16];
    double(*tile)[kT + 2][kLS] = reinterpret_cast<double(*)[kT + 2][kLS]>(smem);
    double(*red)[kRedRow] = reinterpret_cast<double(*)[kRedRow]>(smem);
    double(*red16)[16] = reinterpret_cast<double(*)[16]>(smem + kNV * kRedRow);
    static_assert(2 * (kT + 2) * kLS <= kNV * kRedRow, "the tile must fit under the sums");
    const int tid = threadIdx.x, ly = tid >> 3, lx0 = (tid & 7) * 4;
    const size_t plane = (size_t)a.H * a.W;
    const double wb[9] = {0.0625, 0.125, 0.0625, 0.125, 0.25, 0.125, 0.0625, 0.125, 0.0625};
    for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int tx = t % a.tiles_x, rest = t / a.tiles_x;
        const int ty = rest % a.tiles_y, b = rest / a.tiles_y;
        const int x0 = tx * kT, y0 = ty * kT, x = x0 + lx0, y = y0 + ly;
        const T *g = static_cast<const T *>(a.gt) + (size_t)b * plane, *p = static_cast<const T *>(a.pred) + (size_t)b * plane;
        const bool inside = y < a.H && x + 3 < a.W, vec = a.vec && inside;
        double v[kNV];
#pragma unroll
        for (int j = 0; j < kNV; ++j) v[j] = 0.0;
        T g4[4] = {0, 0, 0, 0}, p4[4] = {0, 0, 0, 0};
        if (a.grad || a.point) load4(g, y, x, a.H, a.W, vec, g4), load4(p, y, x, a.H, a.W, vec, p4);
        if (a.grad) {
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[0][ly + 1][lx0 + 1 + j] = (double)g4[j], tile[1][ly + 1][lx0 + 1 + j] = (double)p4[j];
            if (tid < 4 * kT + 4) {  // the one-pixel ring: top and bottom rows with the corners, then the two columns
                const int r = tid < 2 * (kT + 2) ? (tid < kT + 2 ? 0 : kT + 1) : 1 + (tid - 2 * (kT + 2)) % kT;
                const int c = tid < 2 * (kT + 2) ? tid % (kT + 2) : (tid < 3 * kT + 4 ? 0 : kT + 1);
                const int yy = min(max(y0 - 1 + r, 0), a.H - 1), xx = min(max(x0 - 1 + c, 0), a.W - 1);
                tile[0][r][c] = (double)g[(size_t)yy * a.W + xx];
                tile[1][r][c] = (double)p[(size_t)yy * a.W + xx];
            }
            __syncthreads();
            if (y < a.H && x < a.W) {
                double ggx[4], ggy[4], gpx[4], gpy[4];
                sobel4(tile[0], ly, lx0, ggx, ggy);
                sobel4(tile[1], ly, lx0, gpx, gpy);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < a.W) {
                        if (isfinite(ggx[j])) v[F_GRAD] += fabs(gpx[j] - ggx[j]), v[F_GRAD_N] += 1.0;
                        if (isfinite(ggy[j])) v[F_GRAD] += fabs(gpy[j] - ggy[j]), v[F_GRAD_N] += 1.0;
                    }
            }
        }
        if ((a.point || a.normals) && y < a.H && x < a.W) {  // level 0: T is float
            const size_t px = (size_t)b * plane + (size_t)y * a.W + x;
            if (a.point) {
                uint8_t m4[4];
                float l0[4];
                if (vec) {
                    const uchar4 q = *reinterpret_cast<const uchar4 *>(a.mask + px);
                    m4[0] = q.x, m4[1] = q.y, m4[2] = q.z, m4[3] = q.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) m4[j] = x + j < a.W ? a.mask[px + j] : 0;
                }
                const bool vec0 = vec && a.rx[0] == 1 && a.ry[0] == 1;
                if (vec0) Vec4<float>::load(a.logp[0] + px, l0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!m4[j]) continue;
                    const float pr32 = (float)p4[j];
                    const double gt = (double)g4[j], pr = (double)p4[j], lg = log(gt);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (a.logp[i]) {
                            float lp;
                            if (i == 0 && vec0) {
                                lp = l0[j];
                            } else {
                                const int sy = y / a.ry[i], sx = (x + j) / a.rx[i];
                                lp = a.logp[i][((size_t)b * (a.H / a.ry[i]) + sy) * a.sw[i] + sx];
                            }
                            const double d = lg - (double)lp;
                            v[F_MS0 + i] += fabs(d);
                            if (i == 0) v[F_D] += d, v[F_D2] += d * d;
                        }
                    v[F_ABS] += fabs(gt - pr);
                    v[F_MASK_N] += 1.0;
                    if (pr32 > 0.1f) v[F_INV] += fabs(1.0 / gt - 1.0 / pr), v[F_LIMIT_N] += 1.0;
                }
            }
            if (a.normals) {
                float n[6][4];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    load4(a.n_gt + ((size_t)b * 3 + c) * plane, y, x, a.H, a.W, vec, n[c]);
                    load4(a.n_pred + ((size_t)b * 3 + c) * plane, y, x, a.H, a.W, vec, n[3 + c]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < a.W && isfinite(n[0][j]) && isfinite(n[1][j]) && isfinite(n[2][j]) && isfinite(n[3][j]) && isfinite(n[4][j]) && isfinite(n[5][j])) {
                        const double dot = ((double)n[3][j] * (double)n[0][j] + (double)n[4][j] * (double)n[1][j]) + (double)n[5][j] * (double)n[2][j];
                        v[F_NRM] += 0.5 * (1.0 - dot), v[F_NRM_N] += 1.0;
                    }
            }
        }
        if (a.gt_out) {  // blur_pool2d: zero padding, so a tap outside the image adds nothing (the LDS halo there holds the replicated border)
            const int oy = tid >> 4, ox = tid & 15;
            const int Hn = (a.H + 1) >> 1, Wn = (a.W + 1) >> 1;
            const int Y = (y0 >> 1) + oy, X = (x0 >> 1) + ox;
            if (Y < Hn && X < Wn) {
                double sg = 0.0, sp = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const int r = 2 * oy + k / 3, c = 2 * ox + k % 3;  // LDS position of image (y0 - 1 + r, x0 - 1 + c)
                    const int yy = y0 - 1 + r, xx = x0 - 1 + c;
                    if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) sg = sg + wb[k] * tile[0][r][c], sp = sp + wb[k] * tile[1][r][c];
                }
                const size_t o = ((size_t)b * Hn + Y) * Wn + X;
                a.gt_out[o] = sg, a.pred_out[o] = sp;
            }
        }
        __syncthreads();  // every lane is done with `tile`
#pragma unroll
        for (int j = 0; j < kNV; ++j)
            if (j < a.nv) red[j][tid + (tid >> 4)] = v[j];  // (uniform)
        __syncthreads();
        if (tid < 16 * a.nv) {  // lane (j, s) adds lanes 16 s .. 16 s + 15 of field j, in that order
            const int j = tid >> 4, s16 = tid & 15;
            double sum = red[j][17 * s16];
#pragma unroll
            for (int k = 1; k < 16; ++k) sum += red[j][17 * s16 + k];
            red16[j][s16] = sum;
        }
        __syncthreads();
        if (tid < a.nv) {
            double sum = red16[tid][0];
#pragma unroll
            for (int k = 1; k < 16; ++k) sum += red16[tid][k];
            a.part[(size_t)tid * a.ntiles + t] = sum;
        }
        __syncthreads();  // `tile` and `red` are written again by the next tile
    }
}

struct FinalArgs {
    const double *part[4];
    const float *mv;
    double *out;
    int ntiles[4];
    int levels;  // launches that left records: 0 .. 4
    int grad_levels, point, normals, hypersim, present[4];
    float si_lambda;
};

// thread t adds records t, t + 256, ...; the 256 sums are folded pairwise through LDS: one order, whatever the launches were.
__global__ __launch_bounds__(256) void reg_finalise_k(const FinalArgs a) {
    __shared__ double sS[kSums][256];
    const int t = threadIdx.x;
    double s[kSums];
#pragma unroll
    for (int j = 0; j < kSums; ++j) s[j] = 0.0;
    if (a.levels > 0)
        for (int i = t; i < a.ntiles[0]; i += 256)
#pragma unroll
            for (int j = 0; j < kNV; ++j) s[j] += a.part[0][(size_t)j * a.ntiles[0] + i];
#pragma unroll
    for (int l = 1; l < 4; ++l)
        if (l < a.levels)
            for (int i = t; i < a.ntiles[l]; i += 256) s[kNV + 2 * (l - 1)] += a.part[l][i], s[kNV + 2 * (l - 1) + 1] += a.part[l][(size_t)a.ntiles[l] + i];
#pragma unroll
    for (int j = 0; j < kSums; ++j) sS[j][t] = s[j];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off)
#pragma unroll
            for (int j = 0; j < kSums; ++j) sS[j][t] += sS[j][t + off];
        __syncthreads();
    }
    if (t != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double cnt[7] = {0, 0, 0, 0, 0, 0, 0};
    float grad = __double2float_rn(nan), nrm = grad, ms = grad, ab = grad, l1 = grad, si = grad, inv = grad;
    if (a.hypersim) {
        grad = 0.f, nrm = 0.f;
    } else {
        if (a.grad_levels > 0) {  // 0 / 0: NaN, the mean of nothing
            double gsum = 0.0;
            for (int l = 0; l < a.grad_levels; ++l) {
                const double sum = l ? sS[kNV + 2 * (l - 1)][0] : sS[F_GRAD][0], n = l ? sS[kNV + 2 * (l - 1) + 1][0] : sS[F_GRAD_N][0];
                gsum += sum / n, cnt[l] = n;
            }
            grad = (float)gsum;
        }
        if (a.normals) nrm = (float)(sS[F_NRM][0] / sS[F_NRM_N][0]), cnt[6] = sS[F_NRM_N][0];
    }
    if (a.point) {
        const double n = sS[F_MASK_N][0];
        double m = 0.0, scale = 1.0;
        for (int i = 0; i < 4; ++i, scale *= 0.5)
            if (a.present[i]) m += sS[F_MS0 + i][0] / n * scale;
        const double md = sS[F_D][0] / n;
        ms = (float)m, ab = (float)(sS[F_ABS][0] / n), l1 = (float)(sS[F_MS0][0] / n);
        si = (float)sqrt(sS[F_D2][0] / n - (double)a.si_lambda * (md * md));
        inv = (float)(sS[F_INV][0] / sS[F_LIMIT_N][0]);
        cnt[4] = n, cnt[5] = sS[F_LIMIT_N][0];
    }
    const float mv = a.hypersim ? 0.f : (a.mv ? *a.mv : 0.f);
    const float loss = ((ms + grad) + nrm) + 0.2f * mv;  // depth_model.py:527 on the fp32 values
    const float vals[9] = {loss, si, grad, ab, nrm, ms, inv, l1, mv};
    for (int i = 0; i < 9; ++i) a.out[i] = (double)vals[i];
    for (int i = 0; i < 7; ++i) a.out[9 + i] = cnt[i];
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// sizes of level l and the byte offsets of the workspace: [gt_1, pred_1, gt_2, pred_2, gt_3, pred_3, records 0 .. 3]
struct Layout {
    int H[4], W[4];
    long long tiles[4];
    size_t map[4], part[4], bytes;
};

Layout layout_of(int B, int h, int w) {
    Layout L;
    size_t off = 0;
    for (int l = 0; l < 4; ++l) {
        L.H[l] = l ? (L.H[l - 1] + 1) / 2 : h, L.W[l] = l ? (L.W[l - 1] + 1) / 2 : w;
        L.tiles[l] = (long long)B * idh_cdiv(L.H[l], kT) * idh_cdiv(L.W[l], kT);
        L.map[l] = off;
        if (l) off += 2 * align256((size_t)8 * B * L.H[l] * L.W[l]);
    }
    for (int l = 0; l < 4; ++l) L.part[l] = off, off += align256((size_t)8 * (l ? 2 : kRec0) * (size_t)L.tiles[l]);
    L.bytes = off;
    return L;
}

}  // namespace

extern "C" size_t idh_sizeof_reg_val_losses_args(void) { return sizeof(idh_reg_val_losses_args); }

extern "C" size_t idh_reg_val_losses_workspace_bytes(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0 || (long long)B * h * w >= (1ll << 31)) return 0;
    return layout_of(B, h, w).bytes;
}

extern "C" int idh_reg_val_losses_fwd(const idh_reg_val_losses_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_reg_val_losses_args)) return IDH_EINVAL;
    const idh_reg_val_losses_args &e = *args;
    if (!e.out16 || e.B < 0 || e.h < 1 || e.w < 1 || e.max_workgroups < 0) return IDH_EINVAL;
    if (e.num_scales < 0 || e.num_scales > 4 || (e.terms & ~IDH_REG_TERM_ALL) || !(e.si_lambda == e.si_lambda)) return IDH_EINVAL;
    const int terms = e.terms ? e.terms : IDH_REG_TERM_ALL;
    const bool point = terms & IDH_REG_TERM_POINT, grad = (terms & IDH_REG_TERM_GRAD) && !e.hypersim;
    const bool normals = (terms & IDH_REG_TERM_NORMALS) && !e.hypersim;
    if ((point || grad) && (!e.depth_gt_b1hw || !e.depth_pred_b1hw)) return IDH_EINVAL;
    if (normals && (!e.normals_gt_b3hw || !e.normals_pred_b3hw)) return IDH_EINVAL;
    if (point) {
        if (!e.mask_b_b1hw || !e.log_depth_pred_s[0]) return IDH_EINVAL;
        for (int i = 0; i < 4; ++i)
            if (e.log_depth_pred_s[i] && (e.scale_h[i] < 1 || e.scale_w[i] < 1 || e.h % e.scale_h[i] || e.w % e.scale_w[i])) return IDH_EINVAL;
    }
    if (((uintptr_t)e.workspace & 7u) || ((uintptr_t)e.out16 & 7u)) return IDH_EINVAL;
    if ((long long)e.B * e.h * e.w >= (1ll << 31)) return IDH_EUNSUPPORTED;
    if (e.B == 0) return IDH_OK;
    const Layout L = layout_of(e.B, e.h, e.w);
    if (!e.workspace || e.workspace_bytes < (int64_t)L.bytes) return IDH_EWORKSPACE;
    char *ws = static_cast<char *>(e.workspace);
    const int grad_levels = grad ? (e.num_scales ? e.num_scales : 4) : 0;
    const int levels = grad ? grad_levels : ((point || normals) ? 1 : 0);
    const long long cap = e.max_workgroups > 0 ? e.max_workgroups : 4096;
    hipStream_t st = idh_stream(stream);
    FinalArgs f = {};
    for (int l = 0; l < levels; ++l) {
        LevelArgs a = {};
        const size_t map_bytes = align256((size_t)8 * e.B * L.H[l] * L.W[l]);
        a.gt = l ? static_cast<const void *>(ws + L.map[l]) : e.depth_gt_b1hw;
        a.pred = l ? static_cast<const void *>(ws + L.map[l] + map_bytes) : e.depth_pred_b1hw;
        if (l + 1 < grad_levels) {
            a.gt_out = reinterpret_cast<double *>(ws + L.map[l + 1]);
            a.pred_out = reinterpret_cast<double *>(ws + L.map[l + 1] + align256((size_t)8 * e.B * L.H[l + 1] * L.W[l + 1]));
        }
        a.part = reinterpret_cast<double *>(ws + L.part[l]);
        a.H = L.H[l], a.W = L.W[l], a.tiles_x = idh_cdiv(a.W, kT), a.tiles_y = idh_cdiv(a.H, kT), a.ntiles = (int)L.tiles[l];
        a.nv = l ? 2 : kNV;
        a.grad = grad;
        if (l == 0) {
            a.point = point, a.normals = normals;
            a.mask = point ? e.mask_b_b1hw : nullptr;
            a.n_gt = normals ? e.normals_gt_b3hw : nullptr, a.n_pred = normals ? e.normals_pred_b3hw : nullptr;
            for (int i = 0; i < 4 && point; ++i)
                if (e.log_depth_pred_s[i]) a.logp[i] = e.log_depth_pred_s[i], a.ry[i] = e.h / e.scale_h[i], a.rx[i] = e.w / e.scale_w[i], a.sw[i] = e.scale_w[i];
        }
        uintptr_t bits = (uintptr_t)a.gt | (uintptr_t)a.pred | (uintptr_t)a.mask | (uintptr_t)a.n_gt | (uintptr_t)a.n_pred | (uintptr_t)a.logp[0];
        a.vec = a.W % 4 == 0 && bits % 16 == 0;  // (a NULL adds no bit; the planes of one tensor are then 16-byte multiples apart)
        const unsigned blocks = (unsigned)(L.tiles[l] < cap ? L.tiles[l] : cap);
        if (l == 0) hipLaunchKernelGGL(reg_level_k<float>, dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(reg_level_k<double>, dim3(blocks), dim3(256), 0, st, a);
        IDH_CHECK_LAUNCH();
        f.part[l] = a.part, f.ntiles[l] = a.ntiles;
    }
    f.mv = e.mv_loss, f.out = e.out16, f.levels = levels, f.grad_levels = grad_levels, f.point = point, f.normals = normals;
    f.hypersim = e.hypersim != 0, f.si_lambda = e.si_lambda;
    for (int i = 0; i < 4; ++i) f.present[i] = point && e.log_depth_pred_s[i];
    hipLaunchKernelGGL(reg_finalise_k, dim3(1), dim3(256), 0, st, f);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
