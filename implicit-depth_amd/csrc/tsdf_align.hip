// TSDF pose alignment (include/idh_fusion.h): Gauss-Newton of a depth map's camera on the fused signed distance field.
// The header states the arithmetic; this file follows it expression by expression.
//
//   tsdf_align_rows_k<FIRST, ROWS, WEIGHT>  one lane per selected pixel, a 16 x 16 chunk of them per workgroup pass, an 8 x 8 quarter per
//                     wave (the ray cast's tile).  The pixel's row (J, r, wgt) in fp32 from four 16-byte corner loads, its 29 fp64 products
//                     summed over the wave by shuffles, over the four waves through LDS, one record per chunk.  FIRST reads the caller's
//                     pose, the later iterations the fp64 state rounded to fp32; ROWS also stores the rows (iteration 0 only).
//   tsdf_align_solve_k<FIRST>  one workgroup: the records added in a fixed order, then one lane solves the 6 x 6 system in fp64 (the
//                     matrix lives in LDS: no dynamically indexed registers), updates the pose and writes the iteration's record.
//
// Nothing here depends on the grid: a chunk's record is a function of the chunk, the solve's order a function of the chunk count.
#include "tsdf_common.h"

namespace {

constexpr int kSums = 29;     // 21 A + 6 b + cost + count
constexpr int kRecord = 32;   // doubles per chunk record (kSums, padded)
constexpr int kState = 16;    // doubles in front of the records: R (9, row-major), t (3), stopped flag, 3 spare
constexpr int kSlots = 8;     // partial sums of the solve: record c goes to slot c % 8

struct AlignArgs {
    Vol V;
    const float *depth, *invK, *weight, *pose_in;
    float *pose_out, *rows;
    double *state, *records;  // records: this iteration's 40 doubles
    double damping, min_step, min_pivot_ratio;
    float trunc_voxels, huber;
    int h, w, hs, ws, cx, chunks, stride, min_count;
};

template <bool FIRST, bool ROWS, bool WEIGHT>
__global__ __launch_bounds__(256) void tsdf_align_rows_k(const AlignArgs a) {
    __shared__ double sh[kSums][4];
    const double *st = a.state;
    if (!FIRST && st[12] != 0.0) return;  // converged or failed: uniform over the grid
    const Vol &V = a.V;
    float R[9], t[3];
    if (FIRST) {
#pragma unroll
        for (int k = 0; k < 3; ++k) R[3 * k] = a.pose_in[4 * k], R[3 * k + 1] = a.pose_in[4 * k + 1], R[3 * k + 2] = a.pose_in[4 * k + 2], t[k] = a.pose_in[4 * k + 3];
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = (float)st[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = (float)st[9 + k];
    }
    const float *iK = a.invK;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int chunk = blockIdx.x; chunk < a.chunks; chunk += gridDim.x) {
        const int cy = chunk / a.cx, cxi = chunk - cy * a.cx;
        const int sj = cxi * 16 + (wave & 1) * 8 + (lane & 7), si = cy * 16 + (wave >> 1) * 8 + (lane >> 3);
        const bool live = si < a.hs && sj < a.ws;
        float J[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, r = 0.f, wgt = 0.f;
        bool ok = false;
        int i = 0, j = 0;
        if (live) {
            i = si * a.stride, j = sj * a.stride;  // < h, < w: si < ceil(h / stride)
            const size_t pix = (size_t)i * a.w + j;
            const float d = a.depth[pix];
            float wm = 1.f;
            ok = valid_depth(d);
            if (WEIGHT) {
                wm = a.weight[pix];
                ok = ok && valid_depth(wm);
            }
            if (ok) {
                const float u = (float)j + 0.5f, v = (float)i + 0.5f;
                const float qx = (iK[0] * u + iK[1] * v) + iK[2], qy = (iK[4] * u + iK[5] * v) + iK[6], qz = (iK[8] * u + iK[9] * v) + iK[10];
                const float pcx = qx * d, pcy = qy * d, pcz = qz * d;
                const float pwx = ((R[0] * pcx + R[1] * pcy) + R[2] * pcz) + t[0];
                const float pwy = ((R[3] * pcx + R[4] * pcy) + R[5] * pcz) + t[1];
                const float pwz = ((R[6] * pcx + R[7] * pcy) + R[8] * pcz) + t[2];
                const float gx = (pwx - V.ox) / V.v, gy = (pwy - V.oy) / V.v, gz = (pwz - V.oz) / V.v;
                float fx, fy, fz;
                Corners c;
                ok = cell_of(V, gx, gy, gz, fx, fy, fz);
                if (ok) ok = load_corners(V, gx, gy, gz, fx, fy, fz, c);
                if (ok) {
                    const float f = trilinear(c);
                    float Gx, Gy, Gz;
                    gradient(c, Gx, Gy, Gz);
                    ok = (Gx * Gx + Gy * Gy) + Gz * Gz != 0.f;  // a saturated cell carries no information
                    if (ok) {
                        r = f * V.trunc;
                        const float nx = Gx * a.trunc_voxels, ny = Gy * a.trunc_voxels, nz = Gz * a.trunc_voxels;
                        const float ax = pwx - t[0], ay = pwy - t[1], az = pwz - t[2];
                        J[0] = nx, J[1] = ny, J[2] = nz;
                        J[3] = ay * nz - az * ny, J[4] = az * nx - ax * nz, J[5] = ax * ny - ay * nx;
                        const float ar = fabsf(r);
                        wgt = wm * (a.huber <= 0.f || ar <= a.huber ? 1.f : a.huber / ar);
                    }
                }
            }
            if (!ok) {
#pragma unroll
                for (int k = 0; k < 6; ++k) J[k] = 0.f;
                r = 0.f, wgt = 0.f;
            }
            if (ROWS) {
                // the lane's pixel, and zeros for the pixels of its stride x stride block that are not selected
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                const int i1 = min(i + a.stride, a.h), j1 = min(j + a.stride, a.w);
                for (int ii = i; ii < i1; ++ii)
                    for (int jj = j; jj < j1; ++jj) {
                        float4 *o = reinterpret_cast<float4 *>(a.rows + ((size_t)ii * a.w + jj) * 8);
                        const bool own = ii == i && jj == j;
                        o[0] = own ? make_float4(J[0], J[1], J[2], J[3]) : z;
                        o[1] = own ? make_float4(J[4], J[5], r, wgt) : z;
                    }
            }
        }
        // the 29 products in fp64 from the eight floats (zero for a lane without a row), A as the row-major upper triangle
        double s[kSums];
        {
            const double rd = (double)r, wd = (double)wgt;
            int n = 0;
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                const double wj = wd * (double)J[p];
#pragma unroll
                for (int q = p; q < 6; ++q) s[n++] = wj * (double)J[q];
                s[21 + p] = wj * rd;
            }
            s[27] = (wd * rd) * rd;
            s[28] = ok ? 1.0 : 0.0;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int k = 0; k < kSums; ++k) s[k] += __shfl_down(s[k], off, 64);
        if (lane == 0)
#pragma unroll
            for (int k = 0; k < kSums; ++k) sh[k][wave] = s[k];
        __syncthreads();
        if (tid < kRecord) a.state[kState + (size_t)chunk * kRecord + tid] = tid < kSums ? ((sh[tid][0] + sh[tid][1]) + sh[tid][2]) + sh[tid][3] : 0.0;
        __syncthreads();
    }
}

template <bool FIRST>
__global__ __launch_bounds__(256) void tsdf_align_solve_k(const AlignArgs a) {
    __shared__ double slot[kSlots][kRecord];
    __shared__ double S[kRecord];
    __shared__ double M[6][6];  // A', then L in its lower triangle
    const int tid = threadIdx.x;
    double *st = a.state;
    const bool stopped = !FIRST && st[12] != 0.0;
    if (!stopped) {
        const int e = tid & (kRecord - 1), sl = tid / kRecord;
        double acc = 0.0;
        for (int c = sl; c < a.chunks; c += kSlots) acc += st[kState + (size_t)c * kRecord + e];
        slot[sl][e] = acc;
        __syncthreads();
        if (tid < kRecord) {
            double v = slot[0][tid];
#pragma unroll
            for (int k = 1; k < kSlots; ++k) v += slot[k][tid];
            S[tid] = v;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    double *rec = a.records;
    for (int k = 0; k < IDH_TSDF_ALIGN_RECORD; ++k) rec[k] = 0.0;
    if (FIRST) {
        for (int k = 0; k < 3; ++k) {
            st[3 * k] = (double)a.pose_in[4 * k], st[3 * k + 1] = (double)a.pose_in[4 * k + 1], st[3 * k + 2] = (double)a.pose_in[4 * k + 2];
            st[9 + k] = (double)a.pose_in[4 * k + 3];
        }
        st[12] = 0.0, st[13] = 0.0, st[14] = 0.0, st[15] = 0.0;
    }
    if (stopped) {
        rec[29] = 3.0;
    } else {
        for (int k = 0; k < kSums; ++k) rec[k] = S[k];
        int status = 0;
        double xi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (S[28] < (double)a.min_count) {
            status = 1;
        } else {
            int n = 0;
            for (int p = 0; p < 6; ++p)
                for (int q = p; q < 6; ++q) M[q][p] = S[n++];  // the lower triangle of the symmetric A
            for (int p = 0; p < 6; ++p) M[p][p] = M[p][p] + a.damping * M[p][p];
            for (int k = 0; k < 6 && status == 0; ++k) {
                const double diag = M[k][k];
                double p = diag;
                for (int j = 0; j < k; ++j) p -= M[k][j] * M[k][j];
                if (!(p > a.min_pivot_ratio * diag)) {  // also NaN
                    status = 2;
                    break;
                }
                const double l = sqrt(p);
                M[k][k] = l;
                for (int i = k + 1; i < 6; ++i) {
                    double v = M[i][k];
                    for (int j = 0; j < k; ++j) v -= M[i][j] * M[k][j];
                    M[i][k] = v / l;
                }
            }
            if (status == 0) {
                double *y = &S[0];  // the sums are in the record already
                for (int i = 0; i < 6; ++i) {  // L y = -b
                    double v = -rec[21 + i];
                    for (int j = 0; j < i; ++j) v -= M[i][j] * y[j];
                    y[i] = v / M[i][i];
                }
                for (int i = 5; i >= 0; --i) {  // L^T x = y
                    double v = y[i];
                    for (int j = i + 1; j < 6; ++j) v -= M[j][i] * S[8 + j];
                    S[8 + i] = v / M[i][i];
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) xi[i] = S[8 + i];
            }
        }
        rec[29] = (double)status;
        if (status == 0) {
            const double wx = xi[3], wy = xi[4], wz = xi[5];
            const double nv = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]), th = sqrt((wx * wx + wy * wy) + wz * wz);
            double ca = 1.0, cb = 0.0;  // E = I + ca w^ + cb w^ w^
            if (th >= 1e-12) ca = sin(th) / th, cb = (1.0 - cos(th)) / (th * th);
            const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
            double E[9], Rn[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double kk = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
                    E[3 * i + j] = ((i == j ? 1.0 : 0.0) + ca * K[3 * i + j]) + cb * kk;
                }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (E[3 * i] * st[j] + E[3 * i + 1] * st[3 + j]) + E[3 * i + 2] * st[6 + j];
#pragma unroll
            for (int k = 0; k < 9; ++k) st[k] = Rn[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) st[9 + k] = st[9 + k] + xi[k];
            rec[30] = nv, rec[31] = th;
#pragma unroll
            for (int k = 0; k < 6; ++k) rec[32 + k] = xi[k];
            if (nv < a.min_step && th < a.min_step) st[12] = 1.0;
        } else {
            st[12] = 1.0;
        }
    }
    float *o = a.pose_out;
    for (int k = 0; k < 3; ++k) o[4 * k] = (float)st[3 * k], o[4 * k + 1] = (float)st[3 * k + 1], o[4 * k + 2] = (float)st[3 * k + 2], o[4 * k + 3] = (float)st[9 + k];
    o[12] = 0.f, o[13] = 0.f, o[14] = 0.f, o[15] = 1.f;
}

long long align_chunks(int h, int w, int stride, int &hs, int &ws, int &cx) {
    hs = (int)(((long long)h + stride - 1) / stride), ws = (int)(((long long)w + stride - 1) / stride);
    cx = (ws + 15) / 16;
    return (long long)((hs + 15) / 16) * cx;
}

template <bool FIRST, bool ROWS>
void launch_rows(const AlignArgs &a, unsigned grid, hipStream_t st) {
    if (a.weight) hipLaunchKernelGGL((tsdf_align_rows_k<FIRST, ROWS, true>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((tsdf_align_rows_k<FIRST, ROWS, false>), dim3(grid), dim3(256), 0, st, a);
}

}  // namespace

extern "C" size_t idh_sizeof_tsdf_align_args(void) { return sizeof(idh_tsdf_align_args); }

extern "C" size_t idh_tsdf_align_workspace_bytes(int h, int w, int stride, int iters) {
    if (h < 1 || w < 1 || stride < 1 || iters < 1 || iters > IDH_TSDF_ALIGN_MAX_ITERS || (long long)h * w >= (1ll << 31)) return 0;
    int hs, ws, cx;
    return 8 * ((size_t)kState + (size_t)kRecord * (size_t)align_chunks(h, w, stride, hs, ws, cx));
}

extern "C" int idh_tsdf_align_fwd(const idh_tsdf_align_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_tsdf_align_args)) return IDH_EINVAL;
    const idh_tsdf_align_args &e = *args;
    if (e.h <= 0 || e.w <= 0 || e.iters < 1 || e.iters > IDH_TSDF_ALIGN_MAX_ITERS || e.stride < 1 || e.min_count < 6 || e.max_workgroups < 0) return IDH_EINVAL;
    if (!(fabsf(e.huber) < INFINITY)) return IDH_EINVAL;  // also NaN
    if (!(e.damping >= 0.0 && e.damping < (double)INFINITY) || !(e.min_step >= 0.0 && e.min_step < (double)INFINITY)) return IDH_EINVAL;
    if (!(e.min_pivot_ratio >= 0.0 && e.min_pivot_ratio < 1.0)) return IDH_EINVAL;
    if (!e.depth_11hw || !e.invK_44 || !e.world_T_cam_in_44 || !e.world_T_cam_out_44 || !e.records_i40) return IDH_EINVAL;
    if (((uintptr_t)e.workspace & 7u) || ((uintptr_t)e.rows_hw8 & 15u)) return IDH_EINVAL;
    AlignArgs a;
    if (const int rc = check_volume(e.volume, a.V)) return rc;
    if ((long long)e.h * e.w >= (1ll << 31)) return IDH_EUNSUPPORTED;
    const size_t need = idh_tsdf_align_workspace_bytes(e.h, e.w, e.stride, e.iters);
    if (!e.workspace || e.workspace_bytes < 0 || (size_t)e.workspace_bytes < need) return IDH_EWORKSPACE;
    const long long chunks = align_chunks(e.h, e.w, e.stride, a.hs, a.ws, a.cx);
    a.depth = e.depth_11hw, a.invK = e.invK_44, a.weight = e.weight_11hw, a.pose_in = e.world_T_cam_in_44;
    a.pose_out = e.world_T_cam_out_44, a.rows = e.rows_hw8;
    a.state = static_cast<double *>(e.workspace);
    a.damping = e.damping, a.min_step = e.min_step, a.min_pivot_ratio = e.min_pivot_ratio;
    a.trunc_voxels = e.volume.trunc_voxels, a.huber = e.huber;
    a.h = e.h, a.w = e.w, a.chunks = (int)chunks, a.stride = e.stride, a.min_count = e.min_count;
    const unsigned grid = (unsigned)(e.max_workgroups > 0 && e.max_workgroups < chunks ? e.max_workgroups : chunks);
    hipStream_t st = idh_stream(stream);
    for (int it = 0; it < e.iters; ++it) {
        a.records = e.records_i40 + (size_t)it * IDH_TSDF_ALIGN_RECORD;
        if (it == 0) {
            if (a.rows) launch_rows<true, true>(a, grid, st);
            else launch_rows<true, false>(a, grid, st);
            hipLaunchKernelGGL(tsdf_align_solve_k<true>, dim3(1), dim3(256), 0, st, a);
        } else {
            launch_rows<false, false>(a, grid, st);
            hipLaunchKernelGGL(tsdf_align_solve_k<false>, dim3(1), dim3(256), 0, st, a);
        }
        IDH_CHECK_LAUNCH();
    }
    return IDH_OK;
}
