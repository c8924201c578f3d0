// TSDF fusion (include/idh_fusion.h): depth maps averaged into a dense truncated signed distance volume, and the fused
// surface ray-cast into live cameras.  The header states the arithmetic; this file follows it expression by expression.
//
//   tsdf_reset_k      every voxel to {1, 0}, every block flag to 0.
//   tsdf_flags_k      block flags from the values of a volume made elsewhere (after a clear).
//   tsdf_integrate_k  one lane per voxel, a wave along x; the M cameras are wave-uniform (scalar loads), the voxel's {T, W} pair stays in
//                     registers over the M maps: one 8-byte load at the first map that touches it, one 8-byte store at the end.
//                     With IntegrateColorArgs the same kernel also averages a camera frame's tap into the voxel's {R, G, B, Wc} quad
//                     (one 16-byte load and store per coloured voxel, three byte gathers per coloured voxel and map).
//                     With Weighted<..> on top of either, a weight map tapped where the depth is scales the observation.
//   tsdf_shift_k<COLOR>  a second volume whose grid lies a whole number of voxels further: one lane per voxel of it, the
//                     launch shape of tsdf_integrate_k; what stays is copied bit for bit, what comes in - and what was never observed - is
//                     written in the empty state, and the flags are marked as tsdf_flags_k marks them.
//   tsdf_raycast_k<SKIP, NORMALS, Args>  one lane per pixel, an 8 x 8-pixel tile per wave.  A sample reads its eight corners as four 16-byte
//                     loads: the x-neighbours {T0, W0, T1, W1} are adjacent in memory (8-byte aligned, which the global loads of gfx950
//                     take).  SKIP clips the lattice range to the volume's box and jumps blocks whose flag is 0.  With RaycastColorArgs
//                     also the hit's colour: eight 16-byte loads of {R, G, B, Wc} once per pixel, after the march.
//
// The colour variants are instantiations on an argument struct derived from the plain one: the plain instantiations keep
// their kernel arguments and their code.
//
// Block flags.  A lane's row is 64 consecutive x, so the eight lanes of an aligned group share one block along x: the group's first lane
// stores for the group (one ballot), and a touched voxel on a block's low face also stores for the block before it (the + 1 apron).
// Only the value 1 is ever stored between resets, so concurrent stores need no atomic.
#include <string.h>

#include "tsdf_common.h"

namespace {

__global__ __launch_bounds__(256) void tsdf_reset_k(float2 *__restrict__ values, long long n, uint8_t *__restrict__ flags, long long nb) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i < n) values[i] = make_float2(1.f, 0.f);
    if (i < nb) flags[i] = 0;
}

// flags of the blocks whose cells read a voxel of block column bx (already resolved along x) at row y, slice z
__device__ __forceinline__ void mark_yz(const Vol &V, int bx, int y, int z) {
    if (bx < 0 || bx >= V.nbx) return;
    const int by1 = y >> 3, bz1 = z >> 3;
    const int by0 = (y & 7) == 0 && y > 0 ? by1 - 1 : by1, bz0 = (z & 7) == 0 && z > 0 ? bz1 - 1 : bz1;
    for (int bz = bz0; bz <= bz1; ++bz)
        for (int by = by0; by <= by1; ++by)
            if (bz < V.nbz && by < V.nby) V.flags[((size_t)bz * V.nby + by) * V.nbx + bx] = 1;
}

// `seen`: this lane's voxel (x, y, z) has W > 0.  Called by every lane of the wave (x = 64-aligned base + lane).
__device__ __forceinline__ void mark_blocks(const Vol &V, bool seen, int x, int y, int z) {
    const unsigned long long mask = __ballot(seen);
    const int lane = threadIdx.x & 63;
    if ((lane & 7) != 0) return;
    if ((mask >> lane) & 0xffull) mark_yz(V, x >> 3, y, z);
    if (seen && x > 0) mark_yz(V, (x >> 3) - 1, y, z);
}

__global__ __launch_bounds__(256) void tsdf_flags_k(const Vol V) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    if (y >= V.Ny) return;  // whole wave
    bool seen = false;
    if (x < V.Nx) seen = V.values[2 * (((size_t)z * V.Ny + y) * V.Nx + x) + 1] > 0.f;
    mark_blocks(V, seen, x, y, z);
}

struct IntegrateArgs {
    static constexpr bool kColor = false;
    static constexpr bool kWeighted = false;
    Vol V;
    const float *depth, *K, *T;
    float max_weight;
    int M, h, w;
};

// the colour variant's arguments come after the plain ones, so the plain instantiation's kernel arguments are what they were
struct IntegrateColorArgs : IntegrateArgs {
    static constexpr bool kColor = true;
    float4 *colors;
    const uint8_t *frames;
    const float *Kc;
    int hc, wc;
};

// a per-observation weight map on top of either struct (again after the arguments that were there)
template <class Base>
struct Weighted : Base {
    static constexpr bool kWeighted = true;
    const float *weight;
};

template <class Args>
__global__ __launch_bounds__(256) void tsdf_integrate_k(const Args a) {
    constexpr bool COLOR = Args::kColor, WEIGHTED = Args::kWeighted;
    const Vol &V = a.V;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    if (y >= V.Ny) return;  // whole wave
    const bool live = x < V.Nx;
    const float px = V.ox + V.v * (float)x, py = V.oy + V.v * (float)y, pz = V.oz + V.v * (float)z;
    float2 *cell = reinterpret_cast<float2 *>(V.values) + (((size_t)z * V.Ny + y) * V.Nx + (live ? x : 0));
    float T = 1.f, W = 0.f;
    bool touched = false;
    const float fw = (float)a.w, fh = (float)a.h;
    float4 col = make_float4(0.f, 0.f, 0.f, 0.f);  // {R, G, B, Wc}
    bool coloured = false;
    for (int m = 0; m < a.M; ++m) {
        const float *E = a.T + m * 16, *K = a.K + m * 16;  // wave-uniform
        const float cz = ((E[8] * px + E[9] * py) + E[10] * pz) + E[11];
        if (!(live && cz > 0.f)) continue;
        const float cx = ((E[0] * px + E[1] * py) + E[2] * pz) + E[3];
        const float cy = ((E[4] * px + E[5] * py) + E[6] * pz) + E[7];
        const float u = K[0] * (cx / cz) + K[2], v = K[5] * (cy / cz) + K[6];
        if (!(u >= 0.f && u < fw && v >= 0.f && v < fh)) continue;  // also refuses NaN
        const int j = (int)floorf(u), i = (int)floorf(v);
        const float d = a.depth[((size_t)m * a.h + i) * a.w + j];
        if (!valid_depth(d)) continue;
        float g = 1.f;
        if constexpr (WEIGHTED) {
            g = a.weight[((size_t)m * a.h + i) * a.w + j];
            if (!valid_depth(g)) continue;  // a weight that is not finite and > 0 makes the tap a hole
        }
        const float sdf = d - cz;
        if (sdf < -V.trunc) continue;
        const float s = fminf(1.f, sdf / V.trunc);
        if (!touched) {
            const float2 tw = *cell;
            T = tw.x, W = tw.y;
            touched = true;
        }
        if constexpr (WEIGHTED) {
            T = (W * T + g * s) / (W + g);
            W = fminf(W + g, a.max_weight);
        } else {
            T = (W * T + s) / (W + 1.f);
            W = fminf(W + 1.f, a.max_weight);
        }
        if constexpr (COLOR) {
            if (!(sdf <= V.trunc)) continue;  // free space in front of the band
            const float *Kc = a.Kc + m * 16;
            const float qx = Kc[0] * (cx / cz) + Kc[2], qy = Kc[5] * (cy / cz) + Kc[6];
            if (!(qx >= 0.f && qx < (float)a.wc && qy >= 0.f && qy < (float)a.hc)) continue;
            const uint8_t *tap = a.frames + (((size_t)m * a.hc + (int)floorf(qy)) * a.wc + (int)floorf(qx)) * 3;
            const float r = (float)tap[0], gr = (float)tap[1], b = (float)tap[2];
            float4 *quad = a.colors + (((size_t)z * V.Ny + y) * V.Nx + x);
            if (!coloured) col = *quad, coloured = true;
            if constexpr (WEIGHTED) {
                col.x = (col.w * col.x + g * r) / (col.w + g);
                col.y = (col.w * col.y + g * gr) / (col.w + g);
                col.z = (col.w * col.z + g * b) / (col.w + g);
                col.w = fminf(col.w + g, a.max_weight);
            } else {
                col.x = (col.w * col.x + r) / (col.w + 1.f);
                col.y = (col.w * col.y + gr) / (col.w + 1.f);
                col.z = (col.w * col.z + b) / (col.w + 1.f);
                col.w = fminf(col.w + 1.f, a.max_weight);
            }
        }
    }
    if (touched) *cell = make_float2(T, W);
    if constexpr (COLOR) {
        if (coloured) a.colors[((size_t)z * V.Ny + y) * V.Nx + x] = col;
    }
    mark_blocks(V, touched, x, y, z);  // a touched voxel has W > 0
}

struct ShiftArgs {
    Vol V;  // dst: its dims are src's too
    const float2 *src;
    const float4 *src_colors;
    float4 *dst_colors;
    int sx, sy, sz;
};

// dst voxel (x, y, z) <- src voxel (x + sx, y + sy, z + sz) where that is inside and observed, else the empty state.  The lane's source
// row is a run of consecutive pairs like its destination row, offset by sx pairs: both stay 8-byte (16-byte for the quads) aligned and
// coalesced for every shift.  y + sy and z + sz are wave-uniform.  The quad is read only where W > 0: most of a room's volume is not.
template <bool COLOR>
__global__ __launch_bounds__(256) void tsdf_shift_k(const ShiftArgs a) {
    const Vol &V = a.V;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    if (y >= V.Ny) return;  // whole wave
    const bool live = x < V.Nx;
    const long long ax = (long long)x + a.sx, ay = (long long)y + a.sy, az = (long long)z + a.sz;
    float2 tw = make_float2(1.f, 0.f);
    float4 col = make_float4(0.f, 0.f, 0.f, 0.f);
    bool seen = false;
    if (live && ax >= 0 && ax < V.Nx && ay >= 0 && ay < V.Ny && az >= 0 && az < V.Nz) {
        const size_t s = ((size_t)az * V.Ny + (size_t)ay) * V.Nx + (size_t)ax;
        const float2 t = a.src[s];
        if (t.y > 0.f) {  // false for NaN
            tw = t, seen = true;
            if constexpr (COLOR) col = a.src_colors[s];
        }
    }
    if (live) {
        const size_t d = ((size_t)z * V.Ny + y) * V.Nx + x;
        reinterpret_cast<float2 *>(V.values)[d] = tw;
        if constexpr (COLOR) a.dst_colors[d] = col;
    }
    mark_blocks(V, seen, x, y, z);
}

struct RaycastArgs {
    static constexpr bool kColor = false;
    Vol V;
    const float *world_T_cam, *invK;
    float *depth, *normals;
    uint8_t *flags;
    float near, step_voxels, empty_depth;
    int max_steps, world_normals, B, H, W;
};

struct RaycastColorArgs : RaycastArgs {  // as IntegrateColorArgs: the plain arguments first
    static constexpr bool kColor = true;
    const float4 *colors;
    uint8_t *rgba;
};

__device__ __forceinline__ unsigned channel_byte(float c) { return (unsigned)(int)(fminf(fmaxf(c, 0.f), 255.f) + 0.5f); }

template <bool SKIP, bool NORMALS, class Args>
__global__ __launch_bounds__(256) void tsdf_raycast_k(const Args a) {
    constexpr bool COLOR = Args::kColor;
    const Vol &V = a.V;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), i = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3), b = blockIdx.z;
    if (i >= a.H || j >= a.W) return;
    const float *E = a.world_T_cam + b * 16, *iK = a.invK + b * 16;
    const float u = (float)j + 0.5f, v = (float)i + 0.5f;
    const float qx = (iK[0] * u + iK[1] * v) + iK[2], qy = (iK[4] * u + iK[5] * v) + iK[6], qz = (iK[8] * u + iK[9] * v) + iK[10];
    const float n = sqrtf((qx * qx + qy * qy) + qz * qz);
    const float dcx = qx / n, dcy = qy / n, dcz = qz / n;
    const float dx = (E[0] * dcx + E[1] * dcy) + E[2] * dcz, dy = (E[4] * dcx + E[5] * dcy) + E[6] * dcz, dz = (E[8] * dcx + E[9] * dcy) + E[10] * dcz;
    const float ogx = (E[3] - V.ox) / V.v, ogy = (E[7] - V.oy) / V.v, ogz = (E[11] - V.oz) / V.v;
    const float dgx = dx / V.v, dgy = dy / V.v, dgz = dz / V.v;
    const float step = a.step_voxels * V.v, near = a.near;

    int k = 0, k_last = a.max_steps - 1;
    if (SKIP) {
        // The lattice range that can hold a known sample: the slab test against the box of cells [0, N - 1), widened by kMargin voxels
        // and two samples - far more than the fp32 error of g, so every sample left out is out of the volume.
        const float kMargin = 0.01f;
        const float og[3] = {ogx, ogy, ogz}, dg[3] = {dgx, dgy, dgz}, hi[3] = {(float)(V.Nx - 1), (float)(V.Ny - 1), (float)(V.Nz - 1)};
        float t_in = -INFINITY, t_out = INFINITY;
        bool never = false;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (dg[ax] == 0.f) {
                never |= !(og[ax] >= 0.f && og[ax] < hi[ax]);  // g is og at every sample
            } else {
                const float t1 = (-kMargin - og[ax]) / dg[ax], t2 = ((hi[ax] + kMargin) - og[ax]) / dg[ax];
                t_in = fmaxf(t_in, fminf(t1, t2));
                t_out = fminf(t_out, fmaxf(t1, t2));
            }
        }
        const float top = (float)a.max_steps;
        const float k0 = fminf(fmaxf(floorf((t_in - near) / step) - 2.f, 0.f), top);          // NaN -> 0
        const float k1 = fmaxf(fminf(ceilf((t_out - near) / step) + 2.f, top - 1.f), -1.f);  // NaN -> max_steps - 1
        k = never ? a.max_steps : (int)k0;
        k_last = (int)k1;
    }

    int known_count = 0, hit_k = -1, cur_block = -1;
    unsigned cur_flag = 1;
    bool prev_known = false;
    float f_prev = 0.f, t_star = 0.f;
    while (k <= k_last) {
        const float t = near + (float)k * step;
        const float gx = ogx + t * dgx, gy = ogy + t * dgy, gz = ogz + t * dgz;
        float fx, fy, fz, f = 0.f;
        bool known = cell_of(V, gx, gy, gz, fx, fy, fz);
        Corners c;
        if (SKIP && known) {
            const int bx = (int)fx >> 3, by = (int)fy >> 3, bz = (int)fz >> 3;
            const int block = (bz * V.nby + by) * V.nbx + bx;
            // (fetching the corners together with a new block's flag, so that the flag's latency is not in front of theirs, was measured:
            // no faster where blocks are flagged, 18 % slower where they are not - profiles/tsdf/README.md)
            if (block != cur_block) cur_block = block, cur_flag = V.flags[block];
            if (!cur_flag) {
                // Nothing in this block is known: leave it.  t_exit is where the ray leaves the block shrunk by kMargin; the samples up
                // to two before it lie inside the block (g is monotone in k on every axis, in fp32 too), so they are not known either.
                const float kMargin = 0.01f;
                const float lo[3] = {(float)(bx * 8), (float)(by * 8), (float)(bz * 8)}, og[3] = {ogx, ogy, ogz}, dg[3] = {dgx, dgy, dgz};
                float t_exit = INFINITY;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    if (dg[ax] > 0.f) t_exit = fminf(t_exit, ((lo[ax] + (8.f - kMargin)) - og[ax]) / dg[ax]);
                    if (dg[ax] < 0.f) t_exit = fminf(t_exit, ((lo[ax] + kMargin) - og[ax]) / dg[ax]);
                }
                const float kn = fminf(fmaxf(floorf((t_exit - near) / step) - 1.f, (float)(k + 1)), (float)(k_last + 1));  // NaN -> k + 1
                k = (int)kn;
                prev_known = false;
                continue;
            }
        }
        if (known) known = load_corners(V, gx, gy, gz, fx, fy, fz, c);
        if (known) {
            f = trilinear(c);
            ++known_count;
            if (prev_known && f_prev > 0.f && f <= 0.f) {
                const float t_prev = near + (float)(k - 1) * step;
                t_star = t_prev + step * (f_prev / (f_prev - f));
                hit_k = k;
                break;
            }
        }
        prev_known = known, f_prev = f;
        ++k;
    }

    const int total = hit_k >= 0 ? hit_k + 1 : a.max_steps;
    unsigned flags = hit_k >= 0 ? IDH_TSDF_HIT : 0u;
    if (known_count == 0) flags |= IDH_TSDF_NONE_KNOWN;
    else if (known_count < total) flags |= IDH_TSDF_SOME_KNOWN;
    const size_t pix = ((size_t)b * a.H + i) * a.W + j, plane = (size_t)a.H * a.W;
    a.depth[pix] = hit_k >= 0 ? t_star * dcz : a.empty_depth;
    if (NORMALS) {
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (hit_k >= 0) {
            const float gx = ogx + t_star * dgx, gy = ogy + t_star * dgy, gz = ogz + t_star * dgz;
            float fx, fy, fz;
            Corners c;
            bool ok = cell_of(V, gx, gy, gz, fx, fy, fz);
            if (ok) ok = load_corners(V, gx, gy, gz, fx, fy, fz, c);
            if (ok) {
                float Gx, Gy, Gz;
                gradient(c, Gx, Gy, Gz);
                const float len = sqrtf((Gx * Gx + Gy * Gy) + Gz * Gz);
                ok = len > 0.f;
                if (ok) {
                    float wx = Gx / len, wy = Gy / len, wz = Gz / len;
                    if ((wx * dx + wy * dy) + wz * dz > 0.f) wx = -wx, wy = -wy, wz = -wz;
                    if (a.world_normals) {
                        nx = wx, ny = wy, nz = wz;
                    } else {  // R^T N
                        nx = (E[0] * wx + E[4] * wy) + E[8] * wz;
                        ny = (E[1] * wx + E[5] * wy) + E[9] * wz;
                        nz = (E[2] * wx + E[6] * wy) + E[10] * wz;
                    }
                }
            }
            if (!ok) flags |= IDH_TSDF_NO_NORMAL;
        }
        float *o = a.normals + (size_t)b * 3 * plane + (size_t)i * a.W + j;
        o[0] = nx, o[plane] = ny, o[2 * plane] = nz;
    }
    a.flags[pix] = (uint8_t)flags;
    if constexpr (COLOR) {
        // once per pixel, outside the march: the coloured corners of the hit's cell, weighted trilinearly and renormalised
        unsigned rgba = 0u;
        if (hit_k >= 0) {
            const float gx = ogx + t_star * dgx, gy = ogy + t_star * dgy, gz = ogz + t_star * dgz;
            float fx, fy, fz;
            if (cell_of(V, gx, gy, gz, fx, fy, fz)) {
                const float rx = gx - fx, ry = gy - fy, rz = gz - fz;
                const size_t row = (size_t)V.Nx, slice = row * V.Ny;
                const float4 *p = a.colors + ((size_t)(int)fz * slice + (size_t)(int)fy * row + (size_t)(int)fx);
                float nr = 0.f, ng = 0.f, nb = 0.f, den = 0.f;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int ex = c & 1, ey = (c >> 1) & 1, ez = c >> 2;
                    const float4 q = p[ex + ey * row + ez * slice];
                    if (!(q.w > 0.f)) continue;
                    const float w = ((ex ? rx : 1.f - rx) * (ey ? ry : 1.f - ry)) * (ez ? rz : 1.f - rz);
                    nr += w * q.x, ng += w * q.y, nb += w * q.z, den += w;
                }
                if (den > 0.f) rgba = channel_byte(nr / den) | channel_byte(ng / den) << 8 | channel_byte(nb / den) << 16 | 255u << 24;
            }
        }
        reinterpret_cast<unsigned *>(a.rgba)[pix] = rgba;  // bytes R, G, B, A in memory order
    }
}

dim3 voxel_grid(const Vol &V) { return dim3(idh_cdiv(V.Nx, 64), idh_cdiv(V.Ny, 4), V.Nz); }

int clear_volume(const Vol &V, bool values, hipStream_t st) {
    const long long n = values ? (long long)V.Nx * V.Ny * V.Nz : 0, nb = (long long)V.nbx * V.nby * V.nbz;
    hipLaunchKernelGGL(tsdf_reset_k, dim3(idh_cdiv(n > nb ? n : nb, 256)), dim3(256), 0, st, reinterpret_cast<float2 *>(V.values), n, V.flags, nb);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

}  // namespace

extern "C" size_t idh_sizeof_tsdf_volume(void) { return sizeof(idh_tsdf_volume); }
extern "C" size_t idh_sizeof_tsdf_integrate_args(void) { return sizeof(idh_tsdf_integrate_args); }
extern "C" size_t idh_sizeof_tsdf_raycast_args(void) { return sizeof(idh_tsdf_raycast_args); }
extern "C" size_t idh_sizeof_tsdf_integrate_color_args(void) { return sizeof(idh_tsdf_integrate_color_args); }
extern "C" size_t idh_sizeof_tsdf_raycast_color_args(void) { return sizeof(idh_tsdf_raycast_color_args); }
extern "C" size_t idh_sizeof_tsdf_integrate_weighted_args(void) { return sizeof(idh_tsdf_integrate_weighted_args); }

extern "C" size_t idh_tsdf_block_flag_bytes(int Nz, int Ny, int Nx) {
    if (Nz < 2 || Ny < 2 || Nx < 2) return 0;
    return (size_t)tsdf_blocks(Nz) * (size_t)tsdf_blocks(Ny) * (size_t)tsdf_blocks(Nx);
}

extern "C" int idh_tsdf_reset_fwd(const idh_tsdf_volume *vol, void *stream) {
    if (!vol) return IDH_EINVAL;
    Vol V;
    if (const int rc = check_volume(*vol, V)) return rc;
    return clear_volume(V, true, idh_stream(stream));
}

extern "C" int idh_tsdf_flags_fwd(const idh_tsdf_volume *vol, void *stream) {
    if (!vol) return IDH_EINVAL;
    Vol V;
    if (const int rc = check_volume(*vol, V)) return rc;
    hipStream_t st = idh_stream(stream);
    if (const int rc = clear_volume(V, false, st)) return rc;
    hipLaunchKernelGGL(tsdf_flags_k, voxel_grid(V), dim3(64, 4), 0, st, V);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_tsdf_integrate_fwd(const idh_tsdf_integrate_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_tsdf_integrate_args)) return IDH_EINVAL;
    const idh_tsdf_integrate_args &e = *args;
    if (e.M <= 0 || e.h <= 0 || e.w <= 0) return IDH_EINVAL;
    if (!(e.max_weight >= 1.f && e.max_weight < INFINITY)) return IDH_EINVAL;
    if (!e.depth_m1hw || !e.K_m44 || !e.cam_T_world_m44) return IDH_EINVAL;
    IntegrateArgs a;
    if (const int rc = check_volume(e.volume, a.V)) return rc;
    if (e.M > IDH_TSDF_MAX_MAPS || (long long)e.M * e.h * e.w >= (1ll << 31)) return IDH_EUNSUPPORTED;
    a.depth = e.depth_m1hw, a.K = e.K_m44, a.T = e.cam_T_world_m44;
    a.max_weight = e.max_weight, a.M = e.M, a.h = e.h, a.w = e.w;
    hipLaunchKernelGGL(tsdf_integrate_k<IntegrateArgs>, voxel_grid(a.V), dim3(64, 4), 0, idh_stream(stream), a);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_tsdf_integrate_color_fwd(const idh_tsdf_integrate_color_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_tsdf_integrate_color_args)) return IDH_EINVAL;
    const idh_tsdf_integrate_color_args &e = *args;
    if (e.M <= 0 || e.h <= 0 || e.w <= 0 || e.hc <= 0 || e.wc <= 0) return IDH_EINVAL;
    if (!(e.max_weight >= 1.f && e.max_weight < INFINITY)) return IDH_EINVAL;
    if (!e.depth_m1hw || !e.K_m44 || !e.cam_T_world_m44 || !e.colors_zyx4 || !e.color_mhw3 || !e.color_K_m44) return IDH_EINVAL;
    if ((uintptr_t)e.colors_zyx4 & 15u) return IDH_EINVAL;
    IntegrateColorArgs a;
    if (const int rc = check_volume(e.volume, a.V)) return rc;
    if (e.M > IDH_TSDF_MAX_MAPS || (long long)e.M * e.h * e.w >= (1ll << 31) || (long long)e.M * e.hc * e.wc >= (1ll << 31)) return IDH_EUNSUPPORTED;
    a.depth = e.depth_m1hw, a.K = e.K_m44, a.T = e.cam_T_world_m44;
    a.max_weight = e.max_weight, a.M = e.M, a.h = e.h, a.w = e.w;
    a.colors = reinterpret_cast<float4 *>(e.colors_zyx4), a.frames = e.color_mhw3, a.Kc = e.color_K_m44, a.hc = e.hc, a.wc = e.wc;
    hipLaunchKernelGGL(tsdf_integrate_k<IntegrateColorArgs>, voxel_grid(a.V), dim3(64, 4), 0, idh_stream(stream), a);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_tsdf_integrate_weighted_fwd(const idh_tsdf_integrate_weighted_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_tsdf_integrate_weighted_args)) return IDH_EINVAL;
    const idh_tsdf_integrate_weighted_args &e = *args;
    const bool color = e.colors_zyx4 || e.color_mhw3 || e.color_K_m44;
    if (e.M <= 0 || e.h <= 0 || e.w <= 0 || (color && (e.hc <= 0 || e.wc <= 0))) return IDH_EINVAL;
    if (!(e.max_weight >= 1.f && e.max_weight < INFINITY)) return IDH_EINVAL;
    if (!e.depth_m1hw || !e.K_m44 || !e.cam_T_world_m44 || !e.weight_m1hw) return IDH_EINVAL;
    if (color && (!e.colors_zyx4 || !e.color_mhw3 || !e.color_K_m44 || ((uintptr_t)e.colors_zyx4 & 15u))) return IDH_EINVAL;
    Weighted<IntegrateColorArgs> a;
    if (const int rc = check_volume(e.volume, a.V)) return rc;
    if (e.M > IDH_TSDF_MAX_MAPS || (long long)e.M * e.h * e.w >= (1ll << 31) || (color && (long long)e.M * e.hc * e.wc >= (1ll << 31))) return IDH_EUNSUPPORTED;
    a.depth = e.depth_m1hw, a.K = e.K_m44, a.T = e.cam_T_world_m44;
    a.max_weight = e.max_weight, a.M = e.M, a.h = e.h, a.w = e.w;
    a.colors = reinterpret_cast<float4 *>(e.colors_zyx4), a.frames = e.color_mhw3, a.Kc = e.color_K_m44, a.hc = e.hc, a.wc = e.wc;
    a.weight = e.weight_m1hw;
    if (color) {
        hipLaunchKernelGGL(tsdf_integrate_k<Weighted<IntegrateColorArgs>>, voxel_grid(a.V), dim3(64, 4), 0, idh_stream(stream), a);
    } else {
        Weighted<IntegrateArgs> g;
        static_cast<IntegrateArgs &>(g) = static_cast<const IntegrateArgs &>(a);
        g.weight = e.weight_m1hw;
        hipLaunchKernelGGL(tsdf_integrate_k<Weighted<IntegrateArgs>>, voxel_grid(a.V), dim3(64, 4), 0, idh_stream(stream), g);
    }
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" size_t idh_sizeof_tsdf_shift_args(void) { return sizeof(idh_tsdf_shift_args); }

extern "C" int idh_tsdf_shift_fwd(const idh_tsdf_shift_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_tsdf_shift_args)) return IDH_EINVAL;
    const idh_tsdf_shift_args &e = *args;
    if (!e.src_colors_zyx4 != !e.dst_colors_zyx4) return IDH_EINVAL;
    if (((uintptr_t)e.src_colors_zyx4 & 15u) || ((uintptr_t)e.dst_colors_zyx4 & 15u)) return IDH_EINVAL;
    Vol S;
    ShiftArgs a;
    if (const int rc = check_volume(e.src, S)) return rc;
    if (const int rc = check_volume(e.dst, a.V)) return rc;
    const auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
    if (e.src.Nz != e.dst.Nz || e.src.Ny != e.dst.Ny || e.src.Nx != e.dst.Nx) return IDH_EINVAL;
    if (bits(e.src.voxel_size) != bits(e.dst.voxel_size) || bits(e.src.trunc_voxels) != bits(e.dst.trunc_voxels)) return IDH_EINVAL;
    for (int i = 0; i < 3; ++i) {
        const float step = e.src.voxel_size * (float)e.shift[i];
        const float want = e.src.origin[i] + step;
        if (bits(e.dst.origin[i]) != bits(want)) return IDH_EINVAL;
    }
    const size_t n = (size_t)S.Nx * S.Ny * S.Nz, nb = (size_t)S.nbx * S.nby * S.nbz;
    const bool color = e.src_colors_zyx4 != nullptr;
    const uintptr_t lo_s[3] = {(uintptr_t)S.values, (uintptr_t)S.flags, (uintptr_t)e.src_colors_zyx4};
    const uintptr_t lo_d[3] = {(uintptr_t)a.V.values, (uintptr_t)a.V.flags, (uintptr_t)e.dst_colors_zyx4};
    const size_t len[3] = {8 * n, nb, 16 * n};
    for (int i = 0; i < (color ? 3 : 2); ++i)
        for (int j = 0; j < (color ? 3 : 2); ++j)
            if (lo_s[i] < lo_d[j] + len[j] && lo_d[j] < lo_s[i] + len[i]) return IDH_EINVAL;
    a.src = reinterpret_cast<const float2 *>(S.values);
    a.src_colors = reinterpret_cast<const float4 *>(e.src_colors_zyx4), a.dst_colors = reinterpret_cast<float4 *>(e.dst_colors_zyx4);
    a.sx = e.shift[0], a.sy = e.shift[1], a.sz = e.shift[2];
    hipStream_t st = idh_stream(stream);
    if (const int rc = clear_volume(a.V, false, st)) return rc;
    if (color) hipLaunchKernelGGL(tsdf_shift_k<true>, voxel_grid(a.V), dim3(64, 4), 0, st, a);
    else hipLaunchKernelGGL(tsdf_shift_k<false>, voxel_grid(a.V), dim3(64, 4), 0, st, a);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

namespace {

// what both ray casts check and set, in the header's order (the colour call's own pointers are checked by its entry point in between)
template <class E>
int raycast_check_inputs(const E &e) {
    if (e.B <= 0 || e.H <= 0 || e.W <= 0 || e.max_steps <= 0) return IDH_EINVAL;
    if (!(e.step_voxels > 0.f && e.step_voxels <= 1.f)) return IDH_EINVAL;  // also refuses NaN
    if (!(e.near >= 0.f && e.near < INFINITY) || e.empty_depth != e.empty_depth) return IDH_EINVAL;
    if (!e.world_T_cam_b44 || !e.invK_b44 || !e.depth_b1hw || !e.flags_bhw) return IDH_EINVAL;
    return IDH_OK;
}

template <class E, class A>
int raycast_launch(const E &e, A &a, hipStream_t st) {
    if (const int rc = check_volume(e.volume, a.V)) return rc;
    if (e.B > IDH_TSDF_MAX_CAMERAS || (long long)e.B * e.H * e.W >= (1ll << 31) || e.max_steps > IDH_TSDF_MAX_STEPS) return IDH_EUNSUPPORTED;
    a.world_T_cam = e.world_T_cam_b44, a.invK = e.invK_b44, a.depth = e.depth_b1hw, a.normals = e.normals_b3hw, a.flags = e.flags_bhw;
    a.near = e.near, a.step_voxels = e.step_voxels, a.empty_depth = e.empty_depth;
    a.max_steps = e.max_steps, a.world_normals = e.world_normals, a.B = e.B, a.H = e.H, a.W = e.W;
    const dim3 grid(idh_cdiv(e.W, 16), idh_cdiv(e.H, 16), e.B);
    if (e.skip) {
        if (e.normals_b3hw) hipLaunchKernelGGL((tsdf_raycast_k<true, true, A>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((tsdf_raycast_k<true, false, A>), grid, dim3(256), 0, st, a);
    } else {
        if (e.normals_b3hw) hipLaunchKernelGGL((tsdf_raycast_k<false, true, A>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((tsdf_raycast_k<false, false, A>), grid, dim3(256), 0, st, a);
    }
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

}  // namespace

extern "C" int idh_tsdf_raycast_fwd(const idh_tsdf_raycast_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_tsdf_raycast_args)) return IDH_EINVAL;
    if (const int rc = raycast_check_inputs(*args)) return rc;
    RaycastArgs a;
    return raycast_launch(*args, a, idh_stream(stream));
}

extern "C" int idh_tsdf_raycast_color_fwd(const idh_tsdf_raycast_color_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_tsdf_raycast_color_args)) return IDH_EINVAL;
    if (const int rc = raycast_check_inputs(*args)) return rc;
    if (!args->colors_zyx4 || !args->rgba_bhw4 || ((uintptr_t)args->colors_zyx4 & 15u)) return IDH_EINVAL;
    RaycastColorArgs a;
    a.colors = reinterpret_cast<const float4 *>(args->colors_zyx4), a.rgba = args->rgba_bhw4;
    return raycast_launch(*args, a, idh_stream(stream));
}
