// What the TSDF kernels share (tsdf.hip, tsdf_mesh.hip, tsdf_align.hip): the volume as the kernels take it, the host-side check of an
// idh_tsdf_volume in the order include/idh_fusion.h states, and the sample of a cell (corners, interpolant, gradient).
#pragma once
#include <math.h>

#include "../../include/idh_fusion.h"
#include "idh_common.h"

namespace {

struct Vol {
    float *values;
    uint8_t *flags;
    float ox, oy, oz, v, trunc;
    int Nx, Ny, Nz, nbx, nby, nbz;
};

__host__ __device__ inline int tsdf_blocks(int n) { return (n + 6) / 8; }  // 8-cell blocks over n - 1 cells

inline bool finite_pos(float x) { return x > 0.f && x < INFINITY; }

// the volume's conditions, in the header's order
inline int check_volume(const idh_tsdf_volume &e, Vol &V) {
    if (e.struct_size < (int64_t)sizeof(idh_tsdf_volume)) return IDH_EINVAL;
    if (e.Nz < 2 || e.Ny < 2 || e.Nx < 2) return IDH_EINVAL;
    if (!finite_pos(e.voxel_size) || !finite_pos(e.trunc_voxels)) return IDH_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (!(fabsf(e.origin[i]) < INFINITY)) return IDH_EINVAL;
    if (!e.values) return IDH_EINVAL;
    if ((long long)e.Nz * e.Ny * e.Nx >= (1ll << 31) || e.Nz > 65535 || e.Ny > 262140) return IDH_EUNSUPPORTED;
    if (!e.block_flags || e.block_flag_bytes < 0 || (size_t)e.block_flag_bytes < idh_tsdf_block_flag_bytes(e.Nz, e.Ny, e.Nx)) return IDH_EWORKSPACE;
    V.values = e.values, V.flags = e.block_flags;
    V.ox = e.origin[0], V.oy = e.origin[1], V.oz = e.origin[2];
    V.v = e.voxel_size, V.trunc = e.trunc_voxels * e.voxel_size;
    V.Nx = e.Nx, V.Ny = e.Ny, V.Nz = e.Nz;
    V.nbx = tsdf_blocks(e.Nx), V.nby = tsdf_blocks(e.Ny), V.nbz = tsdf_blocks(e.Nz);
    return IDH_OK;
}

// ---- a sample of the volume: the ray cast (tsdf.hip) and the alignment (tsdf_align.hip) share one statement of it ----
typedef float f4a8 __attribute__((ext_vector_type(4), aligned(8)));  // two neighbouring {T, W} pairs: 8-byte aligned, one 16-byte load

__device__ __forceinline__ bool valid_depth(float d) { return d > 0.f && d < INFINITY; }  // false for NaN

// the eight corners of the cell at floor(g): false when the cell is outside the volume or a corner has W == 0
struct Corners {
    f4a8 a, b, c, d;  // rows (y, z) = (0,0), (1,0), (0,1), (1,1); each {T_x0, W_x0, T_x1, W_x1}
    float rx, ry, rz;
};

__device__ __forceinline__ bool cell_of(const Vol &V, float gx, float gy, float gz, float &fx, float &fy, float &fz) {
    fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
    return fx >= 0.f && fx <= (float)(V.Nx - 2) && fy >= 0.f && fy <= (float)(V.Ny - 2) && fz >= 0.f && fz <= (float)(V.Nz - 2);  // false for NaN
}

__device__ __forceinline__ bool load_corners(const Vol &V, float gx, float gy, float gz, float fx, float fy, float fz, Corners &c) {
    const int x = (int)fx, y = (int)fy, z = (int)fz;
    const size_t row = (size_t)V.Nx * 2, slice = row * V.Ny;
    const float *p = V.values + ((size_t)z * V.Ny + y) * row + (size_t)x * 2;
    c.a = *reinterpret_cast<const f4a8 *>(p);
    c.b = *reinterpret_cast<const f4a8 *>(p + row);
    c.c = *reinterpret_cast<const f4a8 *>(p + slice);
    c.d = *reinterpret_cast<const f4a8 *>(p + slice + row);
    c.rx = gx - fx, c.ry = gy - fy, c.rz = gz - fz;
    return c.a.y > 0.f && c.a.w > 0.f && c.b.y > 0.f && c.b.w > 0.f && c.c.y > 0.f && c.c.w > 0.f && c.d.y > 0.f && c.d.w > 0.f;
}

__device__ __forceinline__ float lerp(float a, float b, float r) { return a + r * (b - a); }

__device__ __forceinline__ float trilinear(const Corners &c) {
    const float a00 = lerp(c.a.x, c.a.z, c.rx), a10 = lerp(c.b.x, c.b.z, c.rx), a01 = lerp(c.c.x, c.c.z, c.rx), a11 = lerp(c.d.x, c.d.z, c.rx);
    return lerp(lerp(a00, a10, c.ry), lerp(a01, a11, c.ry), c.rz);
}

// the gradient of the interpolant in the cell, per voxel and in units of the truncation distance: the header's G
__device__ __forceinline__ void gradient(const Corners &c, float &Gx, float &Gy, float &Gz) {
    // rows: a = (y0,z0), b = (y1,z0), c = (y0,z1), d = (y1,z1); .x / .z are T at x0 / x1
    Gx = lerp(lerp(c.a.z - c.a.x, c.b.z - c.b.x, c.ry), lerp(c.c.z - c.c.x, c.d.z - c.d.x, c.ry), c.rz);
    Gy = lerp(lerp(c.b.x - c.a.x, c.b.z - c.a.z, c.rx), lerp(c.d.x - c.c.x, c.d.z - c.c.z, c.rx), c.rz);
    Gz = lerp(lerp(c.c.x - c.a.x, c.c.z - c.a.z, c.rx), lerp(c.d.x - c.b.x, c.d.z - c.b.z, c.rx), c.ry);
}

}  // namespace
