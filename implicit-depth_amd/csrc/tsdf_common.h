// What the TSDF kernels share (tsdf.hip, tsdf_mesh.hip): the volume as the kernels take it, and the host-side check of an
// idh_tsdf_volume in the order include/idh_fusion.h states.
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

}  // namespace
