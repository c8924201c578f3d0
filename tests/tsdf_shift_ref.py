"""numpy statement of idh_tsdf_shift_fwd (include/idh_fusion.h, "A volume that follows the camera"), written from the
header and independent of the kernel.  Nothing is computed: pairs and quads are moved or replaced by the empty state, so every result is
compared byte for byte.  The flags are the header's rule as tests/tsdf_ref.py states it."""
import numpy as np

import tsdf_ref as R


def shift(values, shift_xyz, colors=None):
    """``values`` (Nz,Ny,Nx,2) float32, ``colors`` (Nz,Ny,Nx,4) float32 or None, ``shift_xyz`` any Python ints.  Returns
    (values, colors or None, flags (NBz,NBy,NBx) uint8) of the destination volume."""
    values = np.asarray(values)
    assert values.dtype == np.float32 and values.shape[3] == 2
    Nz, Ny, Nx = values.shape[:3]
    sx, sy, sz = (int(k) for k in shift_xyz)  # Python ints: x + sx cannot overflow
    out = R.empty_volume((Nz, Ny, Nx))
    out_c = None if colors is None else np.zeros((Nz, Ny, Nx, 4), np.float32)
    # destination voxels whose source a = (x + sx, y + sy, z + sz) is inside: per axis the range lo .. hi - 1
    rng = [(max(0, -s), min(n, n - s)) for s, n in ((sz, Nz), (sy, Ny), (sx, Nx))]
    if all(lo < hi for lo, hi in rng):
        dst = tuple(slice(lo, hi) for lo, hi in rng)
        src = tuple(slice(lo + s, hi + s) for (lo, hi), s in zip(rng, (sz, sy, sx)))
        seen = values[src][..., 1] > 0  # false for NaN
        out[dst] = np.where(seen[..., None], values[src], out[dst])
        if colors is not None:
            c = np.asarray(colors)
            assert c.dtype == np.float32 and c.shape == (Nz, Ny, Nx, 4)
            out_c[dst] = np.where(seen[..., None], c[src], out_c[dst])
    return out, out_c, R.block_flags(out)[0]


def shifted_origin(origin, voxel_size, shift_xyz):
    """dst.origin as the header demands it: one fp32 multiply, one fp32 add per axis."""
    v = np.float32(voxel_size)
    return np.array([np.float32(o) + v * np.float32(int(k)) for o, k in zip(origin, shift_xyz)], np.float32)
