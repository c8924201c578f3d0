"""The host side of the volume that follows the camera (implicit_depth_amd.fusion.leaving_boxes / follow_shift), the
numpy reference the GPU tests compare against (tests/tsdf_shift_ref.py) and the ctypes mirror of idh_tsdf_shift_args.  No GPU."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import tsdf_ref as R
import tsdf_shift_ref as SR

DIMS = (5, 6, 7)  # (Nz, Ny, Nx)
SHIFTS = (-8, -2, -1, 0, 1, 3, 7)


def _dropped(dims, shift):
    """Brute force: the voxels a of the current volume with a - s outside the volume, as a (Nz,Ny,Nx) mask."""
    nz, ny, nx = dims
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    dx, dy, dz = xx - shift[0], yy - shift[1], zz - shift[2]
    stays = (dx >= 0) & (dx < nx) & (dy >= 0) & (dy < ny) & (dz >= 0) & (dz < nz)
    return ~stays


def test_leaving_boxes_cover_exactly_what_a_shift_drops():
    from implicit_depth_amd import fusion

    nz, ny, nx = DIMS
    n = 0
    for s in itertools.product(SHIFTS, repeat=3):
        boxes = fusion.leaving_boxes(DIMS, s)
        want = _dropped(DIMS, s)
        count = np.zeros(DIMS, np.int64)
        for lo, hi in boxes:
            assert len(lo) == 3 and len(hi) == 3
            assert all(0 <= a <= b < m for a, b, m in zip(lo, hi, (nx, ny, nz))), (s, lo, hi)  # inside the volume, not empty
            count[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] += 1
        assert count.max() <= 1, s  # disjoint
        assert np.array_equal(count > 0, want), s
        assert len(boxes) <= 3
        whole = ((0, 0, 0), (nx - 1, ny - 1, nz - 1))
        if s == (0, 0, 0):
            assert boxes == []
        elif any(abs(k) >= m for k, m in zip(s, (nx, ny, nz))):
            assert boxes == [whole], s
        else:
            # the order: the x slab over all y and z, then the y slab over the x that stay, then the z slab over the x and y that stay
            stay = [(max(k, 0), m - 1 + min(k, 0)) for k, m in zip(s, (nx, ny, nz))]
            axes = [i for i in range(3) if s[i] != 0]
            assert len(boxes) == len(axes)
            for (lo, hi), axis in zip(boxes, axes):
                for i in range(3):
                    if i < axis:
                        assert (lo[i], hi[i]) == stay[i], (s, axis, i)
                    elif i > axis:
                        assert (lo[i], hi[i]) == (0, (nx, ny, nz)[i] - 1), (s, axis, i)
                    else:
                        assert (lo[i], hi[i]) == ((0, s[i] - 1) if s[i] > 0 else ((nx, ny, nz)[i] + s[i], (nx, ny, nz)[i] - 1)), (s, axis)
        n += 1
    assert n == 7 ** 3


def test_follow_shift():
    from implicit_depth_amd import fusion

    dims, v = (24, 32, 40), 0.0625  # centre of the grid at origin + v * (39, 31, 23) / 2: exact in binary
    origin = np.array([-1.0, 0.5, 2.0])
    centre = origin + v * (np.array([40, 32, 24]) - 1) / 2
    slack = 0.5  # 8 voxels
    assert fusion.follow_shift(centre, origin, dims, v, slack) == (0, 0, 0)
    # inside the slack, and exactly on it, nothing moves; one ulp beyond it does
    assert fusion.follow_shift(centre + [0.4375, -0.4375, 0.25], origin, dims, v, slack) == (0, 0, 0)
    assert fusion.follow_shift(centre + [0.5, -0.5, 0.5], origin, dims, v, slack) == (0, 0, 0)
    beyond = centre.copy()
    beyond[0] = np.nextafter(centre[0] + 0.5, np.inf)
    assert fusion.follow_shift(beyond, origin, dims, v, slack) == (8, 0, 0)
    # one axis beyond the slack moves every axis to its nearest block; negative directions
    assert fusion.follow_shift(centre + [0.75, 0.0, 0.0], origin, dims, v, slack) == (16, 0, 0)  # 12 voxels: 8 * floor(1.5 + 0.5)
    assert fusion.follow_shift(centre + [-0.5625, 0.0, 0.0], origin, dims, v, slack) == (-8, 0, 0)
    assert fusion.follow_shift(centre + [0.0, -0.75, 0.0], origin, dims, v, slack) == (0, -8, 0)  # -12 voxels: 8 * floor(-1.5 + 0.5)
    assert fusion.follow_shift(centre + [0.625, -0.3125, -0.25], origin, dims, v, slack) == (8, -8, 0)  # (10, -5, -4) voxels
    assert fusion.follow_shift(centre + [0.0, 0.0, -3.0], origin, dims, v, slack) == (0, 0, -48)
    rng = np.random.default_rng(0)
    moved = 0
    for _ in range(500):
        cam = centre + rng.uniform(-1.0, 1.0, 3)  # 16 voxels either way: one draw in eight stays inside the slack
        s = fusion.follow_shift(cam, origin, dims, v, slack)
        c = (cam - centre) / v
        assert all(isinstance(k, int) and k % 8 == 0 for k in s)
        if (np.abs(c) > slack / v).any():
            assert np.abs(c - np.array(s)).max() <= 4.0, (cam, s)  # the camera ends within 4 voxels of the new centre
            # and the new centre is where the shifted origin puts it
            new_centre = (origin + v * np.array(s)) + v * (np.array([40, 32, 24]) - 1) / 2
            assert np.abs((cam - new_centre) / v).max() <= 4.0
            moved += 1
        else:
            assert s == (0, 0, 0)
    assert 100 < moved < 500


def _random_volume(dims, seed, normalised):
    rng = np.random.default_rng(seed)
    values = np.empty((*dims, 2), np.float32)
    values[..., 1] = rng.choice(np.array([0, 0, 0, 1, 2.5], np.float32), size=dims)
    values[..., 0] = rng.uniform(-1, 1, dims).astype(np.float32)
    colors = rng.uniform(0, 255, (*dims, 4)).astype(np.float32)
    if normalised:
        empty = values[..., 1] == 0
        values[empty, 0] = 1
        colors[empty] = 0
    return values, colors


def test_reference_identity_normalisation_and_emptying():
    dims = (9, 10, 11)
    values, colors = _random_volume(dims, 1, normalised=True)
    v, c, f = SR.shift(values, (0, 0, 0), colors)
    assert v.tobytes() == values.tobytes() and c.tobytes() == colors.tobytes()
    assert np.array_equal(f, R.block_flags(values)[0]) and f.any()
    # W == 0 voxels that hold something else come back empty
    dirty, dirty_c = values.copy(), colors.copy()
    empty = values[..., 1] == 0
    dirty[empty, 0] = np.float32(0.3)
    dirty_c[empty] = 7
    assert empty.sum() > 100
    v, c, f = SR.shift(dirty, (0, 0, 0), dirty_c)
    assert v.tobytes() == values.tobytes() and c.tobytes() == colors.tobytes()
    assert (v[empty] == np.array([1, 0], np.float32)).all()
    # a plain move: what stays is where it was in the world, what comes in is empty
    v, c, f = SR.shift(values, (2, -3, 1), colors)
    assert v[0:8, 3:10, 0:9].tobytes() == values[1:9, 0:7, 2:11].tobytes() and c[0:8, 3:10, 0:9].tobytes() == colors[1:9, 0:7, 2:11].tobytes()
    outside = np.ones(dims, bool)
    outside[0:8, 3:10, 0:9] = False
    assert (v[outside] == np.array([1, 0], np.float32)).all() and (c[outside] == 0).all()
    assert np.array_equal(f, R.block_flags(v)[0])
    # a whole dim or more on an axis: the empty volume and all-zero flags
    for s in ((11, 0, 0), (0, -10, 0), (0, 0, 9), (2 ** 31 - 1, 0, 0), (0, -2 ** 31, 0), (1000000, 2, -3)):
        v, c, f = SR.shift(values, s, colors)
        assert v.tobytes() == R.empty_volume(dims).tobytes() and not c.any() and not f.any(), s
    v, c, f = SR.shift(values, (1, 1, 1))
    assert c is None
    assert SR.shifted_origin((-1.0, -0.75, 1.125), 0.0625, (8, 0, -8)).tolist() == [-0.5, -0.75, 0.625]


def test_struct_mirror_matches_the_library():
    from implicit_depth_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    h = ctypes.CDLL(_lib.LIB_PATH)
    h.idh_sizeof_tsdf_shift_args.restype = ctypes.c_size_t
    assert ctypes.sizeof(_lib.TsdfShiftArgs) == h.idh_sizeof_tsdf_shift_args() == _lib.TsdfShiftArgs().struct_size
    assert hasattr(h, "idh_tsdf_shift_fwd") and "idh_tsdf_shift_fwd" in _lib.declared_symbols()
    # argument validation happens before any launch: safe without a GPU
    L = _lib.lib()
    assert L.idh_tsdf_shift_fwd(None, None) == -1
    a = _lib.TsdfShiftArgs()
    a.struct_size -= 1
    assert L.idh_tsdf_shift_fwd(ctypes.byref(a), None) == -1
