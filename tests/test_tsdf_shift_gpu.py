"""idh_tsdf_shift_fwd / TSDFVolume.shift / TSDFVolume.crop on the GPU (include/idh_fusion.h, csrc/tsdf.hip, implicit_depth_amd.fusion;
DESIGN.md §4.26).  Nothing is computed by a shift, so everything here is byte for byte: against the numpy statement of the header
(tests/tsdf_shift_ref.py), against idh_tsdf_flags_fwd, and - scrolling being invisible where nothing left - against the integrate
kernel on a larger volume that never moved."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import tsdf_ref as R
import tsdf_shift_ref as SR
from test_tsdf_shift_cpu import _random_volume

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
INT32_MIN = -2 ** 31
SENTINEL = 0x4D  # what the destination holds before a call: every byte of it must be written (or, for a refused call, kept)


def _cuda(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _same(t, ref):
    """A device tensor against a numpy array, byte for byte."""
    return np.array_equal(_bytes(t).cpu().numpy().reshape(-1), np.ascontiguousarray(ref).view(np.uint8).reshape(-1))


def _vol_struct(values, flags, origin, voxel_size, trunc_voxels=3.0):
    from implicit_depth_amd import _lib

    v = _lib.TsdfVolume()
    v.values, v.block_flags, v.block_flag_bytes = values.data_ptr(), flags.data_ptr(), flags.numel()
    v.origin[0], v.origin[1], v.origin[2] = (float(o) for o in origin)
    v.voxel_size, v.trunc_voxels = voxel_size, trunc_voxels
    v.Nz, v.Ny, v.Nx = values.shape[:3]
    return v


def _shift_args(values, flags, colors, origin, voxel_size, shift):
    """Arguments of a valid call and its destination tensors, filled with SENTINEL bytes."""
    from implicit_depth_amd import _lib

    dst = [torch.full_like(_bytes(values), SENTINEL).view(torch.float32).view(values.shape), torch.full_like(flags, SENTINEL),
           None if colors is None else torch.full_like(_bytes(colors), SENTINEL).view(torch.float32).view(colors.shape)]
    a = _lib.TsdfShiftArgs()
    a.src = _vol_struct(values, flags, origin, voxel_size)
    a.dst = _vol_struct(dst[0], dst[1], SR.shifted_origin(origin, voxel_size, shift), voxel_size)
    a.src_colors_zyx4, a.dst_colors_zyx4 = _lib.ptr(colors), _lib.ptr(dst[2])
    a.shift[0], a.shift[1], a.shift[2] = shift
    return a, dst


def _check_against_reference(values, flags, colors, origin, voxel_size, shift):
    """One call with colours and one without, both against the reference and against idh_tsdf_flags_fwd on a copy of the result."""
    from implicit_depth_amd import _lib, fusion

    want_v, want_c, want_f = SR.shift(values.cpu().numpy(), shift, colors.cpu().numpy())
    keep = [values.clone(), flags.clone(), colors.clone()]
    for with_colors in (True, False):
        a, dst = _shift_args(values, flags, colors if with_colors else None, origin, voxel_size, shift)
        assert _lib.lib().idh_tsdf_shift_fwd(C.byref(a), _lib.stream_ptr()) == 0
        assert _same(dst[0], want_v), (shift, with_colors)
        assert _same(dst[1], want_f), (shift, with_colors)
        if with_colors:
            assert _same(dst[2], want_c), shift
        rebuilt = fusion.TSDFVolume.from_values(dst[0].clone(), voxel_size, SR.shifted_origin(origin, voxel_size, shift))
        assert torch.equal(rebuilt.block_flags, dst[1]), (shift, with_colors)
    for t, k in zip((values, flags, colors), keep):
        assert torch.equal(_bytes(t), _bytes(k))  # the source is only read
    return want_v, want_f


# ---- 1. fused scenes against the reference --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fused_scene(scene):
    """(values, block_flags, colors) of a committed scene integrated on the GPU with random frames of the map size, on the host."""
    from implicit_depth_amd import fusion

    dims, v, origin, depth, K, E = R.scene_inputs(scene)
    frames = np.random.default_rng(5).integers(0, 256, (depth.shape[0], *depth.shape[2:], 3), dtype=np.uint8)
    vol = fusion.TSDFVolume(dims, v, origin, color=True)
    vol.integrate(_cuda(depth), _cuda(K), _cuda(E), _cuda(frames, torch.uint8))
    return vol.values.cpu().numpy(), vol.block_flags.cpu().numpy(), vol.colors.cpu().numpy()


SCENE_SHIFTS = {
    "x+1": lambda d: (1, 0, 0), "x-1": lambda d: (-1, 0, 0), "zero": lambda d: (0, 0, 0), "blocks": lambda d: (8, -8, 0),
    "odd": lambda d: (3, -5, 7), "odd2": lambda d: (-9, 11, -2), "z=Nz": lambda d: (0, 0, d[0]), "z=Nz-1": lambda d: (0, 0, d[0] - 1),
    "x=-(Nx-1)": lambda d: (-(d[2] - 1), 0, 0), "far": lambda d: (1000000, 0, 0), "int32_min": lambda d: (0, INT32_MIN, 0),
}


@pytest.mark.parametrize("scene", sorted(R.SCENES))
@pytest.mark.parametrize("case", list(SCENE_SHIFTS))
def test_fused_scene_matches_the_reference(scene, case):
    dims, v, origin = R.SCENES[scene][:3]
    shift = SCENE_SHIFTS[case](dims)
    values, flags, colors = (_cuda(x, dt) for x, dt in zip(_fused_scene(scene), (torch.float32, torch.uint8, torch.float32)))
    assert (values[..., 1] > 0).sum() > 1000 and (colors[..., 3] > 0).sum() > 100 and flags.any()
    want_v, want_f = _check_against_reference(values, flags, colors, R._f32(origin), v, shift)
    if case in ("z=Nz", "far", "int32_min"):
        assert not want_f.any() and (want_v[..., 1] == 0).all()
    elif case in ("x+1", "x-1", "zero", "blocks", "odd", "odd2"):  # (one slice of the room's edge may well be unobserved)
        assert want_f.any() and (want_v[..., 1] > 0).sum() > 100 and (want_v[..., 1] == 0).sum() > 100


# ---- 2. rows longer than a wave -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(63, 0, 0), (-65, 1, -1), (7, 0, 0)])
def test_rows_longer_than_a_wave(shift):
    from implicit_depth_amd import fusion

    dims = (10, 13, 75)
    values, colors = _random_volume(dims, 3, normalised=False)
    assert ((values[..., 1] == 0) & (values[..., 0] != 1)).sum() > 1000  # unobserved voxels that do not hold the empty state
    values, colors = _cuda(values), _cuda(colors)
    flags = fusion.TSDFVolume.from_values(values, 0.05, (0.1, 0.2, 0.3)).block_flags
    want_v, want_f = _check_against_reference(values, flags, colors, R._f32((0.1, 0.2, 0.3)), 0.05, shift)
    assert (want_v[..., 1] > 0).any() and (want_v[..., 1] == 0).any()


# ---- 3. scrolling is invisible where nothing left -------------------------------------------------------------------------------------
V = 0.0625
SMALL, SMALL_ORIGIN = (20, 28, 36), (-1.0, -0.75, 1.125)
BIG, BIG_ORIGIN = (36, 44, 52), (-1.5, -1.25, 0.625)  # 8 voxels lower on every axis: all voxel centres of both are exact in fp32
SCROLLS = ((8, 0, -8), (-3, 5, 2))


@functools.lru_cache(maxsize=None)
def _scrolled():
    """The small volume scrolled twice between three maps, and three big volumes that never move: one that integrated every map, one
    the last two, one the last alone."""
    from implicit_depth_amd import fusion

    _, _, _, depth, K, E = R.scene_inputs("room24x32")
    frames = np.random.default_rng(7).integers(0, 256, (3, 24, 32, 3), dtype=np.uint8)
    d, K, E, f = _cuda(depth), _cuda(K), _cuda(E), _cuda(frames, torch.uint8)
    small = fusion.TSDFVolume(SMALL, V, SMALL_ORIGIN, color=True)
    bigs = []
    for m in range(3):
        if m:
            small.shift(SCROLLS[m - 1])
        bigs.append(fusion.TSDFVolume(BIG, V, BIG_ORIGIN, color=True))
        for vol in [small] + bigs:
            vol.integrate(d[m:m + 1], K[m:m + 1], E[m:m + 1], f[m:m + 1])
    return small, bigs


def test_scrolling_is_invisible_where_nothing_left():
    small, bigs = _scrolled()
    assert small.origin == (-1.0 + V * 5, -0.75 + V * 5, 1.125 - V * 6)
    nz, ny, nx = SMALL
    # the three windows of the small volume in the big volume's voxel indices (x, y, z)
    w0 = np.array([8, 8, 8])
    w1, w2 = w0 + SCROLLS[0], w0 + SCROLLS[0] + SCROLLS[1]
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    big_idx = np.stack([xx, yy, zz], -1) + w2  # of every voxel of the small volume as it is now

    def inside(w):
        return ((big_idx >= w) & (big_idx < w + np.array([nx, ny, nz]))).all(-1)

    classes = {"stayed": inside(w0) & inside(w1), "entered at the first shift": ~inside(w0) & inside(w1), "entered at the second shift": ~inside(w1)}
    sv, sc = small.values.cpu().numpy(), small.colors.cpu().numpy()
    total = 0
    for (name, mask), big in zip(classes.items(), bigs):
        bv, bc = big.values.cpu().numpy(), big.colors.cpu().numpy()
        bx, by, bz = (big_idx[mask][:, i] for i in range(3))
        assert mask.sum() > 0 and bx.max() < BIG[2] and by.max() < BIG[1] and bz.max() < BIG[0] and min(bx.min(), by.min(), bz.min()) >= 0
        assert sv[mask].tobytes() == bv[bz, by, bx].tobytes(), name
        assert sc[mask].tobytes() == bc[bz, by, bx].tobytes(), name
        observed, coloured = int((sv[mask][:, 1] > 0).sum()), int((sc[mask][:, 3] > 0).sum())
        print(f"{name}: {int(mask.sum())} voxels, {observed} observed, {coloured} coloured")
        assert observed > 0
        total += int(mask.sum())
    assert total == nz * ny * nx
    assert (sv[classes["stayed"]][:, 1] >= 2).any() and (sc[..., 3] > 0).any()


# ---- 4. the rest of the library on a shifted volume -----------------------------------------------------------------------------------
def test_ray_cast_and_mesh_do_not_notice_the_flags_of_a_shifted_volume():
    from implicit_depth_amd import fusion

    small, _ = _scrolled()
    rebuilt = fusion.TSDFVolume.from_values(small.values.clone(), V, small.origin)
    assert torch.equal(rebuilt.block_flags, small.block_flags) and small.block_flags.any() and not small.block_flags.all()
    E, iK, H, W = R.live_camera("near", "30x44")
    kw = dict(near=R.NEAR, max_steps=R.max_steps_for(V), return_normals=True, return_color=True)
    a, b = (fusion.raycast_volume(small, _cuda(E), _cuda(iK), (H, W), skip=skip, **kw) for skip in (True, False))
    assert set(a) == set(b) == {"depth", "flags", "normals", "rgba"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert ((a["flags"] & R.HIT) > 0).float().mean().item() > 0.2
    m, n = (small.extract_mesh(use_block_flags=f, return_weights=True, return_colors=True) for f in (True, False))
    for k in m:
        assert torch.equal(m[k], n[k]), k
    assert m["verts"].shape[0] > 300 and m["faces"].shape[0] > 300


# ---- 5. determinism and ping-pong -----------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes_and_shift_reuses_its_spare():
    from implicit_depth_amd import _lib, fusion

    dims, v, origin = R.SCENES["room30x44"][:3]
    values, flags, colors = (_cuda(x, dt) for x, dt in zip(_fused_scene("room30x44"), (torch.float32, torch.uint8, torch.float32)))
    outs = []
    for _ in range(2):
        a, dst = _shift_args(values, flags, colors, R._f32(origin), v, (3, -5, 7))
        assert _lib.lib().idh_tsdf_shift_fwd(C.byref(a), _lib.stream_ptr()) == 0
        outs.append(dst)
    for x, y in zip(*outs):
        assert torch.equal(_bytes(x), _bytes(y))
    vol = fusion.TSDFVolume.from_values(values.clone(), v, origin, colors=colors.clone())
    first = (vol.values, vol.block_flags, vol.colors)
    ptrs = [tuple(t.data_ptr() for t in first)]
    vol.shift((3, -5, 7))
    second = (vol.values, vol.block_flags, vol.colors)
    ptrs.append(tuple(t.data_ptr() for t in second))
    assert not set(ptrs[0]) & set(ptrs[1])
    for x, y in zip(second, outs[0]):
        assert torch.equal(_bytes(x), _bytes(y))
    assert np.array_equal(np.asarray(vol.origin, np.float32), SR.shifted_origin(R._f32(origin), v, (3, -5, 7)))
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    for i, s in enumerate(((-3, 5, -7), (1, 0, 0), (0, 2, 0))):
        vol.shift(s)
        now = tuple(t.data_ptr() for t in (vol.values, vol.block_flags, vol.colors))
        assert now == ptrs[i % 2], (i, s)  # the two sets alternate
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held  # nothing new was allocated
    # there and back again: what never left is what it was (a reference taken before names a tensor that was overwritten since)
    once = SR.shift(values.cpu().numpy(), (3, -5, 7), colors.cpu().numpy())
    want_v, want_c, want_f = SR.shift(once[0], (-3, 5, -7), once[1])
    back = fusion.TSDFVolume.from_values(values.clone(), v, origin, colors=colors.clone())
    back.shift((3, -5, 7))
    back.shift((-3, 5, -7))
    assert _same(back.values, want_v) and _same(back.colors, want_c) and _same(back.block_flags, want_f)
    there = SR.shifted_origin(R._f32(origin), v, (3, -5, 7))
    assert np.array_equal(np.asarray(back.origin, np.float32), SR.shifted_origin(there, v, (-3, 5, -7)))  # (fp32 sums: not always the first origin)
    with pytest.raises(_lib.IdhError):
        vol.shift((1, 2))
    with pytest.raises(_lib.IdhError):
        vol.shift((2 ** 31, 0, 0))


# ---- 6. error codes -------------------------------------------------------------------------------------------------------------------
def test_error_codes_in_the_headers_order():
    from implicit_depth_amd import _lib, fusion

    L = _lib.lib()
    dims, v, origin = (9, 10, 11), 0.05, R._f32((0.1, -0.2, 0.3))
    values, colors = (_cuda(x) for x in _random_volume(dims, 4, normalised=True))
    flags = fusion.TSDFVolume.from_values(values, v, origin).block_flags
    assert flags.numel() == 4  # 1 x 2 x 2 blocks
    shift = (1, -2, 3)
    good, dst = _shift_args(values, flags, colors, origin, v, shift)
    keep = [t.clone() for t in (values, flags, colors, *dst)]

    def call(**kw):
        """The valid call with fields replaced: ``src__Nz=3`` sets a.src.Nz, ``shift=(..)`` the shift, the rest fields of the struct."""
        a = _lib.TsdfShiftArgs()
        C.memmove(C.byref(a), C.byref(good), C.sizeof(a))
        for k, val in kw.items():
            if k == "shift":
                a.shift[0], a.shift[1], a.shift[2] = val
            elif "__" in k:
                which, field = k.split("__")
                if field == "origin":
                    getattr(a, which).origin[0], getattr(a, which).origin[1], getattr(a, which).origin[2] = val
                else:
                    setattr(getattr(a, which), field, val)
            else:
                setattr(a, k, val)
        return L.idh_tsdf_shift_fwd(C.byref(a), _lib.stream_ptr())

    assert L.idh_tsdf_shift_fwd(None, None) == EINVAL
    assert call(struct_size=C.sizeof(_lib.TsdfShiftArgs) - 1) == EINVAL
    # the colour pointers come before the volumes: with a volume condition that has another code, EINVAL wins
    broken = dict(src__block_flags=None)
    assert call(**broken) == EWORKSPACE
    assert call(src_colors_zyx4=None, **broken) == EINVAL and call(dst_colors_zyx4=None, **broken) == EINVAL
    assert call(src_colors_zyx4=None) == EINVAL and call(dst_colors_zyx4=None) == EINVAL
    assert call(src_colors_zyx4=colors.data_ptr() + 4, **broken) == EINVAL and call(dst_colors_zyx4=dst[2].data_ptr() + 8, **broken) == EINVAL
    assert call(src_colors_zyx4=colors.data_ptr() + 4) == EINVAL and call(dst_colors_zyx4=dst[2].data_ptr() + 8) == EINVAL
    # src's conditions, then dst's, each with check_volume's codes in its order
    huge = dict(Nz=65536, Ny=2, Nx=2)
    for which, other in (("src", "dst"), ("dst", "src")):
        p = which + "__"
        for kw, code in ((dict(struct_size=8), EINVAL), (dict(Nz=1), EINVAL), (dict(Nx=-4), EINVAL), (dict(voxel_size=0.0), EINVAL),
                         (dict(trunc_voxels=float("nan")), EINVAL), (dict(origin=(float("nan"), 0.0, 0.0)), EINVAL), (dict(values=None), EINVAL),
                         (huge, EUNSUPPORTED), (dict(Nz=2, Ny=262141, Nx=2), EUNSUPPORTED), (dict(block_flags=None), EWORKSPACE),
                         (dict(block_flag_bytes=3), EWORKSPACE), (dict(block_flag_bytes=-1), EWORKSPACE)):
            assert call(**{p + k: val for k, val in kw.items()}) == code, (which, kw)
        # inside one volume: EINVAL before EUNSUPPORTED before EWORKSPACE
        assert call(**{p + "values": None, p + "block_flags": None, **{p + k: val for k, val in huge.items()}}) == EINVAL
        assert call(**{p + "block_flags": None, **{p + k: val for k, val in huge.items()}}) == EUNSUPPORTED
    assert call(src__block_flags=None, dst__Nz=65536, dst__Ny=2, dst__Nx=2) == EWORKSPACE  # src first
    assert call(src__Nz=65536, src__Ny=2, src__Nx=2, dst__block_flags=None) == EUNSUPPORTED
    # the volumes' conditions come before what the two must share
    assert call(dst__block_flags=None, dst__Nz=8) == EWORKSPACE and call(dst__block_flags=None, shift=(0, 0, 0)) == EWORKSPACE
    # dims, voxel_size, trunc_voxels
    assert call(dst__Nz=8) == EINVAL and call(dst__Ny=9) == EINVAL and call(src__Nx=10) == EINVAL
    assert call(dst__voxel_size=float(np.nextafter(np.float32(v), np.float32(1)))) == EINVAL
    assert call(dst__trunc_voxels=2.5) == EINVAL and call(src__trunc_voxels=float(np.nextafter(np.float32(3), np.float32(4)))) == EINVAL
    # the origin, bit for bit
    want = SR.shifted_origin(origin, v, shift)
    for i in range(3):
        for towards in (-np.inf, np.inf):
            off = want.copy()
            off[i] = np.nextafter(want[i], np.float32(towards))
            assert call(dst__origin=tuple(float(o) for o in off)) == EINVAL, (i, towards)
    assert call(dst__origin=tuple(float(o) for o in origin)) == EINVAL  # the data moved, the frame did not
    assert call(shift=(1, -2, 4)) == EINVAL and call(shift=(0, 0, 0)) == EINVAL
    # overlaps: never in place
    zero = dict(shift=(0, 0, 0), dst__origin=tuple(float(o) for o in origin))
    assert call(dst__values=values.data_ptr(), **zero) == EINVAL
    assert call(dst__values=values.data_ptr()) == EINVAL
    assert call(dst__values=values.data_ptr() + 8 * (values.numel() // 2 - 1)) == EINVAL  # the last pair of src
    assert call(dst__block_flags=values.data_ptr() + 64) == EINVAL  # dst's flags inside src's values
    assert call(dst__block_flags=flags.data_ptr()) == EINVAL and call(dst__block_flags=flags.data_ptr() + 3) == EINVAL
    assert call(dst__block_flags=colors.data_ptr() + 16) == EINVAL
    assert call(dst_colors_zyx4=colors.data_ptr()) == EINVAL and call(dst_colors_zyx4=values.data_ptr()) == EINVAL
    assert call(src__block_flags=dst[0].data_ptr() + 128) == EINVAL  # src's flags inside dst's values
    assert call(src__values=dst[2].data_ptr()) == EINVAL
    # every refused call left the six buffers as they were
    for t, k in zip((values, flags, colors, *dst), keep):
        assert torch.equal(_bytes(t), _bytes(k))
    assert (_bytes(dst[0]) == SENTINEL).all() and (dst[1] == SENTINEL).all()
    # and the calls they were made from are valid
    assert call(**zero) == 0 and _same(dst[0], keep[0].cpu().numpy()) and _same(dst[2], keep[2].cpu().numpy())  # (the volume is normalised)
    assert call() == 0
    want_v, want_c, want_f = SR.shift(keep[0].cpu().numpy(), shift, keep[2].cpu().numpy())
    assert _same(dst[0], want_v) and _same(dst[1], want_f) and _same(dst[2], want_c)
    assert call(src_colors_zyx4=None, dst_colors_zyx4=None) == 0


# ---- 7. crop --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [((0, 0, 0), (35, 27, 19)), ((3, 5, 7), (20, 14, 9)), ((30, 0, 2), (35, 27, 3)), ((8, 8, 8), (16, 16, 16))])
def test_crop(lo, hi):
    from implicit_depth_amd import _lib, fusion

    dims, v, origin = R.SCENES["room24x32"][:3]
    values, flags, colors = _fused_scene("room24x32")
    vol = fusion.TSDFVolume.from_values(_cuda(values), v, origin, colors=_cuda(colors))
    part = vol.crop(lo, hi)
    box = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
    assert part.dims == tuple(h - l + 1 for l, h in zip(lo[::-1], hi[::-1])) and part.values.is_contiguous() and part.colors.is_contiguous()
    assert _same(part.values, values[box]) and _same(part.colors, colors[box])
    assert _same(part.block_flags, R.block_flags(values[box])[0])
    assert np.array_equal(np.asarray(part.origin, np.float32), SR.shifted_origin(R._f32(origin), v, lo))
    assert (part.voxel_size, part.trunc_voxels, part.max_weight) == (vol.voxel_size, vol.trunc_voxels, vol.max_weight)
    assert part.values.data_ptr() != vol.values.data_ptr() and part.colors.data_ptr() != vol.colors.data_ptr()  # a copy
    part.reset()
    assert _same(vol.values, values) and _same(vol.colors, colors)
    bare = fusion.TSDFVolume.from_values(_cuda(values), v, origin).crop(lo, hi)
    assert bare.colors is None and _same(bare.values, values[box])
    for bad in (((0, 0, 0), (36, 27, 19)), ((-1, 0, 0), (5, 5, 5)), ((4, 4, 4), (4, 9, 9)), ((0, 0), (5, 5, 5))):
        with pytest.raises(_lib.IdhError):
            vol.crop(*bad)
