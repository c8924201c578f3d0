"""TSDF fusion on the GPU (include/idh_fusion.h, csrc/tsdf.hip, implicit_depth_amd.fusion) against the fp64 reference of
tests/tsdf_ref.py outside what that reference calls ambiguous (at most 1 % of the touched voxels, 1 % of the pixels: test_tsdf_cpu.py),
the bit-level promises of the header, closed forms, and the two things the fusion exists for: maps are combined, holes are filled."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import tsdf_ref as R

pytestmark = pytest.mark.gpu


def _cuda(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _volume(name, **kw):
    from implicit_depth_amd import fusion

    dims, v, origin = R.SCENES[name][:3]
    return fusion.TSDFVolume(dims, v, origin, **kw)


def _integrate(name, M=None, max_weight=64.0, calls=1):
    """The scene's maps into a fresh volume, in ``calls`` = 1 call or one call per map."""
    dims, v, origin, depth, K, E = R.scene_inputs(name, M)
    vol = _volume(name, max_weight=max_weight)
    d, K, E = _cuda(depth), _cuda(K), _cuda(E)
    if calls == 1:
        vol.integrate(d, K, E)
    else:
        for m in range(d.shape[0]):
            vol.integrate(d[m:m + 1], K[m:m + 1], E[m:m + 1])
    return vol


@functools.lru_cache(maxsize=None)
def _fused_values(name):
    """The GPU's fused float32 volume of a scene on the host: what both the kernel and the reference ray-cast."""
    return _integrate(name).values.cpu().numpy()


@pytest.mark.parametrize("name", sorted(R.SCENES))
@pytest.mark.parametrize("M,max_weight", [(1, 64.0), (None, 64.0), (None, 2.0)])
def test_integrate_matches_fp64(name, M, max_weight):
    ref = R.scene_integrated(name, M, max_weight)
    vol = _integrate(name, M, max_weight)
    got = vol.values.cpu().numpy()
    ok = ~ref["ambiguous"]
    assert (ref["touched"] & ~ok).sum() <= R.CAP * ref["touched"].sum()
    assert (got[..., 1][ok] == ref["W"][ok]).all()
    err = np.abs(got[..., 0] - ref["T"])[ok].max()
    print(f"{name} M={M} max_weight={max_weight}: max |T - T_ref| = {err:.2e} over {ok.sum()} voxels, W max {got[..., 1].max()}")
    assert err < 1e-4
    untouched = ok & ~ref["touched"]
    assert (got[..., 0][untouched] == 1).all() and (got[..., 1][untouched] == 0).all()
    assert got[..., 1].max() == (1 if M == 1 else min(R.SCENES[name][5], max_weight))
    # the flags the kernel kept are the header's
    seen, _ = R.block_flags(got)
    assert np.array_equal(vol.block_flags.cpu().numpy().reshape(seen.shape), seen)


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_integrate_bits(name):
    from implicit_depth_amd import fusion

    one, again, three = _integrate(name), _integrate(name), _integrate(name, calls=3)
    assert torch.equal(one.values, again.values) and torch.equal(one.block_flags, again.block_flags)
    assert torch.equal(one.values, three.values) and torch.equal(one.block_flags, three.block_flags)
    # a map of invalid taps changes nothing; nor does it set a flag in an empty volume
    dims, v, origin, depth, K, E = R.scene_inputs(name, 1)
    bad = np.full_like(depth, np.nan)
    bad[0, 0, ::2] = 0.0
    bad[0, 0, 1::3] = -2.0
    bad[0, 0, 2, 3] = np.inf
    before, flags = one.values.clone(), one.block_flags.clone()
    one.integrate(_cuda(bad), _cuda(K), _cuda(E))
    assert torch.equal(one.values, before) and torch.equal(one.block_flags, flags)
    empty = _volume(name)
    empty.integrate(_cuda(bad), _cuda(K), _cuda(E))
    assert not empty.block_flags.any() and (empty.values[..., 0] == 1).all() and (empty.values[..., 1] == 0).all()
    # from_values rebuilds the flags integrate kept; reset empties both
    adopted = fusion.TSDFVolume.from_values(three.values.clone(), v, origin)
    assert torch.equal(adopted.block_flags, three.block_flags) and adopted.block_flags.any() and not adopted.block_flags.all()
    three.reset()
    assert not three.block_flags.any() and (three.values[..., 0] == 1).all() and (three.values[..., 1] == 0).all()


def _raycast(values, scene, pose, cam, **kw):
    from implicit_depth_amd import fusion

    dims, v, origin = R.SCENES[scene][:3]
    vol = fusion.TSDFVolume.from_values(_cuda(values), v, origin)
    E, iK, H, W = R.live_camera(pose, cam)
    kw.setdefault("near", R.NEAR)
    kw.setdefault("max_steps", R.max_steps_for(v, kw.get("step_voxels", 1.0)))
    return fusion.raycast_volume(vol, _cuda(E), _cuda(iK), (H, W), **kw)


@pytest.mark.parametrize("scene,pose,cam", R.RAYCAST_CASES)
@pytest.mark.parametrize("world_normals", [True, False])
def test_raycast_matches_fp64_on_the_same_volume(scene, pose, cam, world_normals):
    values = _fused_values(scene)
    dims, v, origin = R.SCENES[scene][:3]
    E, iK, H, W = R.live_camera(pose, cam)
    ref = R.raycast(values, origin, v, E, iK, H, W, near=R.NEAR, max_steps=R.max_steps_for(v), world_normals=world_normals)
    out = _raycast(values, scene, pose, cam, return_normals=True, world_normals=world_normals)
    depth, flags, normals = out["depth"][0, 0].cpu().numpy().astype(np.float64), out["flags"][0].cpu().numpy(), out["normals"][0].cpu().numpy()
    ok = ~ref["ambiguous"]
    assert (~ok).sum() <= R.CAP * H * W
    assert ((flags & 7) == (ref["flags"] & 7))[ok].all()
    hit = ok & ((ref["flags"] & R.HIT) > 0)
    rel = (np.abs(depth - ref["depth"]) / np.abs(ref["depth"]))[hit].max()
    assert hit.sum() > 0.2 * H * W and rel < 1e-4
    assert (depth[ok & ~hit] == -1.0).all()
    nok = hit & ~ref["normal_ambiguous"]
    assert nok.sum() > 0.9 * hit.sum()
    assert ((flags & R.NO_NORMAL) == (ref["flags"] & R.NO_NORMAL))[nok].all()
    both = nok & ((ref["flags"] & R.NO_NORMAL) == 0)
    nerr = np.abs(normals - ref["normals"])[:, both].max()
    print(f"{scene} {pose} {cam} world_normals={world_normals}: {hit.sum()} hits, max relative depth error {rel:.2e}, "
          f"max normal component error {nerr:.2e} over {both.sum()} pixels")
    assert nerr < 1e-3
    assert (normals[:, ok & ~hit] == 0).all()
    # without normals: the same depth and flags (bit 8 aside)
    plain = _raycast(values, scene, pose, cam)
    assert set(plain) == {"depth", "flags"} and torch.equal(plain["depth"], out["depth"]) and torch.equal(plain["flags"], out["flags"] & 7)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("scene,pose,cam", R.RAYCAST_CASES)
@pytest.mark.parametrize("step_voxels", [1.0, 0.37])
def test_skip_returns_the_bits_of_the_plain_march(scene, pose, cam, step_voxels):
    values = _fused_values(scene)
    kw = dict(return_normals=True, step_voxels=step_voxels)
    a, b = _raycast(values, scene, pose, cam, skip=True, **kw), _raycast(values, scene, pose, cam, skip=False, **kw)
    _same(a, b)
    assert 0 < ((a["flags"] & R.HIT) > 0).sum() < a["flags"].numel()
    _same(_raycast(values, scene, pose, cam, skip=True, near=0.0, max_steps=300, step_voxels=step_voxels),
          _raycast(values, scene, pose, cam, skip=False, near=0.0, max_steps=300, step_voxels=step_voxels))


@pytest.mark.parametrize("corner", [(0, 0, 0), (1, 1, 1), (0, 1, 0)])
def test_skip_on_a_volume_with_one_flagged_block_in_a_corner(corner):
    from implicit_depth_amd import fusion

    dims, v, origin = R.SCENES["room24x32"][:3]
    values = R.empty_volume(dims)
    box = tuple(slice(0, 7) if c == 0 else slice(d - 3, d) for c, d in zip(corner, dims))  # inside one block, clear of its apron
    sub = values[box]
    zz, yy, xx = np.meshgrid(*(np.arange(n) for n in sub.shape[:3]), indexing="ij")
    sub[..., 0] = np.clip(0.9 - 0.45 * zz + 0.07 * xx - 0.05 * yy, -1, 1)  # a surface across the box, seen from -z
    sub[..., 1] = 1
    vol = fusion.TSDFVolume.from_values(_cuda(values), v, origin)
    assert int(vol.block_flags.sum()) == 1
    for pose, cam in (("near", "30x44"), ("side", "24x32")):
        a, b = (_raycast(values, "room24x32", pose, cam, skip=s, return_normals=True) for s in (True, False))
        _same(a, b)


def test_two_cameras_equal_two_calls_and_empty_depth_moves_only_the_empties():
    from implicit_depth_amd import fusion

    scene = "room24x32"
    values = _fused_values(scene)
    dims, v, origin = R.SCENES[scene][:3]
    vol = fusion.TSDFVolume.from_values(_cuda(values), v, origin)
    cams = [R.live_camera(p, "24x32") for p in ("near", "side")]
    E, iK = _cuda(np.stack([c[0] for c in cams])), _cuda(np.stack([c[1] for c in cams]))
    kw = dict(near=R.NEAR, max_steps=R.max_steps_for(v), return_normals=True)
    both = fusion.raycast_volume(vol, E, iK, (24, 32), **kw)
    for b in range(2):
        one = fusion.raycast_volume(vol, E[b], iK[b], (24, 32), **kw)
        for k in one:
            assert torch.equal(one[k][0], both[k][b]), (b, k)
    moved = fusion.raycast_volume(vol, E, iK, (24, 32), empty_depth=7.5, **kw)
    hit = (both["flags"] & R.HIT) > 0
    assert torch.equal(moved["flags"], both["flags"]) and torch.equal(moved["normals"], both["normals"])
    assert torch.equal(moved["depth"][:, 0][hit], both["depth"][:, 0][hit])
    assert (moved["depth"][:, 0][~hit] == 7.5).all() and (both["depth"][:, 0][~hit] == -1.0).all() and 0 < hit.sum() < hit.numel()
    # TSDFVolume.raycast derives max_steps from near / far on the host
    a = vol.raycast(E, iK, (24, 32), near=R.NEAR, far=R.FAR, return_normals=True)
    _same(a, both)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
PLANE_D = 1.62
PLANE_POSE = R._pose(0.06, -0.05, 0.03, (0.02, 0.03, -0.01))  # camera A, nearly along the world's z but not aligned with the grid
PLANE_K = R._pinhole(28.9, 28.4, 15.6, 12.3)


def _plane_setup(depths, trunc_voxels):
    """Constant maps (fronto-parallel planes) seen by camera A into the 24x32 room's grid; returns the volume."""
    from implicit_depth_amd import fusion

    dims, v, origin = R.SCENES["room24x32"][:3]
    vol = fusion.TSDFVolume(dims, v, origin, trunc_voxels=trunc_voxels)
    M = len(depths)
    d = np.stack([np.full((1, 24, 32), x, np.float32) for x in depths])
    vol.integrate(_cuda(d), _cuda(np.stack([PLANE_K] * M)), _cuda(np.stack([np.linalg.inv(PLANE_POSE)] * M)))
    return vol, d


def _plane_in_camera_b(pose, cam, D, margin_px, margin_vox):
    """fp64: the depth in live camera B of the plane z_A = D, and the pixels whose hit lies ``margin_px`` inside A's image and
    ``margin_vox`` voxels inside the grid."""
    dims, v, origin = R.SCENES["room24x32"][:3]
    E, iK, H, W = R.live_camera(pose, cam)
    E, iK = E.astype(np.float64), iK.astype(np.float64)
    A = np.linalg.inv(_f32_64(np.linalg.inv(PLANE_POSE)))  # world_T_A as the kernel's float32 cam_T_world implies
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    q = np.stack([jj + 0.5, ii + 0.5, np.ones((H, W))], -1) @ iK[:3, :3].T
    dirw = q @ E[:3, :3].T  # per unit of camera z
    n, a0 = A[:3, 2], A[:3, 3]  # the plane: n . (X - a0) = D
    z = (D - n @ (E[:3, 3] - a0)) / (dirw @ n)
    X = E[:3, 3] + z[..., None] * dirw
    XA = (X - a0) @ A[:3, :3]
    u, w_ = PLANE_K[0, 0] * XA[..., 0] / XA[..., 2] + PLANE_K[0, 2], PLANE_K[1, 1] * XA[..., 1] / XA[..., 2] + PLANE_K[1, 2]
    g = (X - np.asarray(origin, np.float32).astype(np.float64)) / float(np.float32(v))
    hi = np.array([dims[2], dims[1], dims[0]]) - 1
    inside = (z > 0) & (u > margin_px) & (u < 32 - margin_px) & (w_ > margin_px) & (w_ < 24 - margin_px)
    inside &= ((g > margin_vox) & (g < hi - margin_vox)).all(-1)
    return z, inside


def _f32_64(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def test_plane_seen_by_one_camera_is_hit_on_the_plane_from_another():
    """sdf = D - z_A is linear in space, so the TSDF is exactly linear in the band and trilinear interpolation reproduces it: the hit
    lies on the plane.  Samples k - 1 and k read corners at most 1 + sqrt(3) < 3 voxels from the crossing: inside the band."""
    from implicit_depth_amd import fusion

    vol, _ = _plane_setup([PLANE_D], 3.0)
    v = vol.voxel_size
    # margins: the corners of the two bracketing samples lie within 2.8 voxels of the hit: 2.8 v * fx / D = 2.5 px in camera A
    want, inside = _plane_in_camera_b("near", "30x44", PLANE_D, margin_px=3.5, margin_vox=3.0)
    E, iK, H, W = R.live_camera("near", "30x44")
    out = fusion.raycast_volume(vol, _cuda(E), _cuda(iK), (H, W), near=R.NEAR, max_steps=R.max_steps_for(v))
    depth, flags = out["depth"][0, 0].cpu().numpy().astype(np.float64), out["flags"][0].cpu().numpy()
    assert inside.sum() > 0.3 * H * W
    assert ((flags & R.HIT) > 0)[inside].all()  # no hole
    rel = (np.abs(depth - want) / want)[inside].max()
    print(f"plane: {inside.sum()} interior pixels, max relative error {rel:.2e}")
    assert rel < 1e-4


def test_two_offset_planes_fuse_to_the_middle_while_the_warp_returns_the_nearer():
    from implicit_depth_amd import fusion, raster

    dims, v, origin = R.SCENES["room24x32"][:3]
    delta = 1.0 * v  # trunc = 4 voxels: delta = trunc / 4, and 1 + sqrt(3) + 1 < 4 keeps every corner both maps' linear band
    vol, d = _plane_setup([PLANE_D - delta, PLANE_D + delta], 4.0)
    want, inside = _plane_in_camera_b("near", "30x44", PLANE_D, margin_px=4.5, margin_vox=4.0)
    E, iK, H, W = R.live_camera("near", "30x44")
    out = fusion.raycast_volume(vol, _cuda(E), _cuda(iK), (H, W), near=R.NEAR, max_steps=R.max_steps_for(v))
    depth, flags = out["depth"][0, 0].cpu().numpy().astype(np.float64), out["flags"][0].cpu().numpy()
    assert inside.sum() > 0.3 * H * W and ((flags & R.HIT) > 0)[inside].all()
    rel = (np.abs(depth - want) / want)[inside].max()
    assert rel < 1e-4
    # the warp of the same two maps: the nearer sheet wins
    T = raster.relative_poses([R.LIVE_POSES["near"]], [PLANE_POSE, PLANE_POSE]).cuda()
    K_live = _cuda(R.LIVE_CAMERAS["30x44"][2])[None]
    invK_src = _cuda(np.stack([np.linalg.inv(PLANE_K)] * 2))
    warped = raster.warp_depth(_cuda(d), invK_src, T, K_live, H, W)["depth"][0, 0].cpu().numpy().astype(np.float64)
    nearer, _ = _plane_in_camera_b("near", "30x44", PLANE_D - delta, margin_px=4.5, margin_vox=4.0)
    assert (np.abs(warped - nearer) / nearer)[inside].max() < 1e-3
    assert ((want - warped) / want)[inside].min() > 0.5 * delta / PLANE_D
    print(f"fused {rel:.2e} from the plane at D; the warp sits {((want - warped)[inside]).mean():.4f} m in front of it (delta = {delta})")


def test_a_hole_in_one_map_is_filled_by_another():
    """Map 0 has a block of invalid taps; map 1, from another pose, saw that part of the room.  The fused ray cast from map 0's own camera
    hits there; the warp of map 0 alone is empty there."""
    from implicit_depth_amd import fusion, raster

    dims, v, origin, depth, K, E = R.scene_inputs("room24x32", 2)
    depth = np.stack([R._depth_map(24, 32, R.SCENES["room24x32"][4], seed=m, box=False, holes=False)[None] for m in range(2)])
    depth[0, 0, 9:15, 12:20] = np.nan
    vol = fusion.TSDFVolume(dims, v, origin)
    vol.integrate(_cuda(depth), _cuda(K), _cuda(E))
    Kc = R.SCENES["room24x32"][4]
    pose0 = R.KEY_POSES[0]
    out = fusion.raycast_volume(vol, _cuda(pose0), _cuda(np.linalg.inv(Kc)), (24, 32), near=R.NEAR, max_steps=R.max_steps_for(v))
    hit = ((out["flags"][0] & R.HIT) > 0).cpu().numpy()
    core = (slice(10, 14), slice(13, 19))  # the hole's interior in map 0's own pixels
    assert hit[core].all()
    fused = out["depth"][0, 0].cpu().numpy()[core]
    assert np.abs(fused - 1.75).max() < 0.2  # the room's surface
    T = raster.relative_poses([pose0], [pose0]).cuda()
    warped = raster.warp_depth(_cuda(depth[:1]), _cuda(np.linalg.inv(Kc))[None], T, _cuda(Kc)[None], 24, 32)["depth"][0, 0].cpu().numpy()
    assert (warped[core] == -1).all() and (warped > 0).mean() > 0.5


# ---- validation -----------------------------------------------------------------------------------------------------------------------
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4


def _good_args():
    """Argument structs that pass every check, on fake non-null pointers: nothing below reaches a launch."""
    from implicit_depth_amd import _lib

    def vol():
        x = _lib.TsdfVolume()
        x.values, x.block_flags, x.block_flag_bytes = 0x1000, 0x2000, 1 << 20
        x.voxel_size, x.trunc_voxels, x.Nz, x.Ny, x.Nx = 0.04, 3.0, 20, 28, 36
        return x

    i = _lib.TsdfIntegrateArgs()
    i.volume, i.depth_m1hw, i.K_m44, i.cam_T_world_m44, i.max_weight, i.M, i.h, i.w = vol(), 0x3000, 0x4000, 0x5000, 64.0, 2, 24, 32
    r = _lib.TsdfRaycastArgs()
    r.volume, r.world_T_cam_b44, r.invK_b44, r.depth_b1hw, r.flags_bhw = vol(), 0x3000, 0x4000, 0x5000, 0x6000
    r.near, r.step_voxels, r.empty_depth, r.max_steps, r.skip, r.B, r.H, r.W = 0.25, 1.0, -1.0, 100, 1, 1, 24, 32
    return vol, i, r


def test_error_codes():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert L.idh_sizeof_tsdf_volume() == C.sizeof(_lib.TsdfVolume) and L.idh_sizeof_tsdf_raycast_args() == C.sizeof(_lib.TsdfRaycastArgs)
    assert L.idh_sizeof_tsdf_integrate_args() == C.sizeof(_lib.TsdfIntegrateArgs)
    assert L.idh_tsdf_block_flag_bytes(20, 28, 36) == 3 * 4 * 5 and L.idh_tsdf_block_flag_bytes(9, 2, 10) == 1 * 1 * 2
    assert L.idh_tsdf_block_flag_bytes(1, 28, 36) == 0
    vol, _, _ = _good_args()
    calls = {
        "reset": lambda edit: L.idh_tsdf_reset_fwd(C.byref(edit_volume(vol(), edit)), None),
        "flags": lambda edit: L.idh_tsdf_flags_fwd(C.byref(edit_volume(vol(), edit)), None),
        "integrate": lambda edit: L.idh_tsdf_integrate_fwd(C.byref(edit_args(_good_args()[1], edit)), None),
        "raycast": lambda edit: L.idh_tsdf_raycast_fwd(C.byref(edit_args(_good_args()[2], edit)), None),
    }

    def edit_volume(v, edit):
        edit(v)
        return v

    def edit_args(a, edit):
        edit(a.volume)
        return a

    def setv(**kw):
        def f(v):
            for k, x in kw.items():
                setattr(v, k, x)
        return f

    def origin_nan(v):
        v.origin[1] = float("nan")

    volume_cases = [(setv(struct_size=8), EINVAL), (setv(Nz=1), EINVAL), (setv(Ny=0), EINVAL), (setv(Nx=-4), EINVAL),
                    (setv(voxel_size=0.0), EINVAL), (setv(voxel_size=float("inf")), EINVAL), (setv(trunc_voxels=float("nan")), EINVAL),
                    (setv(trunc_voxels=-1.0), EINVAL), (origin_nan, EINVAL), (setv(values=None), EINVAL),
                    (setv(Nz=2048, Ny=1024, Nx=1024, block_flag_bytes=1 << 40), EUNSUPPORTED), (setv(Nz=65536, Ny=2, Nx=2), EUNSUPPORTED),
                    (setv(Nz=2, Ny=262141, Nx=2), EUNSUPPORTED),
                    (setv(block_flags=None), EWORKSPACE), (setv(block_flag_bytes=59), EWORKSPACE), (setv(block_flag_bytes=-1), EWORKSPACE)]
    for name, call in calls.items():
        for edit, code in volume_cases:
            assert call(edit) == code, (name, code)
    assert L.idh_tsdf_reset_fwd(None, None) == EINVAL and L.idh_tsdf_flags_fwd(None, None) == EINVAL
    assert L.idh_tsdf_integrate_fwd(None, None) == EINVAL and L.idh_tsdf_raycast_fwd(None, None) == EINVAL

    def integrate(**kw):
        a = _good_args()[1]
        for k, x in kw.items():
            setattr(a, k, x)
        return L.idh_tsdf_integrate_fwd(C.byref(a), None)

    for kw in (dict(struct_size=16), dict(M=0), dict(h=0), dict(w=-1), dict(max_weight=0.5), dict(max_weight=float("inf")),
               dict(max_weight=float("nan")), dict(depth_m1hw=None), dict(K_m44=None), dict(cam_T_world_m44=None)):
        assert integrate(**kw) == EINVAL, kw
    assert integrate(M=17) == EUNSUPPORTED and integrate(M=16, h=1 << 14, w=1 << 13) == EUNSUPPORTED

    def raycast(**kw):
        a = _good_args()[2]
        for k, x in kw.items():
            setattr(a, k, x)
        return L.idh_tsdf_raycast_fwd(C.byref(a), None)

    for kw in (dict(struct_size=16), dict(B=0), dict(H=0), dict(W=-2), dict(max_steps=0), dict(step_voxels=0.0), dict(step_voxels=1.5),
               dict(step_voxels=float("nan")), dict(near=-0.1), dict(near=float("inf")), dict(empty_depth=float("nan")),
               dict(world_T_cam_b44=None), dict(invK_b44=None), dict(depth_b1hw=None), dict(flags_bhw=None)):
        assert raycast(**kw) == EINVAL, kw
    for kw in (dict(B=129), dict(B=128, H=4096, W=4096), dict(max_steps=65537)):
        assert raycast(**kw) == EUNSUPPORTED, kw


def test_python_layer_refuses_what_it_can_see():
    from implicit_depth_amd import fusion
    from implicit_depth_amd._lib import IdhError

    with pytest.raises(IdhError):
        fusion.TSDFVolume((1, 8, 8), 0.04, (0, 0, 0))
    with pytest.raises(IdhError):
        fusion.TSDFVolume((8, 8, 8), -0.04, (0, 0, 0))
    vol = fusion.TSDFVolume((8, 9, 10), 0.04, (0, 0, 0))
    with pytest.raises(IdhError):
        vol.integrate(torch.ones(1, 4, 5).cuda(), torch.eye(4), torch.eye(4))
    with pytest.raises(IdhError):
        vol.integrate(torch.ones(2, 1, 4, 5).cuda(), torch.eye(4), torch.eye(4))
    with pytest.raises(IdhError):
        vol.integrate(torch.ones(17, 1, 4, 5).cuda(), torch.eye(4).repeat(17, 1, 1), torch.eye(4).repeat(17, 1, 1))
    with pytest.raises(IdhError):
        vol.raycast(torch.eye(4), torch.eye(4), (4, 5), step_voxels=2.0)
    with pytest.raises(IdhError):
        fusion.TSDFVolume.from_values(torch.ones(8, 9, 10).cuda(), 0.04, (0, 0, 0))
