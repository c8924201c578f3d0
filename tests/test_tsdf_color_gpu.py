"""TSDF colour on the GPU (include/idh_fusion.h, csrc/tsdf.hip, csrc/tsdf_mesh.hip, implicit_depth_amd.fusion) against
the fp64 reference of tests/tsdf_color_ref.py outside what it calls ambiguous (test_tsdf_color_cpu.py holds it under 1 %), the
bit-level promises of the header - the geometry keeps the bits of the calls without colour - and closed forms."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref as MR
import tsdf_color_ref as CR
import tsdf_ref as R

pytestmark = pytest.mark.gpu
CONST = (200, 100, 50)


def _cuda(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _volume(scene, **kw):
    from implicit_depth_amd import fusion

    dims, v, origin = R.SCENES[scene][:3]
    return fusion.TSDFVolume(dims, v, origin, color=True, **kw)


def _const_frames(scene, cam, M, rgb=CONST):
    frames, Kc = CR.scene_frames(scene, cam, M)
    out = np.empty_like(frames)
    out[...] = np.asarray(rgb, np.uint8)
    return out, Kc


def _integrate(scene, cam, M=None, max_weight=64.0, calls=1, frames=None):
    """The scene's maps and frames (the reference's, or ``frames``) into a fresh coloured volume, in one call or one call per map."""
    dims, v, origin, depth, K, E = R.scene_inputs(scene, M)
    f, Kc = CR.scene_frames(scene, cam, M)
    if frames is not None:
        f = frames
    vol = _volume(scene, max_weight=max_weight)
    d, K, E, f, Kc = _cuda(depth), _cuda(K), _cuda(E), _cuda(f, torch.uint8), _cuda(Kc)
    if calls == 1:
        vol.integrate(d, K, E, f, None if cam == "same" else Kc)  # the map's own size and K: color_K=None means K
    else:
        for m in range(d.shape[0]):
            vol.integrate(d[m:m + 1], K[m:m + 1], E[m:m + 1], f[m:m + 1], Kc[m:m + 1])
    return vol


def _plain(scene, M=None, max_weight=64.0):
    from implicit_depth_amd import fusion

    dims, v, origin, depth, K, E = R.scene_inputs(scene, M)
    vol = fusion.TSDFVolume(dims, v, origin, max_weight=max_weight)
    vol.integrate(_cuda(depth), _cuda(K), _cuda(E))
    return vol


@functools.lru_cache(maxsize=None)
def _fused(scene, cam, const=False):
    """The GPU's fused (values, colors) of a scene on the host: what both the kernels and the references ray-cast and mesh."""
    vol = _integrate(scene, cam, frames=_const_frames(scene, cam, None)[0] if const else None)
    return vol.values.cpu().numpy(), vol.colors.cpu().numpy()


def _adopt(scene, values, colors):
    from implicit_depth_amd import fusion

    dims, v, origin = R.SCENES[scene][:3]
    return fusion.TSDFVolume.from_values(_cuda(values), v, origin, colors=_cuda(colors))


# ---- integrate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", sorted(R.SCENES))
@pytest.mark.parametrize("cam", CR.COLOR_CAMERAS)
@pytest.mark.parametrize("M", [1, None])
@pytest.mark.parametrize("max_weight", [64.0, 2.0])
def test_integrate_matches_fp64(scene, cam, M, max_weight):
    ref = CR.scene_integrated(scene, cam, M, max_weight)
    vol = _integrate(scene, cam, M, max_weight)
    got = vol.colors.cpu().numpy()
    ok = ~ref["ambiguous"]
    assert (ref["touched"] & ~ok).sum() <= CR.CAP * ref["touched"].sum()
    assert (got[..., 3][ok] == ref["Wc"][ok]).all()
    nothing = ok & ~ref["coloured"]
    assert (got[nothing] == 0).all() and nothing.sum() > 100
    err = np.abs(got[..., :3] - ref["C"])[ok].max()
    print(f"{scene} {cam} M={M} max_weight={max_weight}: max |C - C_ref| = {err:.2e} over {ok.sum()} voxels, {int(ref['coloured'].sum())} coloured, "
          f"Wc max {got[..., 3].max()}")
    assert err < 1e-3
    assert got[..., 3].max() == (1 if M == 1 else min(R.SCENES[scene][5], max_weight))
    plain = _plain(scene, M, max_weight)
    assert torch.equal(vol.values, plain.values) and torch.equal(vol.block_flags, plain.block_flags)
    assert (vol.colors[..., 3] <= vol.values[..., 1]).all()


@pytest.mark.parametrize("scene", sorted(R.SCENES))
def test_integrate_bits(scene):
    one, again, per_map = _integrate(scene, "odd"), _integrate(scene, "odd"), _integrate(scene, "odd", calls=3)
    assert torch.equal(one.colors, again.colors) and torch.equal(one.values, again.values) and torch.equal(one.block_flags, again.block_flags)
    assert torch.equal(one.colors, per_map.colors) and torch.equal(one.values, per_map.values) and torch.equal(one.block_flags, per_map.block_flags)
    assert (one.colors[..., 3] > 0).any()
    # depth-only maps on a coloured volume: the geometry moves, the colours do not
    dims, v, origin, depth, K, E = R.scene_inputs(scene)
    colors, values = one.colors.clone(), one.values.clone()
    one.integrate(_cuda(depth), _cuda(K), _cuda(E))
    assert torch.equal(one.colors, colors) and not torch.equal(one.values, values)
    assert (one.colors[..., 3] <= one.values[..., 1]).all()
    # a map of invalid taps with a valid frame changes nothing
    bad = np.full_like(depth[:1], np.nan)
    bad[0, 0, ::2] = 0.0
    bad[0, 0, 1::3] = -2.0
    bad[0, 0, 2, 3] = np.inf
    frames, Kc = CR.scene_frames(scene, "odd", 1)
    values, flags = one.values.clone(), one.block_flags.clone()
    one.integrate(_cuda(bad), _cuda(K[:1]), _cuda(E[:1]), _cuda(frames, torch.uint8), _cuda(Kc))
    assert torch.equal(one.colors, colors) and torch.equal(one.values, values) and torch.equal(one.block_flags, flags)
    empty = _volume(scene)
    empty.integrate(_cuda(bad), _cuda(K[:1]), _cuda(E[:1]), _cuda(frames, torch.uint8), _cuda(Kc))
    assert not empty.colors.any() and not empty.block_flags.any()
    one.reset()
    assert not one.colors.any() and (one.values[..., 0] == 1).all() and (one.values[..., 1] == 0).all()


def test_constant_frames_give_the_constant_colour():
    scene = "room24x32"
    vol = _integrate(scene, "double", frames=_const_frames(scene, "double", None)[0])
    c = vol.colors.cpu().numpy()
    has = c[..., 3] > 0
    assert has.sum() > 1000 and (c[..., 3] == 3).any()
    assert (c[has][:, :3] == np.asarray(CONST, np.float32)).all() and (c[~has] == 0).all()


def test_two_maps_from_one_pose_average():
    from implicit_depth_amd import fusion

    dims, v, origin, depth, K, E = R.scene_inputs("room24x32", 1)
    frames = np.stack([np.full((24, 32, 3), 100, np.uint8), np.full((24, 32, 3), 200, np.uint8)])
    vol = fusion.TSDFVolume(dims, v, origin, color=True)
    vol.integrate(_cuda(np.concatenate([depth, depth])), _cuda(np.concatenate([K, K])), _cuda(np.concatenate([E, E])), _cuda(frames, torch.uint8))
    c = vol.colors.cpu().numpy()
    two = c[..., 3] == 2
    assert two.sum() > 1000 and (c[two][:, :3] == 150).all() and set(np.unique(c[..., 3])) == {0.0, 2.0}


def test_a_hole_in_one_map_carries_the_other_maps_colour_alone():
    """Map 0 has a block of invalid taps and map 1, from another pose, saw that part of the room: the voxels that project into the hole
    of map 0 hold map 1's colour; elsewhere voxels both maps coloured hold the mean."""
    from implicit_depth_amd import fusion

    dims, v, origin, depth, K, E = R.scene_inputs("room24x32", 2)
    Km = R.SCENES["room24x32"][4]
    depth = np.stack([R._depth_map(24, 32, Km, seed=m, box=False, holes=False)[None] for m in range(2)])
    depth[0, 0, 9:15, 12:20] = np.nan
    frames = np.stack([np.full((24, 32, 3), (10, 20, 30), np.uint8), np.full((24, 32, 3), CONST, np.uint8)])
    vol = fusion.TSDFVolume(dims, v, origin, color=True)
    vol.integrate(_cuda(depth), _cuda(K), _cuda(E), _cuda(frames, torch.uint8))
    c = vol.colors.cpu().numpy()
    # fp64: the voxels whose projection into map 0 lies well inside the hole
    zz, yy, xx = np.meshgrid(*(np.arange(d) for d in dims), indexing="ij")
    p = np.stack([origin[0] + np.float64(np.float32(v)) * xx, origin[1] + np.float64(np.float32(v)) * yy, origin[2] + np.float64(np.float32(v)) * zz], -1)
    cam = p @ E[0, :3, :3].astype(np.float64).T + E[0, :3, 3].astype(np.float64)
    px, py = Km[0, 0] * cam[..., 0] / cam[..., 2] + Km[0, 2], Km[1, 1] * cam[..., 1] / cam[..., 2] + Km[1, 2]
    in_hole = (cam[..., 2] > 0) & (px > 12.1) & (px < 19.9) & (py > 9.1) & (py < 14.9)
    there = in_hole & (c[..., 3] > 0)
    assert there.sum() > 30 and (c[there][:, 3] == 1).all() and (c[there][:, :3] == np.asarray(CONST, np.float32)).all()
    both = c[..., 3] == 2
    assert both.sum() > 1000 and (c[both][:, :3] == np.asarray([105, 60, 40], np.float32)).all()


# ---- ray cast -------------------------------------------------------------------------------------------------------------------------
def _raycast(vol, scene, pose, cam, **kw):
    from implicit_depth_amd import fusion

    v = R.SCENES[scene][1]
    E, iK, H, W = R.live_camera(pose, cam)
    kw.setdefault("near", R.NEAR)
    kw.setdefault("max_steps", R.max_steps_for(v))
    return fusion.raycast_volume(vol, _cuda(E), _cuda(iK), (H, W), **kw)


@pytest.mark.parametrize("scene,pose,cam", R.RAYCAST_CASES)
@pytest.mark.parametrize("color_cam", ["same", "odd"])
def test_raycast_keeps_the_geometry_and_matches_fp64(scene, pose, cam, color_cam):
    values, colors = _fused(scene, color_cam)
    vol = _adopt(scene, values, colors)
    out = None
    for skip in (True, False):
        for normals in (True, False):
            col = _raycast(vol, scene, pose, cam, skip=skip, return_normals=normals, return_color=True)
            plain = _raycast(vol, scene, pose, cam, skip=skip, return_normals=normals)
            assert set(col) == set(plain) | {"rgba"} and col["rgba"].dtype == torch.uint8
            for k in plain:
                assert torch.equal(col[k], plain[k]), (skip, normals, k)
            if out is not None:
                assert torch.equal(col["rgba"], out["rgba"]), (skip, normals)
            out = col
    dims, v, origin = R.SCENES[scene][:3]
    E, iK, H, W = R.live_camera(pose, cam)
    hit = ((out["flags"][0] & R.HIT) > 0).cpu().numpy()
    ref = CR.raycast_colors(colors, out["depth"][0, 0].cpu().numpy(), hit, origin, v, E, iK)
    got = out["rgba"][0].cpu().numpy().astype(np.int64)
    ok = ~ref["ambiguous"]
    assert (~ok).sum() <= CR.CAP * H * W
    assert (got[~hit] == 0).all()
    assert ((got[..., 3] == 255) == ref["alpha"])[ok].all() and np.isin(got[..., 3], (0, 255)).all()
    assert (got[ok & ~ref["alpha"]] == 0).all()
    diff = np.abs(got - ref["rgba"])[ok]
    certain = ok[..., None] & (CR.boundary_distance(ref["value"]) > ref["bound"][..., None]) & ref["alpha"][..., None]
    wrong = (got[..., :3] != ref["rgba"][..., :3]) & certain
    print(f"{scene} {pose} {cam} colours {color_cam}: {int(ref['alpha'].sum())} of {H * W} pixels with alpha, {int((~ok).sum())} ambiguous, max |rgba - ref| = "
          f"{diff.max()}, {int(certain.sum())} of {3 * int(ref['alpha'].sum())} channels certain, bound max {ref['bound'][ref['alpha']].max():.2e}")
    assert diff.max() <= 1
    assert not wrong.any() and certain.sum() > 0.9 * 3 * ref["alpha"].sum()
    assert (hit & ref["alpha"]).sum() > 0.2 * H * W


def test_two_cameras_equal_two_calls_with_colour():
    from implicit_depth_amd import fusion

    scene = "room24x32"
    vol = _adopt(scene, *_fused(scene, "odd"))
    v = R.SCENES[scene][1]
    cams = [R.live_camera(p, "24x32") for p in ("near", "side")]
    E, iK = _cuda(np.stack([c[0] for c in cams])), _cuda(np.stack([c[1] for c in cams]))
    kw = dict(near=R.NEAR, max_steps=R.max_steps_for(v), return_normals=True, return_color=True)
    both = fusion.raycast_volume(vol, E, iK, (24, 32), **kw)
    assert tuple(both["rgba"].shape) == (2, 24, 32, 4)
    for b in range(2):
        one = fusion.raycast_volume(vol, E[b], iK[b], (24, 32), **kw)
        for k in one:
            assert torch.equal(one[k][0], both[k][b]), (b, k)
    a = vol.raycast(E, iK, (24, 32), near=R.NEAR, far=R.FAR, return_normals=True, return_color=True)
    for k in both:
        assert torch.equal(a[k], both[k]), k


@pytest.mark.parametrize("scene,pose,cam", R.RAYCAST_CASES[:2])
def test_raycast_of_the_constant_volume_is_the_constant(scene, pose, cam):
    vol = _adopt(scene, *_fused(scene, "same", True))
    out = _raycast(vol, scene, pose, cam, return_color=True)
    rgba = out["rgba"][0].cpu().numpy()
    has = rgba[..., 3] > 0
    assert has.sum() > 0.2 * has.size and (rgba[has] == np.asarray(CONST + (255,), np.uint8)).all() and (rgba[~has] == 0).all()


# ---- mesh -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", sorted(R.SCENES))
@pytest.mark.parametrize("color_cam", ["same", "odd"])
def test_mesh_colours_match_the_reference_and_keep_the_mesh(scene, color_cam):
    from implicit_depth_amd import fusion

    values, colors = _fused(scene, color_cam)
    dims, v, origin = R.SCENES[scene][:3]
    vol = _adopt(scene, values, colors)
    col, plain = fusion.extract_mesh(vol, return_weights=True, return_colors=True), fusion.extract_mesh(vol, return_weights=True)
    assert set(col) == set(plain) | {"colors"}
    for k in plain:
        assert torch.equal(col[k], plain[k]), k
    m = MR.extract(values, origin, v)
    V = len(m["owner"])
    assert tuple(col["colors"].shape) == (V, 4) and col["colors"].dtype == torch.uint8 and V > 500
    ref = CR.mesh_colors(values, colors, m["owner"], m["axis"])
    got = col["colors"].cpu().numpy().astype(np.int64)
    assert np.abs(got - ref["rgba"]).max() <= 1
    certain = (CR.boundary_distance(ref["value"]) > 1e-3) & ref["alpha"][:, None]
    # (the mean of two integer taps is often exactly k + 0.5: those channels are not "certain", which is why the share is not near 1)
    assert (got[:, :3] == ref["rgba"][:, :3])[certain].all() and certain.sum() > 0.8 * 3 * ref["alpha"].sum()
    assert ((got[:, 3] == 255) == ref["alpha"]).all() and (got[~ref["alpha"]] == 0).all()
    print(f"{scene} {color_cam}: {V} vertices, {int(ref['alpha'].sum())} with a colour, {int((~ref['alpha']).sum())} without")
    again = vol.extract_mesh(return_colors=True)
    assert torch.equal(again["colors"], col["colors"]) and set(again) == {"verts", "faces", "colors"}
    # a capacity smaller than V writes nothing past it
    workspace, totals = fusion.mesh_count(vol)
    assert totals.tolist()[0] == V
    cap = V // 2 + 1
    out = torch.full((V, 4), 77, dtype=torch.uint8, device="cuda")
    fusion.mesh_colors(vol, workspace, out, vert_capacity=cap)
    assert torch.equal(out[:cap], col["colors"][:cap]) and (out[cap:] == 77).all()


def test_empty_mesh_has_no_colours():
    from implicit_depth_amd import fusion
    from implicit_depth_amd._lib import IdhError

    vol = fusion.TSDFVolume((8, 9, 10), 0.04, (0, 0, 0), color=True)
    out = vol.extract_mesh(return_colors=True)
    assert tuple(out["colors"].shape) == (0, 4) and out["colors"].dtype == torch.uint8 and tuple(out["verts"].shape) == (0, 3)
    bare = fusion.TSDFVolume((8, 9, 10), 0.04, (0, 0, 0))
    assert bare.colors is None
    with pytest.raises(IdhError):
        bare.extract_mesh(return_colors=True)
    with pytest.raises(IdhError):
        bare.raycast(torch.eye(4), torch.eye(4), (4, 5), return_color=True)
    with pytest.raises(IdhError):
        bare.integrate(torch.ones(1, 1, 4, 5).cuda(), torch.eye(4), torch.eye(4), torch.zeros(1, 4, 5, 3, dtype=torch.uint8).cuda())
    with pytest.raises(IdhError):  # a frame of another size needs its intrinsics
        vol.integrate(torch.ones(1, 1, 4, 5).cuda(), torch.eye(4), torch.eye(4), torch.zeros(1, 8, 10, 3, dtype=torch.uint8).cuda())
    with pytest.raises(IdhError):
        vol.integrate(torch.ones(1, 1, 4, 5).cuda(), torch.eye(4), torch.eye(4), torch.zeros(1, 4, 5, 3).cuda())


def test_constant_mesh_through_ply_and_the_shaded_renderer(tmp_path):
    from implicit_depth_amd import raster

    scene = "room24x32"
    vol = _adopt(scene, *_fused(scene, "same", True))
    mesh = vol.extract_mesh(return_colors=True)
    colors = mesh["colors"].cpu().numpy()
    assert len(colors) > 500 and (colors == np.asarray(CONST + (255,), np.uint8)).all()
    path = str(tmp_path / "fused.ply")
    raster.save_ply(path, mesh["verts"], mesh["faces"], colors=mesh["colors"])
    verts, faces, back = raster.load_ply(path, return_colors=True)
    assert np.array_equal(np.asarray(back), colors) and np.array_equal(np.asarray(verts), mesh["verts"].cpu().numpy())
    assert np.array_equal(np.asarray(faces), mesh["faces"].cpu().numpy())
    (h, w), K = R.SCENES[scene][3], R.SCENES[scene][4]
    out = raster.render_shaded(mesh["verts"], mesh["faces"], _cuda(np.linalg.inv(R.KEY_POSES[0]))[None], _cuda(K)[None], h, w, colors=mesh["colors"], ambient=1.0)
    rgba, covered = out["rgba"][0].cpu().numpy().astype(np.int64), (out["depth"][0, 0] > 0).cpu().numpy()
    assert covered.sum() > 0.2 * h * w
    assert np.abs(rgba[covered] - np.asarray(CONST + (255,))).max() <= 1 and (rgba[~covered] == 0).all()
