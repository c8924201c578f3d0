"""The fusion of a StreamingSession (start_fusion / fused_depth_for_view / composite_asset(depth_source="fused")) against the public
calls chained by hand, bit for bit: ``fusion.TSDFVolume`` integrating the same maps and ray-casting the same camera, and
``compositing.composite_depth`` on its result.  What the kernels return is held to fp64 in test_tsdf_gpu.py.  Sessions are built as
tests/test_warp_session_gpu.py builds its own."""
import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import warp_ref as WR
from test_render_gpu import _asset_mesh
from test_streaming_gpu import BUFFER, IMG_H, IMG_W, _frame, _model
from test_warp_session_gpu import LIVE, _depth_model

pytestmark = pytest.mark.gpu
FUSION = dict(voxel_size=0.1, dims=(61, 52, 67), trunc_voxels=3.0, max_weight=64.0)  # 6.1 x 5.2 x 6.7 m around the first camera
VIEW = dict(near=0.3, far=4.0)


def _by_hand(maps, origin, **kw):
    """A volume integrating (depth, world_T_cam, invK) triples, oldest first, one call per map as the session does."""
    from implicit_depth_amd import fusion

    vol = fusion.TSDFVolume(FUSION["dims"], FUSION["voxel_size"], origin, FUSION["trunc_voxels"], FUSION["max_weight"])
    for d, pose, invK in maps:
        vol.integrate(d, torch.linalg.inv(invK.reshape(1, 4, 4)), torch.from_numpy(np.linalg.inv(np.asarray(pose, np.float64)).astype(np.float32))[None])
    return vol


def _centred(pose):
    nz, ny, nx = FUSION["dims"]
    return tuple(np.asarray(pose, np.float64)[:3, 3] - FUSION["voxel_size"] * 0.5 * (np.array([nx, ny, nz], np.float64) - 1.0))


def _view_by_hand(vol, pose, invK, size, **kw):
    T = torch.from_numpy(np.asarray(pose, np.float64).astype(np.float32))[None]
    return vol.raycast(T, invK.reshape(1, 4, 4), size, **kw)


def _same_view(got, want, normals):
    assert set(got) == {"view_fused_depth", "view_fused_valid", "view_fused_flags"} | ({"view_fused_normals"} if normals else set())
    assert torch.equal(got["view_fused_depth"], want["depth"]) and torch.equal(got["view_fused_flags"], want["flags"])
    assert got["view_fused_valid"].dtype == torch.bool and torch.equal(got["view_fused_valid"], ((want["flags"] & 1) != 0)[:, None])
    if normals:
        assert torch.equal(got["view_fused_normals"], want["normals"])


def test_depth_model_session_fuses_its_predictions_beyond_the_ring():
    from implicit_depth_amd import AssetRenderer, compositing, raster
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    session = StreamingSession(_depth_model("dot", 2), num_source_views=2, buffer_size=BUFFER, query_keyframes=1)
    verts, faces, colors = _asset_mesh(seed=1)
    asset = AssetRenderer(verts, faces, colors, world_T_asset=np.eye(4), ambient=0.3)
    K_img = syn.intrinsics(IMG_W, IMG_H).float().cuda()
    invK_live = torch.linalg.inv(syn.intrinsics(LIVE[1], LIVE[0]).float().cuda())
    image = torch.randint(0, 256, (1, IMG_H, IMG_W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    with pytest.raises(IdhError, match="start_fusion"):
        session.fused_depth_for_view(poses[0], invK_live, LIVE)
    with pytest.raises(IdhError, match="start_fusion"):
        session.composite_asset(image, asset, poses[0], K_img, depth_source="fused")
    with pytest.raises(IdhError, match="depth_source"):
        session.composite_asset(image, asset, poses[0], K_img, depth_source="lidar")
    session.start_fusion(**FUSION)
    with pytest.raises(IdhError, match="no prediction"):
        session.fused_depth_for_view(poses[0], invK_live, LIVE)
    maps, checked = [], 0
    for t in range(9):
        frame = _frame(t, poses)
        out, code = session.step(frame, world_T_cam=poses[t], dist_to_last_valid=dists[t])
        if out is not None:
            maps.append((out["depth_pred_s0_b1hw"].clone(), poses[t], frame["invK_s0_b44"]))
            continue
        if len(maps) < 2:
            continue
        checked += 1
        # the ring holds one map (query_keyframes = 1); the volume holds them all
        assert len(session._depth_ring) == 1
        vol = _by_hand(maps, _centred(maps[0][1]))
        assert torch.equal(session.fusion_volume.values, vol.values) and torch.equal(session.fusion_volume.block_flags, vol.block_flags)
        newest_only = _by_hand(maps[-1:], _centred(maps[0][1]))
        assert not torch.equal(newest_only.values, vol.values)
        assert float(vol.values[..., 1].max()) >= 2.0  # voxels two predictions saw: the first has left the ring, not the volume
        for kw in (dict(), dict(return_normals=True), dict(step_voxels=0.5, empty_depth=7.0, return_normals=True)):
            got = session.fused_depth_for_view(poses[t], invK_live, LIVE, **VIEW, **kw)
            _same_view(got, _view_by_hand(vol, poses[t], invK_live, LIVE, **VIEW, **kw), kw.get("return_normals", False))
        cover = got["view_fused_valid"].float().mean().item()
        print(f"frame {t}: {len(maps)} fused predictions, hits in {cover:.3f} of the live view")
        assert (got["view_fused_depth"][~got["view_fused_valid"]] == 7.0).all()
        # the whole frame through the fused depth
        cam_T_mesh = torch.from_numpy(np.linalg.inv(poses[t]).astype(np.float32))[None].cuda()
        full = raster.render_shaded(asset.verts, asset.faces, cam_T_mesh, K_img[None], IMG_H, IMG_W, colors=asset.colors, ambient=0.3)
        for size in (None, (45, 60)):
            kw = {} if size is None else {"query_size": size}
            h, w = compositing.MODEL_SIZE if size is None else size
            Kq = K_img[None].clone()
            Kq[:, 0] *= w / IMG_W
            Kq[:, 1] *= h / IMG_H
            fused = _view_by_hand(vol, poses[t], torch.linalg.inv(Kq), (h, w), empty_depth=session.WARP_FAR)["depth"]
            by_hand = compositing.composite_depth(image, fused, virtual_depth=full["depth"][:, 0], virtual_rgba=full["rgba"])
            parts = session.composite_asset(image, asset, poses[t], K_img, return_parts=True, depth_source="fused", **kw)
            assert torch.equal(parts["frame"], by_hand) and torch.equal(parts["view_fused_depth"], fused)
            assert torch.equal(parts["asset_depth"], full["depth"]) and torch.equal(parts["asset_rgba"], full["rgba"])
            assert torch.equal(session.composite_asset(image, asset, poses[t], K_img, depth_source="fused", fade=[0.5], bgr=True, **kw),
                               compositing.composite_depth(image, fused, virtual_depth=full["depth"][:, 0], virtual_rgba=full["rgba"], fade=[0.5], bgr=True))
    assert checked >= 1, "the sequence has no frame between keyframes after two predictions"
    storage = session.fusion_volume.values.data_ptr()
    session.reset()
    v = session.fusion_volume
    assert v.values.data_ptr() == storage and (v.values[..., 0] == 1).all() and (v.values[..., 1] == 0).all() and not v.block_flags.any()
    with pytest.raises(IdhError, match="no prediction"):
        session.fused_depth_for_view(poses[0], invK_live, LIVE)
    with pytest.raises(IdhError, match="no prediction"):
        session.composite_asset(image, asset, poses[0], K_img, depth_source="fused")


def test_bd_model_session_with_fusion_answers_as_before_and_fuses_supplied_maps():
    """Three sessions on models with the same weights see the same frames: a plain one, one with a depth ring alone, one with the ring
    and fusion.  Every existing method returns the same bits in all of them; the fused view is the hand-made one."""
    from implicit_depth_amd import AssetRenderer, compositing
    from implicit_depth_amd.streaming import StreamingSession

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    plain, ringed, fusing = (StreamingSession(_model("mlp", 3), buffer_size=BUFFER, query_keyframes=2) for _ in range(3))
    origin = tuple(float(x) for x in poses[0][:3, 3] - np.array([3.37, 2.58, 2.96]))  # an explicit origin, not the centring default
    fusing.start_fusion(origin=origin, **FUSION)
    verts, faces, colors = _asset_mesh(seed=1)
    asset = AssetRenderer(verts, faces, colors, world_T_asset=np.eye(4), ambient=0.3)
    K_img = syn.intrinsics(IMG_W, IMG_H).float().cuda()
    K_live = syn.intrinsics(LIVE[1], LIVE[0]).float().cuda()
    invK_live = torch.linalg.inv(K_live)
    invK_src = torch.from_numpy(np.linalg.inv(WR.source_K()).astype(np.float32)).cuda()
    image = torch.randint(0, 256, (1, IMG_H, IMG_W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    maps, done = [], False
    for t in range(9):
        outs = [s.step(_frame(t, poses), world_T_cam=poses[t], dist_to_last_valid=dists[t]) for s in (plain, ringed, fusing)]
        assert outs[0][1] == outs[1][1] == outs[2][1]
        if outs[0][0] is not None:
            for k, v in outs[0][0].items():
                for o in outs[1:]:
                    assert (v is None and o[0][k] is None) or torch.equal(v, o[0][k]), (t, k)
            lidar = torch.from_numpy(WR.source_depth(seed=t, box=t % 2 == 0) + np.float32(0.4))[None, None].cuda()
            for s in (ringed, fusing):
                s.remember_depth(lidar, poses[t], invK_src)
            maps.append((lidar.clone(), poses[t], invK_src[None]))
            continue
        if len(maps) < 3:
            continue
        vol = _by_hand(maps, origin)
        got = fusing.fused_depth_for_view(poses[t], invK_live, LIVE, return_normals=True, **VIEW)
        _same_view(got, _view_by_hand(vol, poses[t], invK_live, LIVE, return_normals=True, **VIEW), True)
        cover = got["view_fused_valid"].float().mean().item()
        print(f"frame {t}: {len(maps)} supplied maps fused (the ring holds 2), hits in {cover:.3f} of the live view")
        assert len(fusing._depth_ring) == 2 and cover > 0.2
        depth = asset.render(poses[t], K_live, LIVE)["depth"]
        for name, call in (("occlusion_for_view", lambda s: s.occlusion_for_view(depth, poses[t], invK_live, fill=-20.0)),
                           ("depth_for_view", lambda s: s.depth_for_view(poses[t], invK_live, LIVE)),
                           ("first_hit_for_view", lambda s: s.first_hit_for_view(poses[t], invK_live, LIVE)),
                           ("composite_asset", lambda s: s.composite_asset(image, asset, poses[t], K_img, return_parts=True)),
                           ("warped_depth_for_view", lambda s: s.warped_depth_for_view(poses[t], K_live, LIVE, return_source=True))):
            res = [call(s) for s in ((plain, ringed, fusing) if name != "warped_depth_for_view" else (ringed, fusing))]
            for other in res[1:]:
                assert set(res[0]) == set(other) and "view_fused_depth" not in other
                for k in res[0]:
                    assert (res[0][k] is None and other[k] is None) or torch.equal(res[0][k], other[k]), (name, k)
        # the compositor against the fused surface, in a session that has an occlusion MLP
        Kq = K_img[None].clone()
        h, w = compositing.MODEL_SIZE
        Kq[:, 0] *= w / IMG_W
        Kq[:, 1] *= h / IMG_H
        full = asset.render(poses[t], K_img, (IMG_H, IMG_W))
        fused = _view_by_hand(vol, poses[t], torch.linalg.inv(Kq), (h, w), empty_depth=fusing.WARP_FAR)["depth"]
        assert torch.equal(fusing.composite_asset(image, asset, poses[t], K_img, depth_source="fused"),
                           compositing.composite_depth(image, fused, virtual_depth=full["depth"][:, 0], virtual_rgba=full["rgba"]))
        done = True
        break
    assert done
