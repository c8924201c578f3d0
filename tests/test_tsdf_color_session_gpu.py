"""The colour of a StreamingSession's fusion (start_fusion(color=True), remember_depth / step with a frame, fused_depth_for_view and
fused_mesh with colours) against the public ``fusion`` calls chained by hand, bit for bit.  What the kernels return is held to fp64 in
test_tsdf_color_gpu.py.  Sessions are built as tests/test_tsdf_session_gpu.py builds its own."""
import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import warp_ref as WR
from test_streaming_gpu import BUFFER, IMG_H, IMG_W, _frame
from test_tsdf_session_gpu import FUSION, VIEW, _centred
from test_warp_session_gpu import LIVE, _depth_model

pytestmark = pytest.mark.gpu
FRAME = (60, 84)  # the supplied maps' camera frames: not a multiple of the 24 x 32 maps


def _cam_T_world(pose):
    return torch.from_numpy(np.linalg.inv(np.asarray(pose, np.float64)).astype(np.float32))[None]


def _by_hand(maps, origin, color=True):
    """A volume integrating (depth, world_T_cam, invK, frame, frame_K) tuples, oldest first, one call per map as the session does."""
    from implicit_depth_amd import fusion

    vol = fusion.TSDFVolume(FUSION["dims"], FUSION["voxel_size"], origin, FUSION["trunc_voxels"], FUSION["max_weight"], color=color)
    for d, pose, invK, frame, frame_K in maps:
        vol.integrate(d, torch.linalg.inv(invK.reshape(1, 4, 4)), _cam_T_world(pose), frame, None if frame is None else frame_K.reshape(1, 4, 4))
    return vol


def _frames(n, size, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (1, size[0], size[1], 3), dtype=torch.uint8, generator=g).cuda() for _ in range(n)]


def test_supplied_maps_with_frames_equal_the_calls_by_hand():
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    poses, _ = syn.keyframe_trajectory("stream12", seed=0)
    given, scaled, plain, coloured_unused = (StreamingSession(_depth_model("dot", 2), num_source_views=2, buffer_size=BUFFER, query_keyframes=1) for _ in range(4))
    origin = tuple(float(x) for x in poses[0][:3, 3] - np.array([3.37, 2.58, 2.96]))
    given.start_fusion(origin=origin, color=True, **FUSION)
    scaled.start_fusion(origin=origin, color=True, **FUSION)
    plain.start_fusion(origin=origin, **FUSION)
    coloured_unused.start_fusion(origin=origin, color=True, **FUSION)
    K_src = torch.from_numpy(WR.source_K().astype(np.float32)).cuda()
    invK_src = torch.from_numpy(np.linalg.inv(WR.source_K()).astype(np.float32)).cuda()
    K_scaled = torch.linalg.inv(invK_src[None])  # the rule of frame_K=None: the inverse of invK, rows 0 and 1 scaled
    K_scaled[:, 0] *= FRAME[1] / WR.SRC_W
    K_scaled[:, 1] *= FRAME[0] / WR.SRC_H
    K_own = K_src.clone()  # an unrelated colour camera
    K_own[0, 0], K_own[1, 1], K_own[0, 2], K_own[1, 2] = 70.0, 73.0, 40.5, 31.0
    frames = _frames(4, FRAME)
    with pytest.raises(IdhError, match="color=True"):
        plain.remember_depth(torch.ones(1, 1, 24, 32).cuda(), poses[0], invK_src, frame_u8=frames[0])
    assert not plain._depth_ring and plain.fusion_volume is None  # refused before anything was remembered
    maps_given, maps_scaled, maps_plain = [], [], []
    for t in range(4):
        lidar = torch.from_numpy(WR.source_depth(seed=t, box=t % 2 == 0) + np.float32(0.4))[None, None].cuda()
        given.remember_depth(lidar, poses[t], invK_src, frame_u8=frames[t], frame_K=K_own)
        scaled.remember_depth(lidar, poses[t], invK_src, frame_u8=frames[t])
        plain.remember_depth(lidar, poses[t], invK_src)
        coloured_unused.remember_depth(lidar, poses[t], invK_src)
        maps_given.append((lidar, poses[t], invK_src, frames[t], K_own))
        maps_scaled.append((lidar, poses[t], invK_src, frames[t], K_scaled))
        maps_plain.append((lidar, poses[t], invK_src, None, None))
    for session, maps in ((given, maps_given), (scaled, maps_scaled)):
        vol, sv = _by_hand(maps, origin), session.fusion_volume
        assert torch.equal(sv.values, vol.values) and torch.equal(sv.block_flags, vol.block_flags) and torch.equal(sv.colors, vol.colors)
        assert float(sv.colors[..., 3].max()) >= 2.0
        T = torch.from_numpy(np.asarray(poses[4], np.float64).astype(np.float32))[None]
        for kw in (dict(), dict(return_normals=True, step_voxels=0.5, empty_depth=7.0)):
            got = session.fused_depth_for_view(poses[4], torch.linalg.inv(syn.intrinsics(LIVE[1], LIVE[0]).float().cuda()), LIVE, return_color=True, **VIEW, **kw)
            want = vol.raycast(T, torch.linalg.inv(syn.intrinsics(LIVE[1], LIVE[0]).float().cuda()).reshape(1, 4, 4), LIVE, return_color=True, world_normals=True, **VIEW, **kw)
            assert set(got) == {"view_fused_depth", "view_fused_valid", "view_fused_flags", "view_fused_rgba"} | ({"view_fused_normals"} if kw else set())
            assert torch.equal(got["view_fused_rgba"], want["rgba"]) and tuple(got["view_fused_rgba"].shape) == (1, LIVE[0], LIVE[1], 4)
            assert torch.equal(got["view_fused_depth"], want["depth"]) and torch.equal(got["view_fused_flags"], want["flags"])
            assert (got["view_fused_rgba"][..., 3] == 255).float().mean().item() > 0.2
        mesh, by_hand = session.fused_mesh(return_colors=True), vol.extract_mesh(return_colors=True)
        assert set(mesh) == {"verts", "faces", "colors"} and len(mesh["colors"]) > 100
        for k in mesh:
            assert torch.equal(mesh[k], by_hand[k]), k
    assert not torch.equal(given.fusion_volume.colors, scaled.fusion_volume.colors)
    # with no new argument every key and bit is what it was, in a session with colours and in one without
    bare = _by_hand(maps_plain, origin, color=False)
    invK_live = torch.linalg.inv(syn.intrinsics(LIVE[1], LIVE[0]).float().cuda())
    T = torch.from_numpy(np.asarray(poses[4], np.float64).astype(np.float32))[None]
    want_view, want_mesh = bare.raycast(T, invK_live.reshape(1, 4, 4), LIVE, return_normals=True, **VIEW), bare.extract_mesh()
    assert plain.fusion_volume.colors is None and not coloured_unused.fusion_volume.colors.any()
    for session in (plain, coloured_unused, given):
        assert torch.equal(session.fusion_volume.values, bare.values) and torch.equal(session.fusion_volume.block_flags, bare.block_flags)
        got = session.fused_depth_for_view(poses[4], invK_live, LIVE, return_normals=True, **VIEW)
        assert set(got) == {"view_fused_depth", "view_fused_valid", "view_fused_flags", "view_fused_normals"}
        assert torch.equal(got["view_fused_depth"], want_view["depth"]) and torch.equal(got["view_fused_flags"], want_view["flags"])
        assert torch.equal(got["view_fused_normals"], want_view["normals"])
        mesh = session.fused_mesh()
        assert set(mesh) == {"verts", "faces"} and torch.equal(mesh["verts"], want_mesh["verts"]) and torch.equal(mesh["faces"], want_mesh["faces"])
    with pytest.raises(IdhError, match="color=True"):
        plain.fused_depth_for_view(poses[4], invK_live, LIVE, return_color=True)
    with pytest.raises(IdhError, match="color=True"):
        plain.fused_mesh(return_colors=True)
    given.reset()
    assert not given.fusion_volume.colors.any() and (given.fusion_volume.values[..., 1] == 0).all()


def test_depth_model_session_colours_its_volume_from_the_steps_frames():
    from implicit_depth_amd.streaming import StreamingSession

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    session = StreamingSession(_depth_model("dot", 2), num_source_views=2, buffer_size=BUFFER, query_keyframes=1)
    session.start_fusion(color=True, **FUSION)
    K_img = syn.intrinsics(IMG_W, IMG_H).float().cuda()
    images = _frames(9, (IMG_H, IMG_W), seed=5)
    maps = []
    for t in range(9):
        frame = _frame(t, poses)
        out, code = session.step(frame, world_T_cam=poses[t], dist_to_last_valid=dists[t], frame_u8=images[t], frame_K=K_img)
        if out is not None:
            maps.append((out["depth_pred_s0_b1hw"].clone(), poses[t], frame["invK_s0_b44"], images[t], K_img))
    assert len(maps) >= 2
    vol, sv = _by_hand(maps, _centred(maps[0][1])), session.fusion_volume
    assert float(sv.colors[..., 3].max()) > 0
    assert torch.equal(sv.values, vol.values) and torch.equal(sv.block_flags, vol.block_flags) and torch.equal(sv.colors, vol.colors)
