"""A StreamingSession whose TSDF volume follows the camera (start_fusion(follow=, on_scroll=)) against the public calls
chained by hand, byte for byte: ``fusion.follow_shift`` on the host, ``TSDFVolume.shift`` and ``TSDFVolume.integrate``.  What a shift
returns is held to the header in test_tsdf_shift_gpu.py.  The session and its supplied maps are those of tests/test_tsdf_session_gpu.py."""
import numpy as np
import pytest
import torch

import warp_ref as WR
from test_streaming_gpu import BUFFER, _model

pytestmark = pytest.mark.gpu
FUSION = dict(voxel_size=0.0625, dims=(24, 32, 40), color=True)  # 2.5 x 2 x 1.5 m around the first camera
FOLLOW = 0.5
MAPS = 8


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _inputs():
    """Eight supplied maps from a camera that walks 0.25 m in +x and 0.125 m in -z per map: (depth (1,1,24,32), pose, frame (1,24,32,3));
    WR.source_depth's room scaled to 0.3 of its depth - a wall about 0.6 m and a box about 0.37 m ahead - because the volume reaches
    only 0.75 m ahead of a camera at its centre (holes stay holes: 0, NaN, negative and infinite taps scale to themselves)."""
    frames = torch.randint(0, 256, (MAPS, 1, WR.SRC_H, WR.SRC_W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    out = []
    for t in range(MAPS):
        pose = np.eye(4)
        pose[:3, 3] = (0.3 + 0.25 * t, -0.2, 0.1 - 0.125 * t)
        depth = torch.from_numpy(WR.source_depth(seed=t, box=True) * np.float32(0.3))[None, None].cuda()
        out.append((depth, pose, frames[t]))
    return out


def _session():
    from implicit_depth_amd.streaming import StreamingSession

    return StreamingSession(_model("mlp", 3), buffer_size=BUFFER, query_keyframes=2)


def _centred(pose):
    nz, ny, nx = FUSION["dims"]
    return tuple(np.asarray(pose, np.float64)[:3, 3] - FUSION["voxel_size"] * 0.5 * (np.array([nx, ny, nz], np.float64) - 1.0))


def _same_volume(a, b):
    assert a.origin == b.origin and a.dims == b.dims
    assert torch.equal(_bytes(a.values), _bytes(b.values)) and torch.equal(_bytes(a.colors), _bytes(b.colors)) and torch.equal(a.block_flags, b.block_flags)


def test_session_volume_follows_the_camera_like_the_calls_by_hand():
    from implicit_depth_amd import fusion
    from implicit_depth_amd._lib import IdhError

    invK = torch.from_numpy(np.linalg.inv(WR.source_K()).astype(np.float32)).cuda()
    K = torch.linalg.inv(invK.reshape(1, 4, 4))  # as the session forms it
    maps = _inputs()
    session = _session()
    for bad in (dict(follow=0.0), dict(follow=-1.0), dict(follow=float("nan")), dict(on_scroll=print), dict(follow=0.5, on_scroll=3)):
        with pytest.raises(IdhError):
            session.start_fusion(**FUSION, **bad)
    seen = []  # what on_scroll was called with, and what was about to leave

    def on_scroll(volume, shift_xyz):
        assert volume is session.fusion_volume
        boxes = fusion.leaving_boxes(volume.dims, shift_xyz)
        leaving = sum(int((volume.crop(lo, hi).values[..., 1] > 0).sum()) for lo, hi in boxes if all(b > a for a, b in zip(lo, hi)))
        seen.append((tuple(shift_xyz), volume.origin, session.fusion_scrolls, len(boxes), leaving))

    session.start_fusion(**FUSION, follow=FOLLOW, on_scroll=on_scroll)
    assert session.fusion_scrolls == 0 and session.last_scroll is None
    hand = fusion.TSDFVolume(FUSION["dims"], FUSION["voxel_size"], _centred(maps[0][1]), color=True)
    shifts = []
    for t, (depth, pose, frame) in enumerate(maps):
        session.remember_depth(depth, pose, invK, frame_u8=frame)
        s = fusion.follow_shift(pose[:3, 3], hand.origin, hand.dims, hand.voxel_size, FOLLOW)
        if any(s):
            assert seen[-1][:3] == (s, hand.origin, len(shifts))  # called before the move, with the volume where it was
            hand.shift(s)
            shifts.append(s)
            assert session.last_scroll == s
        hand.integrate(depth, K, torch.from_numpy(np.linalg.inv(pose).astype(np.float32))[None], frame, K)
        assert session.fusion_scrolls == len(shifts) == len(seen)
        _same_volume(session.fusion_volume, hand)
    print(f"shifts {shifts}, on_scroll saw {seen}")
    # the camera walks 4 voxels in x and 2 in -z per map with a slack of 8: it leaves the slack more than once, and in both axes
    assert len(shifts) >= 2 and all(s[0] > 0 and s[1] == 0 for s in shifts) and any(s[2] < 0 for s in shifts)
    assert [x[0] for x in seen] == shifts
    assert any(x[4] > 0 for x in seen) and all(1 <= x[3] <= 2 for x in seen)  # observed voxels left the volume
    v = session.fusion_volume
    # (one map's frustum up to the wall 0.6 m ahead is a pyramid of about 0.6 / 3 * 0.66 * 0.5 m^3, 270 voxels, and the band of
    # 3 voxels either side of the wall's 0.33 m^2 holds about 500 coloured ones where it lies inside the grid; the walk drops most of
    # what earlier maps saw ahead of them, so the floors are fractions of ONE map's share)
    assert (v.values[..., 1] > 0).sum() > 200 and (v.colors[..., 3] > 0).sum() > 50
    # the camera has walked 1.75 m, more than half the grid's 2.5 m, and still stands inside the volume that followed it
    c = (maps[-1][1][:3, 3] - np.array(v.origin)) / FUSION["voxel_size"]
    assert (c > 0).all() and (c < np.array(FUSION["dims"][::-1]) - 1).all() and maps[-1][1][0, 3] - maps[0][1][0, 3] > 1.25
    last = fusion.TSDFVolume(FUSION["dims"], FUSION["voxel_size"], v.origin, color=True)
    last.integrate(maps[-1][0], K, torch.from_numpy(np.linalg.inv(maps[-1][1]).astype(np.float32))[None], maps[-1][2], K)
    assert (last.values[..., 1] > 0).sum() > 200
    # the consumers read the volume that moved
    out = session.fused_depth_for_view(maps[-1][1], invK, (WR.SRC_H, WR.SRC_W), near=0.3, far=2.0, return_color=True)
    want = hand.raycast(torch.from_numpy(maps[-1][1].astype(np.float32))[None], invK[None], (WR.SRC_H, WR.SRC_W), near=0.3, far=2.0, return_color=True)
    assert torch.equal(out["view_fused_depth"], want["depth"]) and torch.equal(out["view_fused_rgba"], want["rgba"])
    mesh, mesh_hand = session.fused_mesh(return_colors=True), hand.extract_mesh(return_colors=True)
    for k in mesh_hand:
        assert torch.equal(mesh[k], mesh_hand[k]), k
    # reset() clears the counters and a new sequence centres and follows again
    session.reset()
    assert session.fusion_scrolls == 0 and session.last_scroll is None
    n = len(seen)
    for depth, pose, frame in maps[:4]:
        session.remember_depth(depth, pose, invK, frame_u8=frame)
    again = fusion.TSDFVolume(FUSION["dims"], FUSION["voxel_size"], _centred(maps[0][1]), color=True)
    k = 0
    for depth, pose, frame in maps[:4]:
        s = fusion.follow_shift(pose[:3, 3], again.origin, again.dims, again.voxel_size, FOLLOW)
        if any(s):
            again.shift(s)
            k += 1
        again.integrate(depth, K, torch.from_numpy(np.linalg.inv(pose).astype(np.float32))[None], frame, K)
    _same_volume(session.fusion_volume, again)
    assert session.fusion_scrolls == k == len(seen) - n and k >= 1


def test_follow_none_is_the_fixed_grid():
    """``follow=None`` and a call without the new arguments give the same bytes, and nothing scrolls."""
    invK = torch.from_numpy(np.linalg.inv(WR.source_K()).astype(np.float32)).cuda()
    maps = _inputs()
    a, b = _session(), _session()
    a.start_fusion(**FUSION)
    b.start_fusion(**FUSION, follow=None, on_scroll=None)
    for depth, pose, frame in maps:
        for s in (a, b):
            s.remember_depth(depth, pose, invK, frame_u8=frame)
    _same_volume(a.fusion_volume, b.fusion_volume)
    assert a.fusion_scrolls == b.fusion_scrolls == 0 and a.last_scroll is None and b.last_scroll is None
    assert a.fusion_volume._spare is None and b.fusion_volume._spare is None  # no second set of tensors
    assert a.fusion_volume.origin == _centred(maps[0][1])
    assert (a.fusion_volume.values[..., 1] > 0).sum() > 200
