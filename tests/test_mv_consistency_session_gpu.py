"""The consistency check of a StreamingSession (start_fusion(consistency=, weighted=)): a wall seen from three poses,
the third map carrying a patch of flying pixels in front of the wall.  With the check the patch leaves nothing in the volume and the
fused view through it shows the wall; without it the session makes the calls it made before, bit for bit.  What the kernels return is
held to fp64 in test_mv_consistency_gpu.py.  Sessions are built as tests/test_warp_session_gpu.py builds its own."""
import numpy as np
import pytest
import torch

import mv_consistency_ref as R
import tsdf_ref
from test_streaming_gpu import BUFFER
from test_warp_session_gpu import _depth_model

pytestmark = pytest.mark.gpu

H, W = 30, 41
FUSION = dict(voxel_size=0.05, dims=(64, 40, 56), origin=(-1.2, -1.0, -0.6), trunc_voxels=3.0, max_weight=64.0)
PATCH = (slice(11, 17), slice(18, 26))  # rows, columns of the third map
FACTOR = 0.6                             # the patch floats at 0.6 of the wall's depth: 0.8 m in front of it, far more than the truncation


def _scene():
    """[(depth (1,1,H,W) cuda, world_T_cam float64, invK (1,4,4) cuda)] of the wall z = 2 from three poses, and the clean third map."""
    K = tsdf_ref._pinhole(36.0, 36.0, W / 2, H / 2)
    maps = []
    for x, ry in ((-0.2, 0.05), (0.0, -0.03), (0.2, -0.08)):
        T = tsdf_ref._pose(ry, 0.02, 0.0, np.array([x, 0.0, 0.0]))
        d = R._wall_depth(H, W, K, T).astype(np.float32)[None, None]
        maps.append([torch.from_numpy(d).cuda(), T, torch.from_numpy(np.linalg.inv(K).astype(np.float32))[None].cuda()])
    clean = maps[2][0].clone()
    maps[2][0][0, 0][PATCH] *= FACTOR
    return maps, clean


def _session(**fusion):
    from implicit_depth_amd.streaming import StreamingSession

    s = StreamingSession(_depth_model("dot", 2), num_source_views=2, buffer_size=BUFFER, query_keyframes=3)
    s.start_fusion(**FUSION, **fusion)
    return s


def _volume():
    from implicit_depth_amd import fusion

    return fusion.TSDFVolume(FUSION["dims"], FUSION["voxel_size"], FUSION["origin"], FUSION["trunc_voxels"], FUSION["max_weight"])


def _cams(pose, invK):
    return torch.linalg.inv(invK.reshape(1, 4, 4)), torch.from_numpy(np.linalg.inv(np.asarray(pose, np.float64)).astype(np.float32))[None]


def _by_hand(maps, weights=None):
    vol = _volume()
    for m, (d, pose, invK) in enumerate(maps):
        vol.integrate(d, *_cams(pose, invK), **({} if weights is None or weights[m] is None else {"weight": weights[m]}))
    return vol


def _same(a, b):
    return torch.equal(a.values, b.values) and torch.equal(a.block_flags, b.block_flags)


def test_flying_pixels_stay_out_of_the_volume():
    maps, clean = _scene()
    checked, plain = _session(consistency=dict(log_tol=0.05)), _session()
    for d, pose, invK in maps:
        checked.remember_depth(d, pose, invK)
        plain.remember_depth(d, pose, invK)
    counts = checked.last_depth_counts
    assert counts.shape == (1, 3, H, W) and counts.dtype == torch.uint8
    patch = torch.zeros(H, W, dtype=torch.bool, device="cuda")
    patch[PATCH] = True
    assert (counts[0, 2][patch] >= 1).all() and (counts[0, 1][patch] == 0).all()  # both older maps saw through the patch
    assert (counts[0, 2][~patch] == 0).all() and (counts[0, 1][~patch] >= 1).float().mean() > 0.9
    # the ring keeps the raw maps, newest first: the warp path is unchanged
    assert len(checked._depth_ring) == 3 and all(torch.equal(r[0], m[0]) for r, m in zip(checked._depth_ring, maps[::-1]))
    # the volume: the third map with the patch punched out (and the few border pixels no older map covers), the others as they are
    third = maps[2][0].clone()
    ok3 = (counts[0, 1] >= 1) & (counts[0, 2] == 0)
    third[0, 0][~ok3] = 0
    assert not ok3[patch].any() and ok3[~patch].float().mean() > 0.9
    from implicit_depth_amd import geometry

    K1, E1 = _cams(maps[0][1], maps[0][2])
    c2 = geometry.depth_consistency(maps[1][0], maps[1][2], torch.from_numpy(maps[1][1].astype(np.float32))[None].cuda(), maps[0][0][None], K1[None].cuda(),
                                    E1[None].cuda(), log_tol=0.05)
    second = c2["filtered_depth"]
    by_hand = _by_hand([maps[0], (second, *maps[1][1:]), (third, *maps[2][1:])])
    assert _same(checked.fusion_volume, by_hand) and not _same(checked.fusion_volume, plain.fusion_volume)
    # the voxels of the patch's band - where the unchecked volume holds the patch's surface - are plain free space in the checked one:
    # T == 1 from the older maps, which saw through them, and fewer observations.  (W == 0 cannot be: a voxel a source sees through,
    # which is what makes the conflict, is a voxel that source observed.)
    vc, vp = checked.fusion_volume.values, plain.fusion_volume.values
    band = (vp[..., 0] < 0.8) & (vc[..., 0] == 1)
    assert band.sum() > 10 and (vc[..., 1][band] < vp[..., 1][band]).all()
    # through the patch the fused view shows the wall
    view_c = checked.fused_depth_for_view(maps[2][1], maps[2][2], (H, W), near=0.3, far=4.0)
    view_p = plain.fused_depth_for_view(maps[2][1], maps[2][2], (H, W), near=0.3, far=4.0)
    inner = torch.zeros_like(patch)
    inner[PATCH[0].start + 1:PATCH[0].stop - 1, PATCH[1].start + 1:PATCH[1].stop - 1] = True
    assert view_c["view_fused_valid"][0, 0][inner].all() and view_p["view_fused_valid"][0, 0][inner].all()
    wall, got_c, got_p = clean[0, 0][inner], view_c["view_fused_depth"][0, 0][inner], view_p["view_fused_depth"][0, 0][inner]
    print(f"through the patch: wall {wall.mean():.3f} m, checked {got_c.mean():.3f} m, unchecked {got_p.mean():.3f} m")
    assert ((got_c - wall).abs() < FUSION["voxel_size"]).all()


def test_without_consistency_the_session_makes_the_calls_it_made():
    maps, _ = _scene()
    session = _session()
    for d, pose, invK in maps:
        session.remember_depth(d, pose, invK)
    assert _same(session.fusion_volume, _by_hand(maps)) and session.last_depth_counts is None and session._ring_cams == []
    assert len(session._depth_ring) == 3 and all(torch.equal(r[0], m[0]) and torch.equal(r[2], m[2]) for r, m in zip(session._depth_ring, maps[::-1]))


def test_weighted_fusion_with_every_count_zero_is_plain_fusion():
    """Cameras that look away from each other: nothing is visible anywhere, every count is 0, and with min_consistent = 0 every valid
    sample is kept at weight 1 + 0 - the bits of the unweighted call."""
    from implicit_depth_amd._lib import IdhError

    maps, _ = _scene()
    maps[1][1] = tsdf_ref._pose(np.pi, 0.0, 0.0, np.array([0.0, 0.0, 1.0]))  # behind the first camera, looking the other way
    maps[1][0] = torch.full_like(maps[1][0], 1.5)
    maps = maps[:2]
    weighted, plain = _session(consistency=dict(min_consistent=0), weighted=True), _session()
    for d, pose, invK in maps:
        weighted.remember_depth(d, pose, invK)
        plain.remember_depth(d, pose, invK)
    assert weighted.last_depth_counts is not None and not weighted.last_depth_counts.any()
    assert _same(weighted.fusion_volume, plain.fusion_volume) and float(plain.fusion_volume.values[..., 1].max()) >= 1
    # weights at work: the patch scene again, the raw third map at the check's weights equals the call by hand
    maps, _ = _scene()
    session = _session(consistency=dict(log_tol=0.05), weighted=True)
    for d, pose, invK in maps:
        session.remember_depth(d, pose, invK)
    assert float(session.fusion_volume.values[..., 1].max()) > 3  # 1 + 2 + 3: agreeing maps weigh more
    with pytest.raises(IdhError, match="consistency"):
        _session(weighted=True)
    with pytest.raises(IdhError, match="unknown"):
        _session(consistency=dict(tolerance=0.1))
