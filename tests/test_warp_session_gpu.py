"""The depth ring of a StreamingSession (remember_depth / warped_depth_for_view / the depth route of composite_asset) against the public
calls chained by hand: ``raster.warp_depth`` on the stored maps and ``compositing.composite_depth`` on its result, bit for bit.  What
``raster.warp_depth`` itself returns is held to the fp64 brute force in test_depth_warp_gpu.py.  Sessions are built as
tests/test_streaming_gpu.py builds its own; the DepthModel is the same holder with the regression decoder and no occlusion MLP."""
import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import warp_ref as WR
from hot_helpers import holder
from test_render_gpu import _asset_mesh
from test_streaming_gpu import BUFFER, IMG_H, IMG_W, D, _frame, _model, _RunOpts

pytestmark = pytest.mark.gpu
LIVE = (45, 60)  # the live camera's image for the plain queries: not the keyframe's 48 x 64


def _depth_model(volume, K):
    from implicit_depth_amd import backbone
    from implicit_depth_amd import networks as net

    m = holder(K, volume, IMG_H // 4, IMG_W // 4, D, decoder="depth", with_mlp=False, with_head=False)
    m.matching_model = net.ResnetMatchingEncoder(backbone.resnet18_stem(), 16)
    m.encoder = syn.StubImageEncoder()
    m.run_opts = _RunOpts(False)
    m.thresholder = None
    syn.fill_state_dict(m, seed=30)
    return m.cuda().eval()


def _by_hand(maps, live_pose, K, size, **kw):
    """``raster.warp_depth`` on (depth, world_T_cam, invK) triples, newest first."""
    from implicit_depth_amd import raster

    T = raster.relative_poses([live_pose], [p for _, p, _ in maps]).cuda()
    return raster.warp_depth(torch.cat([d for d, _, _ in maps]), torch.cat([k for _, _, k in maps]), T, K.reshape(1, 4, 4), size[0], size[1], **kw)


def _same_view(got, want, return_source):
    assert set(got) == {"view_warp_depth", "view_warp_valid"} | ({"view_warp_source"} if return_source else set())
    assert torch.equal(got["view_warp_depth"], want["depth"])
    assert got["view_warp_valid"].dtype == torch.bool and torch.equal(got["view_warp_valid"], (want["source"] >= 0)[:, None])
    if return_source:
        assert torch.equal(got["view_warp_source"], want["source"])


@pytest.mark.parametrize("query_keyframes", [1, 2])
def test_depth_model_session_warps_its_predictions_into_the_live_camera(query_keyframes):
    from implicit_depth_amd import AssetRenderer, compositing, raster
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    session = StreamingSession(_depth_model("dot", 2), num_source_views=2, buffer_size=BUFFER, query_keyframes=query_keyframes)
    verts, faces, colors = _asset_mesh(seed=1)
    asset = AssetRenderer(verts, faces, colors, world_T_asset=np.eye(4), ambient=0.3)
    K_img = syn.intrinsics(IMG_W, IMG_H).float().cuda()
    K_live = syn.intrinsics(LIVE[1], LIVE[0]).float().cuda()
    image = torch.randint(0, 256, (1, IMG_H, IMG_W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    with pytest.raises(IdhError, match="no prediction"):
        session.warped_depth_for_view(poses[0], K_live, LIVE)
    with pytest.raises(IdhError, match="no prediction"):
        session.composite_asset(image, asset, poses[0], K_img)
    maps, done = [], False
    for t in range(9):
        frame = _frame(t, poses)
        out, code = session.step(frame, world_T_cam=poses[t], dist_to_last_valid=dists[t])
        if out is not None:
            d = out["depth_pred_s0_b1hw"]
            assert tuple(d.shape) == (1, 1, IMG_H // 2, IMG_W // 2) and bool(torch.isfinite(d).all()) and bool((d > 0).all())
            maps.insert(0, (d.clone(), poses[t], frame["invK_s0_b44"]))
            continue
        if len(maps) < query_keyframes:
            continue
        last = maps[:query_keyframes]  # the ring: the last query_keyframes predictions, newest first
        for kw in (dict(), dict(return_source=True), dict(tear_ratio=float("inf"), empty_depth=7.0, return_source=True)):
            got = session.warped_depth_for_view(poses[t], K_live, LIVE, **kw)
            want = _by_hand(last, poses[t], K_live, LIVE, **{**kw, "return_source": True})
            _same_view(got, want, kw.get("return_source", False))
        cover = got["view_warp_valid"].float().mean().item()
        print(f"query_keyframes={query_keyframes} frame {t}: the rubber sheet of {len(last)} prediction(s) covers {cover:.3f} of the live view")
        assert cover > 0.2 and (got["view_warp_depth"][~got["view_warp_valid"]] == 7.0).all()
        if query_keyframes == 2:
            m = raster.decode_source(got["view_warp_source"], IMG_H // 2, IMG_W // 2)[0]
            assert set(m.unique().tolist()) <= {-1, 0, 1}
        # the whole frame by the depth route
        cam_T_mesh = torch.from_numpy(np.linalg.inv(poses[t]).astype(np.float32))[None].cuda()  # world_T_asset is the identity
        full = raster.render_shaded(asset.verts, asset.faces, cam_T_mesh, K_img[None], IMG_H, IMG_W, colors=asset.colors, ambient=0.3)
        assert 0.01 < (full["rgba"][0, ..., 3] > 0).float().mean() < 0.9
        for size in (None, (45, 60)):
            kw = {} if size is None else {"query_size": size}
            h, w = compositing.MODEL_SIZE if size is None else size
            Kq = K_img[None].clone()
            Kq[:, 0] *= w / IMG_W
            Kq[:, 1] *= h / IMG_H
            warped = _by_hand(last, poses[t], Kq, (h, w), empty_depth=session.WARP_FAR)["depth"]
            by_hand = compositing.composite_depth(image, warped, virtual_depth=full["depth"][:, 0], virtual_rgba=full["rgba"])
            parts = session.composite_asset(image, asset, poses[t], K_img, return_parts=True, **kw)
            assert torch.equal(parts["frame"], by_hand) and torch.equal(parts["asset_depth"], full["depth"]) and torch.equal(parts["asset_rgba"], full["rgba"])
            assert torch.equal(parts["view_warp_depth"], warped) and by_hand.shape == image.shape and by_hand.dtype == torch.uint8
            assert torch.equal(session.composite_asset(image, asset, poses[t], K_img, **kw), by_hand)
            faded = session.composite_asset(image, asset, poses[t], K_img, bgr=True, fade=[0.5], **kw)
            assert torch.equal(faded, compositing.composite_depth(image, warped, virtual_depth=full["depth"][:, 0], virtual_rgba=full["rgba"],
                                                                  fade=[0.5], bgr=True))
        done = True
        break
    assert done, "the sequence has no frame between keyframes after enough predictions"
    session.reset()
    with pytest.raises(IdhError, match="no prediction"):
        session.warped_depth_for_view(poses[0], K_live, LIVE)
    with pytest.raises(IdhError, match="no prediction"):
        session.composite_asset(image, asset, poses[0], K_img)


def test_bd_model_session_warps_a_supplied_map_and_answers_as_before():
    """Two sessions on models with the same weights see the same frames; one is also given lidar-like maps.  Its warp is
    ``raster.warp_depth``'s; everything else it returns is, bit for bit, what the other session returns."""
    from implicit_depth_amd import AssetRenderer
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    plain = StreamingSession(_model("mlp", 3), buffer_size=BUFFER, query_keyframes=2)
    ringed = StreamingSession(_model("mlp", 3), buffer_size=BUFFER, query_keyframes=2)
    verts, faces, colors = _asset_mesh(seed=1)
    asset = AssetRenderer(verts, faces, colors, world_T_asset=np.eye(4), ambient=0.3)
    K_img = syn.intrinsics(IMG_W, IMG_H).float().cuda()
    K_live = syn.intrinsics(LIVE[1], LIVE[0]).float().cuda()
    invK_src = torch.from_numpy(np.linalg.inv(WR.source_K()).astype(np.float32)).cuda()
    image = torch.randint(0, 256, (1, IMG_H, IMG_W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    with pytest.raises(IdhError, match="no prediction"):
        ringed.warped_depth_for_view(poses[0], K_live, LIVE)
    maps, predictions, done = [], 0, False
    for t in range(9):
        outs = [s.step(_frame(t, poses), world_T_cam=poses[t], dist_to_last_valid=dists[t]) for s in (plain, ringed)]
        assert outs[0][1] == outs[1][1] and (outs[0][0] is None) == (outs[1][0] is None)
        if outs[0][0] is not None:
            predictions += 1
            for k, v in outs[0][0].items():
                assert (v is None and outs[1][0][k] is None) or torch.equal(v, outs[1][0][k]), (t, k)
            lidar = torch.from_numpy(WR.source_depth(seed=t, box=t % 2 == 0) + np.float32(0.4))[None, None].cuda()
            ringed.remember_depth(lidar, poses[t], invK_src)  # (4,4) intrinsics, a host pose
            maps.insert(0, (lidar.clone(), poses[t], invK_src[None]))
            lidar.add_(100.0)  # the session keeps its own copy
            continue
        if predictions < 2:
            continue
        got = ringed.warped_depth_for_view(poses[t], K_live, LIVE, return_source=True)
        _same_view(got, _by_hand(maps[:2], poses[t], K_live, LIVE, return_source=True), True)
        cover = got["view_warp_valid"].float().mean().item()
        print(f"frame {t}: two supplied maps cover {cover:.3f} of the live view")
        assert 0.2 < cover < 1.0
        # the MLP's answers are untouched by the ring: the view query, the dense depth and the whole frame
        invK_live = torch.linalg.inv(K_live)
        depth = asset.render(poses[t], K_live, LIVE)["depth"]
        for a, b in ((plain.occlusion_for_view(depth, poses[t], invK_live, fill=-20.0), ringed.occlusion_for_view(depth, poses[t], invK_live, fill=-20.0)),
                     (plain.depth_for_view(poses[t], invK_live, LIVE), ringed.depth_for_view(poses[t], invK_live, LIVE)),
                     (plain.composite_asset(image, asset, poses[t], K_img, return_parts=True), ringed.composite_asset(image, asset, poses[t], K_img, return_parts=True))):
            assert set(a) == set(b) and "view_warp_depth" not in b
            for k in a:
                assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
        done = True
        break
    assert done
    with pytest.raises(IdhError):
        ringed.remember_depth(torch.ones(1, 1, 10, 12).cuda(), poses[0], invK_src)  # another size than the ring's maps
    with pytest.raises(IdhError):
        ringed.remember_depth(torch.ones(1, 24, 32).cuda(), poses[0], invK_src)
    ringed.reset()
    with pytest.raises(IdhError, match="no prediction"):
        ringed.warped_depth_for_view(poses[0], K_live, LIVE)
    ringed.remember_depth(torch.ones(1, 1, 10, 12).cuda(), poses[0], invK_src)  # an empty ring takes any size
