"""``StreamingSession.fused_mesh``: the session's own reconstruction handed to the mesh consumers.  The mesh's render and the ray cast
of the same volume are two interpolants of one field (linear along the grid's edges and flat over each triangle against trilinear
inside each cell), so they are held together by a geometric cap - one voxel diagonal on at least 99 % of the pixels both hit - that
the fp64 references must meet on their own first (no GPU needed for that)."""
import numpy as np
import pytest
import torch

import mesh_ref as M
import raster_ref as RR
import tsdf_ref as R

SCENE, POSE, CAM = "room24x32", "near", "30x44"
SHARE = 0.99


def _report(what, mesh_depth, cast_depth, diagonal):
    both = (mesh_depth > 0) & (cast_depth > 0)
    diff = np.abs(mesh_depth - cast_depth)[both]
    q = np.quantile(diff, [0.5, 0.9, 0.99, 1.0])
    within = float((diff <= diagonal).mean())
    print(f"{what}: mesh hits {int((mesh_depth > 0).sum())}, ray cast hits {int((cast_depth > 0).sum())}, both {int(both.sum())} of {both.size}; "
          f"|difference| median {q[0]:.4f} p90 {q[1]:.4f} p99 {q[2]:.4f} max {q[3]:.4f} m; within one voxel diagonal ({diagonal:.4f} m): {within:.4f}")
    return int(both.sum()), within


def test_the_fp64_references_alone_meet_the_cap():
    dims, v, origin = R.SCENES[SCENE][:3]
    values = R.reference_values(SCENE)
    E, iK, H, W = R.live_camera(POSE, CAM)
    cast = R.raycast(values, origin, v, E, iK, H, W, near=R.NEAR, max_steps=R.max_steps_for(v))
    mesh = M.extract(values, origin, v)
    K = np.linalg.inv(iK.astype(np.float64))
    depth, _ = RR.render(mesh["verts"], mesh["faces"], np.linalg.inv(E.astype(np.float64)), K, H, W)
    both, within = _report("fp64 references", depth, np.where((cast["flags"] & R.HIT) > 0, cast["depth"], -1.0), np.sqrt(3) * v)
    assert both > 0.2 * H * W and within >= SHARE


@pytest.mark.gpu
def test_fused_mesh_loads_into_the_rasterizer_and_agrees_with_the_fused_depth():
    from implicit_depth_amd import raster
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession
    from test_streaming_gpu import BUFFER, _model

    dims, v, origin, depth, K, cam_T_world = R.scene_inputs(SCENE)
    session = StreamingSession(_model("mlp", 3), buffer_size=BUFFER, query_keyframes=2)
    with pytest.raises(IdhError, match="start_fusion"):
        session.fused_mesh()
    session.start_fusion(voxel_size=v, dims=dims, origin=tuple(float(o) for o in origin))
    with pytest.raises(IdhError, match="no prediction"):
        session.fused_mesh()
    invK = torch.from_numpy(np.linalg.inv(K[0].astype(np.float64)).astype(np.float32)).cuda()
    for m in range(depth.shape[0]):
        session.remember_depth(torch.from_numpy(depth[m:m + 1]).cuda(), R.KEY_POSES[m], invK)
    mesh = session.fused_mesh()
    assert mesh["verts"].dtype == torch.float32 and mesh["faces"].dtype == torch.int32 and mesh["faces"].shape[0] > 300
    ref = M.extract(session.fusion_volume.values.cpu().numpy(), origin, v)
    assert np.array_equal(mesh["faces"].cpu().numpy(), ref["faces"])
    assert mesh["faces"].shape[0] > session.fused_mesh(min_weight=1.0)["faces"].shape[0] > 0
    E, iK, H, W = R.live_camera(POSE, CAM)
    rasterizer = raster.MeshDepthRasterizer(H, W)
    rasterizer.load_gt_mesh(verts=mesh["verts"], faces=mesh["faces"])  # unchanged: tensors on the GPU, int32 faces
    assert torch.equal(rasterizer.gt_mesh[0], mesh["verts"]) and torch.equal(rasterizer.gt_mesh[1], mesh["faces"].long())
    cam = torch.from_numpy(np.linalg.inv(E.astype(np.float64)).astype(np.float32))[None].cuda()
    Kl = torch.from_numpy(np.linalg.inv(iK.astype(np.float64)).astype(np.float32))[None].cuda()
    rendered = rasterizer.render_depth(cam, Kl, mesh=rasterizer.gt_mesh)[0, 0].cpu().numpy().astype(np.float64)
    view = session.fused_depth_for_view(R.LIVE_POSES[POSE], torch.from_numpy(iK).cuda(), (H, W), near=R.NEAR, far=R.FAR)
    cast = np.where(view["view_fused_valid"][0, 0].cpu().numpy(), view["view_fused_depth"][0, 0].cpu().numpy().astype(np.float64), -1.0)
    both, within = _report("session", rendered, cast, np.sqrt(3) * v)
    assert both > 0.2 * H * W and within >= SHARE
    # the consumers take it as it is: the vertex sampling of the temporal evaluation, and a PLY file
    rasterizer.update_gt_vertex_predictions(torch.from_numpy(cast.astype(np.float32))[None, None].cuda(), cam, Kl)
    seen = rasterizer.gt_vertex_predictions[0]
    assert tuple(seen.shape) == (mesh["verts"].shape[0],) and (seen > 0).sum() > 100
