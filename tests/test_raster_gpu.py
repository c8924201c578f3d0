"""Mesh depth rasteriser and temporal evaluation on the GPU (csrc/raster.hip, raster.py, evaluation.TemporalEvaluator) against the
closed-form plane depth and the fp64 brute force of tests/raster_ref.py.  What counts as ambiguous (and is left out of the exact
comparisons) is defined there; test_raster_cpu.py checks that the scenes used here stay under the 1 % caps."""
import argparse
import math

import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import raster_ref as rr

pytestmark = pytest.mark.gpu
RTOL = 1e-4  # the project's bar (README: "< 1e-4 of scale")
CELL = 0.025


def _pose(ry=0.0, t=(0.0, 0.0, 0.0)):
    T = syn._rot_y(ry)
    T[0, 3], T[1, 3], T[2, 3] = t
    return T


def test_plane_matches_the_closed_form_without_holes():
    from implicit_depth_amd.raster import MeshDepthRasterizer

    H, W, dist = 192, 256, 2.0
    r = MeshDepthRasterizer(H, W)
    r.create_plane_from_camera(syn.plane_pose(0).cuda(), distance=torch.tensor(dist))
    world_T_cam = [_pose(), _pose(0.0, (0.5, -0.3, 0.4)), _pose(0.1, (0.1, 0.0, 0.0)), _pose(1.45, (0.0, 0.1, 0.0)), _pose(math.pi, (0.0, 0.0, 0.5))]
    cams = torch.stack([torch.linalg.inv(T) for T in world_T_cam]).float()
    K = syn.intrinsics(W, H).float()[None].expand(len(cams), 4, 4).contiguous()
    got = r(cams.cuda(), K.cuda())
    torch.cuda.synchronize()
    assert tuple(got.shape) == (len(cams), 1, H, W) and got.dtype == torch.float32
    got = got.cpu().numpy()[:, 0].astype(np.float64)
    kinds = []
    for b in range(len(cams)):
        t, margin = rr.plane_depth(syn.plane_pose(0)[0].numpy(), dist, cams[b].numpy(), K[b].numpy(), H, W)
        with np.errstate(invalid="ignore"):
            inside = np.isfinite(t) & (t > 0) & (margin > CELL)
            outside = ~np.isfinite(t) | (t <= 0) | (margin < -CELL)
        band = ~(inside | outside)
        err = np.abs(got[b][inside] - t[inside]) / t[inside]
        print(f"view {b}: inside {inside.mean():.3f} outside {outside.mean():.3f} band {band.mean():.4f} max rel err {err.max() if err.size else 0:.2e} "
              f"holes {(got[b][inside] <= 0).sum()} stray {(got[b][outside] != -1).sum()}")
        assert band.mean() < 0.01
        assert (got[b][inside] > 0).all(), f"view {b}: {(got[b][inside] <= 0).sum()} holes in the plane"
        assert err.size == 0 or err.max() < RTOL, (b, err.max())
        assert (got[b][outside] == -1).all(), b
        kinds.append((inside.any(), outside.any()))
    assert kinds[0] == (True, False) and kinds[2] == (True, False) and kinds[3] == (True, True) and kinds[4] == (False, True)


@pytest.mark.parametrize("case", [0, 1])
def test_general_mesh_matches_the_brute_force(case):
    from implicit_depth_amd import raster

    name, H, W, verts, faces, cams, K = list(rr.general_cases())[case]
    got = raster.render_depth(verts.cuda(), faces.cuda(), cams.cuda(), K.cuda(), H, W)
    again = raster.render_depth(verts.cuda(), faces.cuda(), cams.cuda(), K.cuda(), H, W)
    torch.cuda.synchronize()
    assert torch.equal(got, again), "two renders of the same scene differ"
    one = raster.render_depth(verts.cuda(), faces.cuda(), cams[1:].cuda(), K[1:].cuda(), H, W)
    assert torch.equal(one[0], got[1]), "a camera's render depends on its place in the batch"
    for b in range(2):
        ref, amb = rr.render(verts.numpy(), faces.numpy(), cams[b].numpy(), K[b].numpy(), H, W)
        wrong, err, empties = rr.compare_render(got[b, 0].cpu().numpy(), ref, amb)
        print(f"{name} view {b}: ambiguous {amb.mean():.4%}, coverage mismatches {wrong}, max rel depth err {err:.2e}")
        assert amb.mean() <= rr.AMBIGUOUS_CAP
        assert wrong == 0 and empties, (name, b, wrong)
        assert err < RTOL, (name, b, err)


def test_meshes_that_draw_nothing():
    from implicit_depth_amd import raster

    cams, K = torch.eye(4)[None].cuda(), syn.intrinsics(40, 30).float()[None].cuda()
    verts = torch.tensor([[0.0, 0.0, 1.0], [float("nan"), 0.0, 1.0], [0.0, float("inf"), 1.0], [0.1, 0.0, 1.0], [0.0, 0.1, 1.0]]).cuda()
    for faces in (torch.zeros(0, 3, dtype=torch.int64), torch.tensor([[0, 1, 3], [0, 2, 4], [0, 0, 3], [0, 3, 77], [-1, 3, 4]])):
        out = raster.render_depth(verts, faces.cuda(), cams, K, 30, 40)
        assert (out == -1).all()
    out = raster.render_depth(verts, torch.tensor([[0, 3, 4], [0, 1, 3]]).cuda(), cams, K, 30, 40)
    assert ((out == -1) | (out == 1.0)).all() and (out == 1.0).any()


def _run_track(case):
    from implicit_depth_amd import TemporalEvaluator

    verts, faces, cams, K, preds = case
    H, W = preds.shape[-2:]
    ev = TemporalEvaluator()
    ev.initialise_new_scene(verts=verts, faces=faces, height=H, width=W)
    ev.rasterizer.gt_vertex_predictions = []
    for t in range(len(cams)):
        ev.update_vertex_predictions(preds[t].clone().cuda(), cams[t].cuda(), K.cuda())
    ev.compute_vertex_occlusion_changes()
    torch.cuda.synchronize()
    got = torch.stack(ev.rasterizer.gt_vertex_predictions).cpu().numpy().astype(np.float64)
    ref, amb = rr.track_reference(verts, faces, cams, K, preds)
    return ev, got, ref, amb


def test_vertex_predictions_and_flip_count_match_the_brute_force():
    ev, got, ref, amb = _run_track(rr.track_case())
    assert (amb.mean(1) <= rr.AMBIGUOUS_CAP).all()
    bad = (got != ref.astype(np.float32)) & ~amb
    print(f"track: ambiguous pairs {amb.sum()}, mismatches outside them {bad.sum()}, total_diffs {ev.total_diffs} vs {rr.occlusion_changes(ref)}")
    assert bad.sum() == 0
    assert ev.total_verts == got.shape[1]
    assert abs(ev.total_diffs - rr.occlusion_changes(ref)) <= amb.sum()
    # the integer count equals the statement applied to what the GPU sampled, exactly
    assert ev.total_diffs == rr.occlusion_changes(got)


def test_static_scene_without_borderline_cases_is_exact():
    ev, got, ref, amb = _run_track(rr.static_case())
    assert amb.sum() == 0
    np.testing.assert_array_equal(got, ref.astype(np.float32))
    assert ev.total_diffs == rr.occlusion_changes(ref) > 10


def test_flip_count_kernel_on_seeded_histories():
    from implicit_depth_amd.raster import vertex_occlusion_changes

    for T, V, seed in ((6, 500, 1), (2, 64, 2), (30, 200000, 3), (1, 10, 4)):
        h = syn.vertex_histories(T, V, seed)
        h[0, 0] = float("nan")
        assert vertex_occlusion_changes(h.cuda()) == rr.occlusion_changes(h.numpy())


def test_temporal_eval_loop_end_to_end():
    """INTEGRATION.md §2e on a short synthetic sequence with carried prior: plumbing, not numerics."""
    from bench import TemporalWorkload
    from implicit_depth_amd import TemporalEvaluator, temporal_final_metrics
    from implicit_depth_amd import evaluation as ev_keys
    from implicit_depth_amd.evaluation import bd_frame_scores

    dev = torch.device("cuda:0")
    wl = TemporalWorkload(argparse.Namespace(batch=1, sequences=1, views=2, planes=16, height=96, width=128, volume="mlp", conv_math="fp32", mlp_math="fp32"), dev, 0)
    h, w = wl.rd.shape[-2:]
    verts, faces, _, _ = syn.raster_scene(h, w, seed=5, cells=24)
    eval_length, warmup, n_frames = 4, 1, 8
    ev = TemporalEvaluator()
    ev.initialise_new_scene(verts=verts, faces=faces, height=h, width=w)
    gt = (2.6 + 0.8 * torch.from_numpy(syn.smooth_field((1, 1, 2 * h, 2 * w), 9, "e2e_gt")).float()).to(dev)
    depth_lo = gt[:, :, ::2, ::2].contiguous()
    rows, count = [], 0
    with torch.inference_mode():
        for i in range(n_frames):
            world_T_cam, cam_T_world = wl.poses[wl.t % len(wl.poses)]
            if i % eval_length == 0:
                ev.initialise_new_plane(gt, world_T_cam)
                count = 0
            rendered = ev.rasterizer(cam_T_world, wl.K0)
            assert tuple(rendered.shape) == tuple(wl.rd.shape) and (rendered > 0).all()
            wl.rd = rendered
            wl.step()  # carries sigmoid(pred_0) and cam_T_world as the next frame's prior
            ev.mask_prediction_edges(wl.prev[0])  # test_bd.py:219, INTEGRATION.md 2e: the carried prior's border is unreliable
            outputs = {"pred_0": wl.out["pred_0"]}
            count += 1
            if count < warmup + 1:
                continue
            ev.update_vertex_predictions(torch.sigmoid(outputs["pred_0"]).clone(), cam_T_world, wl.K0)
            if i % (eval_length - 1) == 0:
                ev.compute_vertex_occlusion_changes()
            scores, keep = bd_frame_scores(outputs, {"depth_b1hw": depth_lo, "rendered_depth": rendered, "full_res_depth_b1hw": gt}, temporal_eval=True)
            rows.append(scores)
    torch.cuda.synchronize()
    final = {k: torch.stack([r[k] for r in rows]).nanmean().item() for k in rows[0]}
    final.update(temporal_final_metrics(ev.total_diffs, eval_length, warmup, 2, 1))
    # the reference's key set under temporal_eval: one query plane named -1.0, constant thresholds 0.3 .. 0.7, three families
    fam = [f"iou{s}_{t:.1f}_d_-1.0" for t in (0.3, 0.4, 0.5, 0.6, 0.7) for s in ("", "_pos", "_neg")]
    expected = fam + [f"{tag}_{k}" for tag in ("surface", "boundary") for k in fam]
    assert list(rows[0]) == expected == ev_keys.bd_score_keys(1, temporal_eval=True)
    assert list(final) == expected + ["total_diffs_d_-1.0", "temporal_score_d_-1.0"]
    assert ev.total_verts > 0 and math.isfinite(final["total_diffs_d_-1.0"]) and math.isfinite(final["temporal_score_d_-1.0"])
    # the untagged family is finite in every frame.  surface_* / boundary_* may be NaN in a frame, as in the reference: a fronto-parallel
    # query plane may have no pixel within 5 % of the depth map / no occlusion edge, and an IoU over an empty mask is 0 / 0
    assert all(torch.isfinite(r[k]).all() for r in rows for k in fam)
