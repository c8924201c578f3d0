"""Sparse occlusion queries on the GPU: idh_binary_mlp_rays_fwd and idh_project_points_fwd called by hand on hostile buffers
(tests/ray_query_ref.py: case tables, fp64 restatement, derived elementwise bound), then the same kernels through HotPath.forward /
query_rays / query_points, dropin.fused_forward and StreamingSession at the smallest model shapes the other end-to-end tests use."""
import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import mlp_op_ref as R
import ray_query_ref as Q
from hot_helpers import holder, to_cuda

pytestmark = pytest.mark.gpu


def _lib():
    from implicit_depth_amd import _lib as L

    return L.lib()


def _hold(got, ref, tol, what):
    """|got - ref| <= tol elementwise; prints the worst err / bound."""
    got, ref, tol = got.double().cpu(), ref.double().cpu(), tol.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    ratio = ((got - ref).abs() / tol).max().item()
    print(f"{what}: worst err/bound {ratio:.3g} (max err {(got - ref).abs().max().item():.3g}, n = {got.numel()})")
    assert ratio <= 1.0, (what, ratio)
    return ratio


# ---- the op ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Q.RAY_CASES, ids=lambda c: c.name)
def test_rays_op_within_the_derived_bound(case):
    feat, rays, depths, prior = Q.case_inputs(case)
    m = R.make_net(case.cf, case.has_prior, R._seed(case.name))
    rc, out = Q.run_rays(_lib(), case, m, feat, rays, depths, prior)
    assert rc == Q.OK
    got, clean = out.read()
    assert clean, "a store outside out (B, Nq, S)"
    ref, tol = Q.ray_bound(R.weights64(m), feat, rays, depths, prior if prior is not None else case.prior, case.grid, case.step)
    _hold(got.view(case.B, case.Nq, case.S), ref, tol, case.name)
    # rays more than a pixel outside: all-zero feature, finite logit
    zero = (Q.sample64(torch.ones(case.B, 1, case.H, case.W), rays[:, ::case.step], case.grid)[:, 0] == 0)
    if zero.any():
        assert bool(torch.isfinite(got.view(case.B, case.Nq, case.S)[zero]).all())


# ---- projection -----------------------------------------------------------------------------------------------------
def test_project_points_rays_depth_valid_and_prior():
    from implicit_depth_amd import mlp

    B, H, W, N = Q.PROJ_B, Q.PROJ_H, Q.PROJ_W, Q.PROJ_N
    pts, cTw, K, prior, pcTw, pK = Q.projection_inputs()
    ref = Q.projection_reference(pts, cTw, K, H, W)
    pval, sx, sy, pcz = Q.prior_nearest_reference(pts, pcTw, pK, prior, H, W)
    share = Q.near_boundary_share(ref, sx, sy, pcz, H, W)
    assert share == 0.0, share  # nothing is filtered below: the table keeps clear of every boundary
    L = _lib()
    from implicit_depth_amd import _lib as lib

    d = [t.cuda().contiguous() for t in (pts, cTw, K, prior, pcTw, pK)]
    rays, depth, pr = R.Out(B * N * 2), R.Out(B * N), R.Out(B * N)
    valid = torch.full((B * N + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = L.idh_project_points_fwd(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), B, N, H, W, rays.ptr, depth.ptr, valid.data_ptr() + 8,
                                  d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), pr.ptr, lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == Q.OK
    (gr, c1), (gd, c2), (gp, c3) = rays.read(), depth.read(), pr.read()
    v = valid.cpu()
    assert c1 and c2 and c3 and bool((v[:8] == 0x5A).all()) and bool((v[8 + B * N:] == 0x5A).all())
    _hold(gr.view(B, N, 2), ref["rays"], ref["e_rays"], "project rays")
    _hold(gd.view(B, N), ref["depth"], ref["e_depth"], "project depth")
    u, vv, cz = ref["rays"][..., 0], ref["rays"][..., 1], ref["cz"]
    want_valid = (cz > 0) & (u >= 0) & (u < W) & (vv >= 0) & (vv < H)
    assert torch.equal(v[8:8 + B * N].view(B, N).bool(), want_valid)
    assert torch.equal(gp.view(B, N), pval.float())  # the prior's own fp32 values, or -1
    # the Python wrapper: the same launch, with and without a prior
    r2, d2, v2, p2 = mlp.project_points(d[0], d[1], d[2], H, W, d[3], d[4], d[5])
    assert torch.equal(r2.cpu().view(-1), gr) and torch.equal(d2.cpu().view(-1), gd) and torch.equal(v2.cpu(), want_valid) and torch.equal(p2.cpu().view(-1), gp)
    r3, d3, v3, p3 = mlp.project_points(d[0], d[1], d[2], H, W)
    assert p3 is None and torch.equal(r3, r2) and torch.equal(d3, d2) and torch.equal(v3, v2)


# ---- pipeline -------------------------------------------------------------------------------------------------------
def _build(B, K, H, W, D, P, use_prior=False, seed=0):
    """As tests/test_pipeline_gpu.py: the small BD model on synthetic inputs (s0 map 2H x 2W)."""
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from implicit_depth_amd.pipeline import HotPath

    enc_ch = [24, 48, 64, 160, 256]
    cve = net.CVEncoder(D, enc_ch[1:], [64, 128, 256, 384])
    dec = net.BDDecoderPP(enc_ch[:1] + cve.num_ch_enc)
    mlp = net.BinaryMLPNetwork(dec.num_ch_dec, use_prior=use_prior)
    for i, m in enumerate([cve, dec, mlp]):
        syn.fill_state_dict(m, seed=seed + 50 + i, gain=1.1 if i == 2 else 1.0)
    inp = syn.cost_volume_inputs(B, K, 16, H, W, seed=seed, behind_view=K - 1)
    pyr = syn.encoder_pyramid(B, H * 4, W * 4, seed=seed)
    rd = syn.rendered_depth_planes(B, H * 2, W * 2, P)
    return HotPath(CostVolumeManager(H, W, D), cve, dec, mlp).cuda(), {k: v.cuda() for k, v in inp.items()}, [t.cuda() for t in pyr], rd.cuda()


def _fwd(model, d, pyr, **kw):
    return model(d["cur_feats"], d["src_feats"], pyr, d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"], **kw)


def _rays_in(B, N, gh, gw, seed):
    g = torch.Generator().manual_seed(seed)
    rays = torch.rand((B, N, 2), generator=g) * torch.tensor([gw + 3.0, gh + 3.0]) - 1.5  # up to 1.5 px outside on every side
    depths = 0.5 + 5 * torch.rand((B, N, 3), generator=g)
    return rays, depths


def test_forward_with_query_rays_matches_the_composition():
    """forward(query_rays=..., query_scales=(0,1,2,3)) against the composition a caller had before: export the four maps, float64 grid_sample,
    float64 MLP.  The exported maps are copies of the plan's buffers, so the op's own bound applies; with and without rendered_depth."""
    B, K, H, W, D, P = 2, 2, 16, 24, 16, 2
    model, d, pyr, rd = _build(B, K, H, W, D, P)
    grid = (4 * H, 4 * W)  # the rays live on a grid twice the s0 map
    rays, depths = _rays_in(B, 37, *grid, seed=11)
    rc = rays.cuda()
    keep = rc.clone()
    out = _fwd(model, d, pyr, rendered_depth=rd, return_features=True, query_rays=rc, query_depths=depths.cuda(), query_grid=grid, query_scales=(0, 1, 2, 3))
    assert torch.equal(rc, keep) and out["pred_0"].shape == (B, P, 2 * H, 2 * W)
    w = R.weights64(model.binary_mlp)
    for s in range(4):
        feat = out[f"feature_s{s}_b1hw"].cpu()
        ref, tol = Q.ray_bound(w, feat, rays, depths, None, grid, step=s + 1, scale=s)
        got = out[f"ray_pred_{s}"]
        assert got.shape == (B, 1, -(-37 // (s + 1)), 3)
        _hold(got[:, 0], ref, tol, f"forward ray_pred_{s}")
    # without rendered_depth and without the exports: scale 0 only, the same bits; the coarse scales are then refused
    out0 = _fwd(model, d, pyr, query_rays=rc, query_depths=depths.cuda(), query_grid=grid)
    assert "pred_0" not in out0 and set(k for k in out0 if k.startswith("ray_pred")) == {"ray_pred_0"}
    assert torch.equal(out0["ray_pred_0"], out["ray_pred_0"])
    from implicit_depth_amd._lib import IdhError

    with pytest.raises(IdhError, match="scales"):
        model.query_rays(rc, depths.cuda(), grid=grid, scales=(1,))
    again = model.query_rays(rc, depths.cuda(), grid=grid)
    assert torch.equal(again["ray_pred_0"], out["ray_pred_0"])


def test_pixel_centre_rays_agree_with_the_plane_path():
    B, K, H, W, D, P = 1, 2, 16, 24, 16, 3
    model, d, pyr, rd = _build(B, K, H, W, D, P, use_prior=True)
    Hs, Ws = 2 * H, 2 * W
    g = torch.Generator().manual_seed(3)
    N = 41
    px, py = torch.randint(0, Ws, (B, N), generator=g), torch.randint(0, Hs, (B, N), generator=g)
    px[0, :4], py[0, :4] = torch.tensor([0, Ws - 1, 0, Ws - 1]), torch.tensor([0, 0, Hs - 1, Hs - 1])  # the four corner pixels
    rays = torch.stack([px + 0.5, py + 0.5], -1).float()
    bi = torch.arange(B).view(B, 1)
    depths = rd.cpu()[bi, :, py, px]  # (B, N, P): the planes' own depths at those pixels
    out = _fwd(model, d, pyr, rendered_depth=rd, return_features=True, query_rays=rays.cuda(), query_depths=depths.cuda())
    feat = out["feature_s0_b1hw"].cpu()
    w = R.weights64(model.binary_mlp)
    ref_r, tol_r = Q.ray_bound(w, feat, rays, depths, -1.0, (Hs, Ws))
    ref_p, tol_p = R.logit_bound(w, feat.flatten(2), rd.cpu().flatten(2), torch.full((B, P, Hs * Ws), -1.0))
    plane = out["pred_0"].cpu()[bi, :, py, px]  # B, N, P
    tol = tol_r + tol_p.view(B, P, Hs, Ws)[bi, :, py, px] + (ref_r - ref_p.view(B, P, Hs, Ws)[bi, :, py, px]).abs()
    _hold(out["ray_pred_0"][:, 0], plane, tol, "pixel-centre rays vs pred_0")
    _hold(out["ray_pred_0"][:, 0], ref_r, tol_r, "pixel-centre rays vs fp64")


def test_query_points_equals_forward_with_projected_rays():
    B, K, H, W, D, P = 2, 2, 16, 24, 16, 1
    model, d, pyr, rd = _build(B, K, H, W, D, P, use_prior=True)
    Hs, Ws = 2 * H, 2 * W
    K0 = torch.stack([syn.intrinsics(Ws, Hs).float()] * B).cuda()
    wTc = torch.stack([syn.source_pose(b + 1).float() for b in range(B)])
    cTw = torch.linalg.inv(wTc).cuda()
    g = torch.Generator().manual_seed(5)
    cam = torch.rand((B, 53, 3), generator=g) * torch.tensor([3.0, 2.0, 4.0]) + torch.tensor([-1.5, -1.0, -0.5])  # some behind, some outside
    pts = (cam @ wTc[:, :3, :3].transpose(1, 2) + wTc[:, None, :3, 3]).cuda()
    prior_pred = torch.sigmoid(syn.randn((B, 1, Hs, Ws), 8, "pp")).cuda()
    pcTw = torch.linalg.inv(torch.stack([syn.source_pose(b + 2).float() for b in range(B)])).cuda()
    from implicit_depth_amd import mlp
    from implicit_depth_amd._lib import IdhError

    with pytest.raises(IdhError, match="no forward"):
        model.query_points(pts, cTw, K0)
    _fwd(model, d, pyr, rendered_depth=rd)
    for pi in (None, {"prior_prediction": prior_pred, "prior_cam_T_world": pcTw}):
        q = model.query_points(pts, cTw, K0, prior_inputs=pi)
        assert q["point_pred"].shape == (B, 1, 53, 1) and q["point_valid"].dtype == torch.bool and q["point_valid"].shape == (B, 53)
        assert 0 < int(q["point_valid"].sum()) < B * 53
        rays, depth, valid, prior = mlp.project_points(pts, cTw, K0, Hs, Ws, *((prior_pred, pcTw, K0) if pi else ()))
        assert torch.equal(rays, q["point_rays"]) and torch.equal(depth, q["point_depth"]) and torch.equal(valid, q["point_valid"])
        out = _fwd(model, d, pyr, rendered_depth=rd, query_rays=rays, query_depths=depth.unsqueeze(-1), query_prior=None if prior is None else prior.unsqueeze(-1))
        assert torch.equal(out["ray_pred_0"], q["point_pred"])
        if pi:
            assert bool((prior == -1).any()) and bool((prior > 0).any())
    with pytest.raises(IdhError, match="batch size"):
        model.query_points(pts[:1], cTw[:1], K0[:1])


# ---- drop-in and streaming --------------------------------------------------------------------------------------------
IMG_H, IMG_W, D, BUFFER = 96, 128, 16, 4


class _RunOpts:
    matching_scale = 1
    min_matching_depth = 0.25
    max_matching_depth = 5.0

    def __init__(self, use_prior):
        self.use_prior = use_prior


def _model(volume, K, use_prior=False):
    """As tests/test_streaming_gpu.py."""
    from implicit_depth_amd import backbone
    from implicit_depth_amd import networks as net

    m = holder(K, volume, IMG_H // 4, IMG_W // 4, D, use_prior=use_prior, with_head=False)
    m.matching_model = net.ResnetMatchingEncoder(backbone.resnet18_stem(), 16)
    m.encoder = syn.StubImageEncoder()
    m.run_opts = _RunOpts(use_prior)
    m.thresholder = None
    syn.fill_state_dict(m, seed=30)
    return m.cuda().eval()


def _frame(t, poses, P=1):
    Hm, Wm = IMG_H // 4, IMG_W // 4
    K1, K0 = syn.intrinsics(Wm, Hm).float(), syn.intrinsics(IMG_W // 2, IMG_H // 2).float()
    w = poses[t].astype(np.float32)
    return to_cuda({
        "image_b3hw": syn.randn((1, 3, IMG_H, IMG_W), 500 + t, "stream_img"),
        "K_s1_b44": K1[None].clone(), "invK_s1_b44": torch.linalg.inv(K1)[None], "K_s0_b44": K0[None].clone(), "invK_s0_b44": torch.linalg.inv(K0)[None],
        "world_T_cam_b44": torch.from_numpy(w)[None], "cam_T_world_b44": torch.from_numpy(np.linalg.inv(w))[None],
        "rendered_depth": syn.rendered_depth_planes(1, IMG_H // 2, IMG_W // 2, P),
    })


def test_fused_forward_with_sampled_rays():
    from implicit_depth_amd.dropin import fused_forward, hot_path_of

    K, N, S = 2, 37, 3
    poses, _ = syn.keyframe_trajectory("stream12", seed=0)
    assert np.isfinite(poses[:3]).all()
    m = _model("dot", K)
    frames = [_frame(t, poses) for t in range(3)]
    keys = ("image_b3hw", "K_s1_b44", "invK_s1_b44", "world_T_cam_b44", "cam_T_world_b44")
    src = {k: torch.stack([frames[i][k][0] for i in (0, 1)])[None] for k in keys}
    fwd = fused_forward(m)
    plain = fwd("test", dict(frames[2]), src)
    assert not any(k.startswith("ray_pred") for k in plain)
    gh, gw = IMG_H, IMG_W  # depth_b1hw at twice the s0 map
    rays, depths = _rays_in(1, N, gh, gw, seed=21)
    cur = dict(frames[2], sampled_rays=rays.cuda(), sampled_depths=depths.cuda(), depth_b1hw=torch.ones(1, 1, gh, gw, device="cuda"))
    keep = cur["sampled_rays"].clone()
    out = fwd("test", cur, src)
    assert torch.equal(cur["sampled_rays"], keep)  # the reference normalises them in place; this path does not
    assert torch.equal(out["pred_0"], plain["pred_0"])
    for s in range(4):
        assert out[f"ray_pred_{s}"].shape == (1, 1, -(-N // (s + 1)), S)  # run_mlp_train's shapes (bd_model.py:352-353, :387)
    hot = hot_path_of(m)  # the same converted modules: a second HotPath computes the same bits
    E = src["cam_T_world_b44"] @ frames[2]["world_T_cam_b44"].unsqueeze(1)
    Pm = frames[2]["cam_T_world_b44"].unsqueeze(1) @ src["world_T_cam_b44"]
    with torch.inference_mode():
        stem = m.matching_model.net[:5]
        l1 = stem(torch.cat([frames[2]["image_b3hw"].unsqueeze(1), src["image_b3hw"]], 1).flatten(0, 1)).unflatten(0, (1, K + 1))
        o = hot(None, None, list(m.encoder(frames[2]["image_b3hw"])), E, Pm, src["K_s1_b44"], frames[2]["invK_s1_b44"], matching_layer1=l1,
                return_features=True, query_rays=keep, query_depths=cur["sampled_depths"], query_grid=(gh, gw), query_scales=(0, 1, 2, 3))
    w = R.weights64(m.binary_mlp)
    for s in range(4):
        assert torch.equal(o[f"ray_pred_{s}"], out[f"ray_pred_{s}"])
        ref, tol = Q.ray_bound(w, o[f"feature_s{s}_b1hw"].cpu(), rays, depths, None, (gh, gw), step=s + 1, scale=s)
        _hold(out[f"ray_pred_{s}"][:, 0], ref, tol, f"fused_forward ray_pred_{s}")
    from implicit_depth_amd._lib import IdhError

    with pytest.raises(IdhError):
        fwd("train", cur, src)


@pytest.mark.parametrize("use_prior", [False, True])
def test_streaming_point_queries(use_prior):
    """step(query_points=...) equals session.query_points(...) right after it, and on the following frames without a prediction the
    session still answers with the same bits (the last keyframe's features, pose and - with use_prior - carried prior)."""
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    session = StreamingSession(_model("mlp", 3, use_prior=use_prior), buffer_size=BUFFER)
    Hs, Ws = IMG_H // 2, IMG_W // 2
    g = torch.Generator().manual_seed(9)
    uvz = torch.rand((1, 45, 3), generator=g) * torch.tensor([Ws + 8.0, Hs + 8.0, 4.0]) + torch.tensor([-4.0, -4.0, 0.6])
    K0 = syn.intrinsics(Ws, Hs).float()
    cam = torch.stack([(uvz[..., 0] - K0[0, 2]) / K0[0, 0] * uvz[..., 2], (uvz[..., 1] - K0[1, 2]) / K0[1, 1] * uvz[..., 2], uvz[..., 2]], -1)
    with pytest.raises(IdhError, match="no prediction"):
        session.query_points(torch.zeros(1, 4, 3, device="cuda"))
    answered = between = 0
    last = pts = w_key = None
    for t in range(12):
        if not np.isfinite(poses[t]).all():
            break
        w = torch.from_numpy(poses[t].astype(np.float32))
        if last is None:  # points in front of THIS frame's camera, some outside its image
            pts = (cam @ w[:3, :3].t() + w[:3, 3]).cuda()
        out, code = session.step(_frame(t, poses), world_T_cam=poses[t], dist_to_last_valid=dists[t], query_points=pts)
        if out is not None and last is None:
            assert out["point_pred"].shape == (1, 1, 45, 1) and 0 < int(out["point_valid"].sum()) < 45
            assert bool(torch.isfinite(out["point_pred"]).all())
            q = session.query_points(pts)
            for k in ("point_pred", "point_valid", "point_depth", "point_rays"):
                assert torch.equal(q[k], out[k]), (t, k)
            if use_prior:  # the carried prior reaches the points
                assert session._prior is not None
            last, w_key = {k: v.clone() for k, v in q.items()}, w
            answered += 1
        elif out is None and last is not None:
            q = session.query_points(pts)
            for k, v in last.items():
                assert torch.equal(q[k], v), (t, k)
            q2 = session.query_points(cam.cuda(), world_T_cam=w_key)  # the same points, given in the keyframe camera's own frame
            assert (q2["point_depth"] - last["point_depth"]).abs().max().item() < 1e-4
            between += 1
            break
        elif out is not None:  # a newer keyframe answers from now on: start over from it
            last = None
            pts = (cam @ w[:3, :3].t() + w[:3, 3]).cuda()
            q = session.query_points(pts)
            last, w_key = {k: v.clone() for k, v in q.items()}, w
            answered += 1
    assert answered >= 1 and between == 1, (answered, between)
