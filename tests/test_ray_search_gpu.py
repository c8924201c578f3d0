"""Depth and hit points at sparse rays on the GPU: idh_binary_mlp_rays_search_fwd called by hand on hostile buffers (tests/ray_search_ref.py:
case table, fp64 simulation, the hit points' derived bound), then the same kernel through mlp.ray_depths / HotPath.query_ray_depths /
StreamingSession.raycast at the smallest model shapes of test_ray_query_gpu.py.

The op is checked by teacher forcing over iters = 1 .. 12, as test_mlp_op_gpu.py::test_search_by_teacher_forcing: (a) every last logit
within ray_query_ref.ray_bound of the fp64 MLP at the kernel's own previous query, (b) every query bitwise the fp32 rule replayed on the
kernel's own logit, (c) the flags the OR of the replayed decisions, (d) every depth inside [lo, hi], (e) every last logit bitwise that of
idh_binary_mlp_rays_fwd at S = 1 with the depth set to that previous query.  No ray is excluded."""
import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import mlp_op_ref as R
import ray_query_ref as Q
import ray_search_ref as S
from conftest import TOL, load_golden, rel_err
from hot_helpers import holder, rel_poses, search_agrees, to_cuda

pytestmark = pytest.mark.gpu


def _lib():
    from implicit_depth_amd import _lib as L

    return L.lib()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _twice(run):
    """Run twice into fresh outputs: both IDH_OK, guard words untouched, results bitwise equal.  Returns the first run's outputs (CPU)."""
    res = []
    for _ in range(2):
        rc, *outs = run()
        assert rc == R.OK
        vals = []
        for o in outs:
            if o is None:
                vals.append(None)
                continue
            v, clean = o.read()
            assert clean, "a store landed outside the output"
            vals.append(v)
        res.append(vals)
    for a, b in zip(*res):
        assert (a is None and b is None) or torch.equal(_bits(a), _bits(b)), "two launches of the same call differ in bits"
    return res[0]


def _other_query(lo, hi, q, logit, thr):
    """The query the opposite decision leads to."""
    vis = ~(logit < thr)
    hi2 = np.where(vis, q, hi).astype(np.float32)
    lo2 = np.where(vis, lo, q).astype(np.float32)
    return ((hi2 + lo2) * np.float32(0.5)).astype(np.float32)


def _hold(got, ref, tol, what):
    """|got - ref| <= tol elementwise; prints the worst err / bound."""
    got, ref, tol = got.double().cpu(), ref.double().cpu(), tol.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    ratio = (err / tol.clamp_min(1e-300)).max().item()
    print(f"{what}: worst err/bound {ratio:.3g} (max err {err.max().item():.3g}, n = {got.numel()})")
    assert bool((err <= tol).all()), (what, ratio)
    return ratio


# ---- the op ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_search_by_teacher_forcing(case):
    L = _lib()
    feat, rays, prior = S.case_inputs(case)
    m = S.search_net(case)
    dev = S.Device(case, m, feat, rays, prior)
    B, N = case.B, case.N
    shape = (B, N)
    prior3 = prior.unsqueeze(-1) if prior is not None else None
    lo = np.full(shape, case.lo, dtype=np.float32)
    hi = np.full(shape, case.hi, dtype=np.float32)
    q = np.full(shape, R.first_query(case), dtype=np.float32)
    flags = np.zeros(shape, np.uint8)
    skipped = np.zeros(shape, bool)
    may_skip = case.table is None and case.thr != 0.5  # the host's logf may differ from numpy's by an ulp; logit(0.5) is exactly 0
    asked, answered = [], []
    for n in range(1, S.ITERS + 1):
        q_n, l_n, f_n, _ = _twice(lambda: S.run_search(L, case, dev, n))
        q_n, l_n, f_n = q_n.view(shape).numpy(), l_n.view(shape), f_n.view(shape).numpy()
        asked.append(q.copy())
        answered.append(l_n.clone())
        # (e) the same evaluation through idh_binary_mlp_rays_fwd, S = 1, at the kernel's own previous query: the same bits
        rc, one = Q.run_rays(L, case, m, feat, rays, torch.from_numpy(q).view(B, N, 1), prior3)
        assert rc == R.OK
        l_rays = one.read()[0].view(shape)
        diff = _bits(l_rays) != _bits(l_n)
        assert not diff.any(), f"{case.name} step {n}: {int(diff.sum())} logits differ in bits from idh_binary_mlp_rays_fwd, first at {tuple(diff.nonzero()[0].tolist())}"
        # (b) the next query: the fp32 rule replayed on the kernel's own logit
        thr, _ = R.thresholds_at(case, q)
        l32 = l_n.numpy()
        lo_v, hi_v, q_v = R.search_step(case, lo, hi, q, l32, thr)
        if may_skip:
            knife = np.abs(l32 - thr) <= 2 * np.spacing(np.abs(thr))
            took_other = knife & (q_n.view(np.int32) != q_v.view(np.int32))
            skipped |= took_other
        else:
            took_other = np.zeros(shape, bool)
        expect = np.where(took_other, _other_query(lo, hi, q, l32, thr), q_v).astype(np.float32)
        bad = q_n.view(np.int32) != expect.view(np.int32)
        assert not bad.any(), f"{case.name} step {n}: {int(bad.sum())} queries differ from the replay, first at {tuple(np.argwhere(bad)[0])}"
        vis = (l32 < thr) ^ took_other
        # (c) the flags: the OR of the replayed decisions up to n
        flags |= np.where(vis, 1, 2).astype(np.uint8)
        assert (f_n == flags).all(), f"{case.name} step {n}: {int((f_n != flags).sum())} flags differ from the replay"
        # (d)
        assert (q_n >= np.float32(case.lo)).all() and (q_n <= np.float32(case.hi)).all()
        hi = np.where(vis, q, hi).astype(np.float32)
        lo = np.where(vis, lo, q).astype(np.float32)
        q = q_n.copy()
    assert np.isfinite(q).all()  # non-finite rays included: f = 0, a finite depth
    if B * N > 1:
        assert (flags & 1).any() and (flags & 2).any()
    assert skipped.mean() <= 1e-3, skipped.mean()
    # (a) all twelve evaluations against the fp64 MLP at the queries the kernel asked, within the derived bound; in runs of rays
    w = R.weights64(m)
    d_all, l_all = torch.from_numpy(np.stack(asked, -1)), torch.stack(answered, -1)  # B, N, 12
    fin = S.finite_rays(rays)
    worst, run = 0.0, 1024
    for j in range(0, N, run):
        sl = slice(j, min(N, j + run))
        ref, tol = Q.ray_bound(w, feat, fin[:, sl], d_all[:, sl], prior3[:, sl] if prior3 is not None else case.prior, case.grid)
        err = (l_all[:, sl].double() - ref).abs()
        ok = err <= tol
        worst = max(worst, (err / tol).nan_to_num(nan=float("inf")).max().item())
        assert ok.all(), f"{case.name}: {int((~ok).sum())} logits exceed the bound, worst err / bound {worst:.3g}, first (b, ray, step) {tuple((~ok).nonzero()[0].tolist())}"
    share = {v: float((flags == v).mean()) for v in (1, 2, 3)}
    print(f"{case.name}: worst err / bound over {S.ITERS} steps {worst:.4f}, skipped {int(skipped.sum())} rays, "
          f"flags 1 / 2 / 3 = {share[1]:.1%} / {share[2]:.1%} / {share[3]:.1%}")


@pytest.mark.parametrize("case", [S.CASES[1], S.CASES[5]], ids=lambda c: c.name)
def test_hit_points_within_the_derived_bound(case):
    """World- and camera-space points against the fp64 restatement of include/idh.h's expression at the kernel's own depth; the optional
    outputs left out change nothing else."""
    L = _lib()
    feat, rays, prior = S.case_inputs(case)
    dev = S.Device(case, S.search_net(case), feat, rays, prior)
    iK, wTc = S.camera_matrices(case)
    iKd, wTcd = iK.cuda().contiguous(), wTc.cuda().contiguous()
    B, N = case.B, case.N
    d_w, l_w, f_w, p_w = _twice(lambda: S.run_search(L, case, dev, S.ITERS, iKd, wTcd))
    d_c, l_c, f_c, p_c = _twice(lambda: S.run_search(L, case, dev, S.ITERS, iKd, None))
    d_0, l_0, f_0, p_0 = _twice(lambda: S.run_search(L, case, dev, S.ITERS, None, None, want_flags=False))
    assert f_0 is None and p_0 is None
    for a, b in ((d_w, d_c), (d_w, d_0), (l_w, l_c), (l_w, l_0)):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(f_w, f_c)
    depth = d_w.view(B, N)
    ref, tol = S.points_reference(rays, depth, iK, wTc)
    _hold(p_w.view(B, N, 3), ref, tol, f"{case.name} world points")
    ref, tol = S.points_reference(rays, depth, iK)
    _hold(p_c.view(B, N, 3), ref, tol, f"{case.name} camera points")
    # the expression is not vacuous: the camera-space z is the depth itself up to the bound (invK's third row is (0, 0, 1, 0))
    assert (p_c.view(B, N, 3)[..., 2] - depth).abs().max().item() <= 4 * R.U * depth.abs().max().item()
    assert (p_w.view(B, N, 3) - p_c.view(B, N, 3)).abs().max().item() > 0.1  # and the pose is applied


# ---- through the layers ---------------------------------------------------------------------------------------------
def _thresholder():
    from implicit_depth_amd.metrics import Thresholder

    return Thresholder(torch.tensor([1.5 + 0.5 * i for i in range(8)]), torch.tensor([0.3, 0.35, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7]))


def _pixel_centres(H, W):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32) + 0.5, torch.arange(W, dtype=torch.float32) + 0.5, indexing="ij")
    return torch.stack([xs, ys], -1).view(1, H * W, 2)


@pytest.mark.parametrize("thr", [False, True])
def test_pixel_centre_rays_match_the_reference_search(thr):
    """BDModel.forward(infer_depth=True) of the reference (golden g5_bdmodel_mlp, as test_hot_path_head_gpu.py): query_ray_depths at all
    48 x 64 pixel-centre rays under the project's rule and tolerance for the dense search."""
    from implicit_depth_amd.dropin import hot_path_of

    g = load_golden("g5_bdmodel_mlp")
    K = int(g["K"])
    h = holder(K, "mlp", 24, 32, 16).cuda()
    cur, src = (to_cuda(d) for d in syn.frame_tuple(1, K, 96, 128, seed=31, P=3))
    E, P = rel_poses(cur, src)
    hot = hot_path_of(h)
    hot.thresholder = _thresholder() if thr else None
    t = lambda name: torch.as_tensor(g[name]).cuda()
    out = hot(t("matching_cur"), t("matching_src"), [t(f"enc{i}") for i in range(5)], E, P, src["K_s1_b44"], cur["invK_s1_b44"],
              rendered_depth=cur["rendered_depth"], infer_depth=True)
    q = hot.query_ray_depths(_pixel_centres(48, 64).cuda())
    assert q["ray_points"] is None and q["ray_hit"].dtype == torch.uint8 and tuple(q["ray_depth"].shape) == (1, 48 * 64)
    tag = "_thr" if thr else ""
    sd, pred = q["ray_depth"].view(1, 1, 48, 64), q["ray_pred"].view(1, 1, 48, 64)
    dense_agree = search_agrees(out["search_depths"], g["search_depths" + tag], g["search_margin" + tag])
    agree = search_agrees(sd, g["search_depths" + tag], g["search_margin" + tag])
    err = rel_err(pred.cpu()[agree], torch.as_tensor(g["search_pred" + tag])[agree])
    same = (sd == out["search_depths"]).float().mean().item()
    print(f"thr={thr}: rays agree with the reference on {agree.float().mean().item():.2%} of the pixels (dense search {dense_agree.float().mean().item():.2%}), "
          f"logit rel err {err:.3g}, depth equal to the dense search's on {same:.2%}")
    assert err < TOL
    hit = q["ray_hit"].view(48, 64).cpu()
    assert set(hit.unique().tolist()) <= {1, 2, 3}


def _build(B, K, H, W, D, use_prior=False, seed=0):
    """As tests/test_ray_query_gpu.py: the small BD model on synthetic inputs (s0 map 2H x 2W)."""
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
    return HotPath(CostVolumeManager(H, W, D), cve, dec, mlp).cuda(), {k: v.cuda() for k, v in inp.items()}, [t.cuda() for t in pyr]


def _fwd(model, d, pyr, **kw):
    return model(d["cur_feats"], d["src_feats"], pyr, d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"], **kw)


def _rays_in(B, N, gh, gw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((B, N, 2), generator=g) * torch.tensor([gw + 3.0, gh + 3.0]) - 1.5  # up to 1.5 px outside on every side


@pytest.mark.parametrize("thr", [False, True])
def test_query_ray_depths_is_the_twelve_step_composition(thr):
    """What a caller had before: twelve query_rays(S = 1) calls with the fp32 rule between them.  The same bits."""
    from implicit_depth_amd._lib import IdhError

    B, K, H, W, D = 2, 2, 16, 24, 16
    model, d, pyr = _build(B, K, H, W, D, use_prior=True)
    grid = (4 * H, 4 * W)  # the rays live on a grid twice the s0 map
    rays = _rays_in(B, 53, *grid, seed=13).cuda()
    with pytest.raises(IdhError, match="no forward"):
        model.query_ray_depths(rays, grid=grid)
    _fwd(model, d, pyr)
    th = _thresholder() if thr else None
    keep = rays.clone()
    q = model.query_ray_depths(rays, grid=grid, thresholder=th)
    assert torch.equal(rays, keep)
    N = rays.shape[1]
    lo, hi = torch.full((B, N), 0.5, device="cuda"), torch.full((B, N), 8.0, device="cuda")
    sd = (hi - lo) * 0.5
    flags = torch.zeros(B, N, dtype=torch.uint8, device="cuda")
    if thr:
        bins = th.bins.cuda().float()
        tl = torch.log(th.thresholds.cuda().float() / (1 - th.thresholds.cuda().float()))
    for _ in range(12):
        logit = model.query_rays(rays, sd.unsqueeze(-1), grid=grid)["ray_pred_0"][:, 0, :, 0]
        if thr:
            idx = (bins.view(1, 1, -1) < sd.unsqueeze(-1)).sum(-1).clamp(max=bins.numel() - 1)
            t = tl[idx]
        else:
            t = torch.zeros_like(sd)  # logit(0.5)
        vis = logit < t
        hi, lo = torch.where(vis, sd, hi), torch.where(vis, lo, sd)
        flags |= torch.where(vis, 1, 2).to(torch.uint8)
        sd = (hi + lo) * 0.5
    assert torch.equal(q["ray_depth"], sd) and torch.equal(q["ray_pred"], logit) and torch.equal(q["ray_hit"], flags)
    assert model.query_ray_depths(rays, grid=grid, thresholder=th, prior=-1.0)["ray_depth"].equal(q["ray_depth"])  # None is the constant -1
    model.binary_mlp.mlp_math = "f16x3"
    with pytest.raises(IdhError, match="fp32 only"):
        model.query_ray_depths(rays, grid=grid)


def _exact_cameras(B, Hs, Ws):
    """Cameras whose inverses are exact in fp32, so that back-projection followed by projection is the identity in exact arithmetic:
    a power-of-two pinhole, and poses made of a signed axis permutation and a dyadic translation."""
    K = R._pinhole(32.0, 32.0, Ws / 2, Hs / 2)
    rots = [torch.tensor([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]), torch.tensor([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])]
    wTc = []
    for b in range(B):
        T = torch.eye(4, dtype=torch.float64)
        T[:3, :3] = rots[b % 2].double()
        T[:3, 3] = torch.tensor([0.5 + b, -0.25, 1.0 + 0.5 * b], dtype=torch.float64)
        wTc.append(T)
    wTc = torch.stack(wTc)
    cTw = wTc.clone()  # [R | t]^-1 = [R^T | -R^T t]: exact for a permutation and dyadic t
    cTw[:, :3, :3] = wTc[:, :3, :3].transpose(1, 2)
    cTw[:, :3, 3] = -(wTc[:, :3, :3].transpose(1, 2) @ wTc[:, :3, 3:])[..., 0]
    iK = torch.eye(4, dtype=torch.float64)
    iK[0, 0], iK[1, 1], iK[0, 2], iK[1, 2] = 1 / 32.0, 1 / 32.0, -Ws / 64.0, -Hs / 64.0
    mats = torch.stack([K] * B), torch.stack([iK] * B), wTc, cTw
    for m in mats:
        assert torch.equal(m.float().double(), m)
    assert torch.equal(mats[0] @ mats[1], torch.eye(4, dtype=torch.float64).expand(B, 4, 4)) and torch.equal(mats[2] @ mats[3], mats[0] @ mats[1])
    return tuple(m.float() for m in mats)


def test_hit_points_project_back_onto_their_rays():
    """ray_points through mlp.project_points land on the input rays at the returned depths.  With cameras whose inverses are exact, the
    composition is the identity in exact arithmetic, so two derived bounds cover the difference: the projection's own at the kernel's points
    (ray_query_ref.projection_reference), and the points' own (ray_search_ref.points_reference) carried through P = K cam_T_world."""
    from implicit_depth_amd import mlp

    B, K, H, W, D = 2, 2, 16, 24, 16
    model, d, pyr = _build(B, K, H, W, D)
    Hs, Ws = 2 * H, 2 * W
    K0, iK0, wTc, cTw = _exact_cameras(B, Hs, Ws)
    rays = _rays_in(B, 53, Hs, Ws, seed=17)
    _fwd(model, d, pyr)
    q = model.query_ray_depths(rays.cuda(), invK_s0_b44=iK0.cuda(), world_T_cam_b44=wTc.cuda())
    pts, depth = q["ray_points"], q["ray_depth"].cpu()
    assert tuple(pts.shape) == (B, 53, 3)
    ref_p, e_p = S.points_reference(rays, depth, iK0, wTc)
    _hold(pts, ref_p, e_p, "query_ray_depths world points")
    back_rays, back_depth, valid, _ = mlp.project_points(pts, cTw.cuda(), K0.cuda(), Hs, Ws)
    proj = Q.projection_reference(pts.cpu(), cTw, K0, Hs, Ws)  # fp64 projection of the kernel's fp32 points, with the projection's bound
    _hold(back_rays, proj["rays"], proj["e_rays"], "project_points rays at the hit points")
    _hold(back_depth, proj["depth"], proj["e_depth"], "project_points depth at the hit points")
    # the points' own error through P: e_c = |P| e_p, then u = c_x / z
    Pm = (K0.double() @ cTw.double())[:, :3, :3]
    e_c = e_p @ Pm.abs().transpose(1, 2)
    z = proj["depth"]
    e_u = (e_c[..., :2] + proj["rays"].abs() * e_c[..., 2:]) / (z - e_c[..., 2]).unsqueeze(-1)
    _hold(proj["rays"], rays.double(), e_u, "exact projection of the hit points vs the input rays")
    _hold(proj["depth"], depth.double(), e_c[..., 2], "exact depth of the hit points vs ray_depth")
    assert 0 < int(valid.sum()) < valid.numel()  # rays inside and outside the image
    # camera-space points when no pose is given
    qc = model.query_ray_depths(rays.cuda(), invK_s0_b44=iK0.cuda())
    ref_c, e_cam = S.points_reference(rays, depth, iK0)
    _hold(qc["ray_points"], ref_c, e_cam, "query_ray_depths camera points")
    assert torch.equal(qc["ray_depth"], q["ray_depth"])


# ---- streaming --------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("use_prior", [False, True])
def test_streaming_raycast(use_prior):
    """raycast raises before the first prediction, answers on a frame where step returned None, and equals HotPath.query_ray_depths with the
    keyframe's invK_s0 and world_T_cam (with use_prior: the constant -1 in the prior channel)."""
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    session = StreamingSession(_model("mlp", 3, use_prior=use_prior), buffer_size=BUFFER)
    Hs, Ws = IMG_H // 2, IMG_W // 2
    rays = _rays_in(1, 45, Hs, Ws, seed=19).cuda()
    with pytest.raises(IdhError, match="no prediction"):
        session.raycast(rays)
    key = None
    between = 0
    for t in range(12):
        if not np.isfinite(poses[t]).all():
            break
        frame = _frame(t, poses)
        out, code = session.step(frame, world_T_cam=poses[t], dist_to_last_valid=dists[t])
        if out is not None:
            key = frame
        elif key is not None:  # a frame without a prediction: the keyframe's features and camera answer
            r = session.raycast(rays)
            want = session.hot.query_ray_depths(rays, invK_s0_b44=key["invK_s0_b44"], world_T_cam_b44=key["world_T_cam_b44"],
                                                prior=-1.0 if use_prior else None)
            assert set(r) == {"ray_depth", "ray_pred", "ray_hit", "ray_points"}
            for k in r:
                assert torch.equal(r[k], want[k]), (t, k)
            assert tuple(r["ray_points"].shape) == (1, 45, 3) and bool(torch.isfinite(r["ray_points"]).all())
            ref, tol = S.points_reference(rays.cpu(), r["ray_depth"].cpu(), key["invK_s0_b44"].cpu(), key["world_T_cam_b44"].cpu())
            _hold(r["ray_points"], ref, tol, f"raycast world points (frame {t})")
            between += 1
            break
    assert between == 1
