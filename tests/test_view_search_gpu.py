"""Depth in a moving camera on the GPU: idh_binary_mlp_view_search_fwd called by hand on hostile buffers (tests/view_search_ref.py: case
table, fp64 simulation, device call), against the twelve-launch composition it replaces, the reference's own modules
(tests/golden/view_search.npz), and through mlp.view_depths / HotPath.query_view_depths / StreamingSession.depth_for_view / raycast_view.

The op is checked by teacher forcing over iters = 1 .. 12, as test_ray_search_gpu.py: (a) every last logit within view_query_ref.view_bound
of the fp64 chain at the kernel's own previous query (`fill`, exactly, at an invalid probe; the probes within PROJ_MARGIN of a
discontinuity - at most NEAR_CAP per step - left out), (b) every query, flag byte and threshold index bitwise the fp32 rule replayed on the
kernel's own logit and on the keyframe z that idh_binary_mlp_view_fwd returns for that probe."""
import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import view_search_ref as VS
from conftest import TOL, load_golden
from test_ray_query_gpu import _build, _frame, _fwd, _model, BUFFER, IMG_H, IMG_W

V, Q, R, S = VS.V, VS.Q, VS.R, VS.S
pytestmark = pytest.mark.gpu
_CACHE = {}


def _lib():
    from implicit_depth_amd import _lib as L

    return L.lib()


def _bits(t):
    t = torch.as_tensor(t)
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _hold(got, ref, tol, what):
    got, ref, tol = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu(), torch.as_tensor(tol).double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    ratio = (err / tol.clamp_min(1e-300)).max().item() if got.numel() else 0.0
    print(f"{what}: worst err/bound {ratio:.3g} (n = {got.numel()})")
    assert bool((err <= tol).all()), (what, ratio)


def _setup(case):
    """Inputs, network and device buffers of a case, built once and shared by the tests."""
    if case.name not in _CACHE:
        feat, rays, cams, prior = VS.case_inputs(case)
        m = VS.search_net(case)
        _CACHE[case.name] = (feat, rays, cams, prior, m, VS.Device(case, m, feat, rays, cams, prior))
    return _CACHE[case.name]


def _read(outs):
    vals = []
    for o in outs:
        if o is None:
            vals.append(None)
            continue
        v, clean = o.read()
        assert clean, "a store landed outside the output"
        vals.append(v)
    return vals


def _run(case, dev, iters=None, **kw):
    rc, *outs = VS.run_view_search(_lib(), case, dev, iters, **kw)
    assert rc == R.OK
    d, l, f, p = _read(outs)
    return d.view(case.shape), l.view(case.shape), None if f is None else f.view(case.shape), None if p is None else p.view(*case.shape, 3)


# ---- exact fp32 points on the host: what the probes of a ray LIST are (no depth map can express them) ----------------------------
def _round32(x64, inexact=None):
    """float64 -> float32.  Of an exact float64 value this is one rounding.  Of a sum that was itself rounded to float64 (``inexact``) it is
    the rounding of the exact value too, unless the float64 lies exactly half way between two float32 neighbours (asserted not to happen)."""
    r = x64.astype(np.float32)
    if inexact is not None and inexact.any():
        r64 = r.astype(np.float64)
        for side in (-np.inf, np.inf):
            n = np.nextafter(r, np.float32(side)).astype(np.float64)
            assert not (inexact & (x64 == (r64 + n) / 2)).any(), "a double rounding could differ from fmaf"
    return r


def _fma32(a, b, c):
    """fmaf(a, b, c) of fp32 operands: the product is exact in float64, the sum's rounding error is recovered by TwoSum."""
    p, c = np.asarray(a, np.float64) * np.asarray(b, np.float64), np.asarray(c, np.float64)
    s = p + c
    cc = s - p
    err = (p - (s - cc)) + (c - cc)
    return _round32(s, err != 0)


def _points32(rays, q, cams):
    """The world point of include/idh.h at depth q along the rays, in exactly rounded fp32: c_i, X_i = q c_i, p_i."""
    iK, T = cams[0].numpy(), cams[1].numpy()
    x, y = rays[..., 0].numpy(), rays[..., 1].numpy()
    X = []
    for i in range(3):
        c = _fma32(iK[:, i, 0, None], x, _fma32(iK[:, i, 1, None], y, np.broadcast_to(iK[:, i, 2, None], x.shape)))
        X.append(_round32(q.astype(np.float64) * c.astype(np.float64)))
    p = [_fma32(T[:, i, 0, None], X[0], _fma32(T[:, i, 1, None], X[1], _fma32(T[:, i, 2, None], X[2], np.broadcast_to(T[:, i, 3, None], x.shape))))
         for i in range(3)]
    return torch.from_numpy(np.stack(p, -1))


def _probe(case, feat, rays, cams, prior, m):
    """probe(q, n) of view_search_ref.compose: one step as the parent commit computes it."""
    if case.listed:
        return lambda q, n: VS.probe_by_points(_lib(), case, m, feat, cams, prior, _points32(rays, q, cams))
    return lambda q, n: VS.probe_by_view_fwd(_lib(), case, m, feat, cams, prior, q)


# ---- the op ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", VS.SMALL, ids=lambda c: c.name)
def test_search_by_teacher_forcing(case):
    feat, rays, cams, prior, m, dev = _setup(case)
    w = R.weights64(m)
    probe = _probe(case, feat, rays, cams, prior, m)
    shape = case.shape
    lo = np.full(shape, case.lo, dtype=np.float32)
    hi = np.full(shape, case.hi, dtype=np.float32)
    q = np.full(shape, R.first_query(case), dtype=np.float32)
    flags = np.zeros(shape, np.uint8)
    fill = np.float32(case.fill)
    worst, shares = 0.0, []
    for n in range(1, case.iters + 1):
        q_n, l_n, f_n, _ = _run(case, dev, n, want_points=False)
        q_n, l32, f_n = q_n.numpy(), l_n.numpy(), f_n.numpy()
        # (a) the logit at the kernel's own query q against the fp64 chain there
        ref, ch = VS.step64(case, w, feat, rays, cams, prior, q)
        ref_b, tol = V.view_bound(w, feat, ch, VS.prior_const(case))
        near, valid64 = ch["near"].numpy(), ch["valid"].numpy()
        shares.append(near.mean())
        assert near.mean() <= VS.NEAR_CAP, (case.name, n, near.mean())
        on, off = ~near & valid64, ~near & ~valid64
        assert (l32[off] == fill).all(), f"{case.name} step {n}: an invalid probe's logit is not fill"
        err = np.abs(l32.astype(np.float64) - ref_b.numpy())[on]
        bound = tol.numpy()[on]
        if on.any():
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), f"{case.name} step {n}: {int((err > bound).sum())} logits exceed the bound, worst err / bound {worst:.3g}"
        # (b) the rule replayed in fp32 on the kernel's own logit and the probe's keyframe z and validity as idh_binary_mlp_view_fwd gives them
        _, z, valid = probe(q, n - 1)
        assert (valid[~near] == valid64[~near]).all()
        thr, idx = R.thresholds_at(case, z)
        if case.table:
            _, idx64 = R.thresholds_at(case, ch["z"].float().numpy())
            edge = np.abs(ch["z"].numpy()[..., None] - np.asarray(case.table[0])).min(-1) < 1e-5
            assert (idx[~edge] == idx64[~edge]).all()  # the index is the bucket of the probe's KEYFRAME depth, not of the query
        lo, hi, q_v = R.search_step(case, lo, hi, q, l32, thr)
        bad = q_n.view(np.int32) != q_v.view(np.int32)
        assert not bad.any(), f"{case.name} step {n}: {int(bad.sum())} queries differ from the replay, first at {tuple(np.argwhere(bad)[0])}"
        flags |= (np.where(l32 < thr, 1, 2) | np.where(valid, 0, 4)).astype(np.uint8)
        assert (f_n == flags).all(), f"{case.name} step {n}: {int((f_n != flags).sum())} flags differ from the replay"
        assert (q_n >= np.float32(case.lo)).all() and (q_n <= np.float32(case.hi)).all()
        q = q_n.copy()
    print(f"{case.name}: worst err / bound over {case.iters} steps {worst:.4f}, largest share within the margin {max(shares):.4f}, "
          "flags " + " ".join(f"{v}:{(flags == v).mean():.2f}" for v in range(1, 8)))
    if case.camera == "behind":
        assert (flags == (5 if case.fill < 0 else 6)).all()
        assert (q == np.float32(VS.simulate(case, w, feat, rays, cams, prior)[0])).all()  # the bound the rule runs into


@pytest.mark.parametrize("case", VS.CASES, ids=lambda c: c.name)
def test_bit_identity_with_the_composition(case):
    """depth, last logit and flags equal `iters` single-probe launches of the parent commit's kernels with the fp32 rule between them:
    idh_binary_mlp_view_fwd on rendered = q_n (its view_pred with fill, view_depth for the threshold's bucket, view_valid for bit 2); for the
    ray list, whose rays no depth map expresses, idh_project_points_fwd + idh_binary_mlp_rays_fwd on the probes' exactly rounded world
    points - the bits idh_binary_mlp_view_fwd is documented to carry."""
    feat, rays, cams, prior, m, dev = _setup(case)
    depth, logit, flags, steps = VS.compose(case, _probe(case, feat, rays, cams, prior, m))
    d, l, f, _ = _run(case, dev, want_points=False)
    for what, got, want in (("depth", d, depth), ("last logit", l, logit), ("flags", f, flags)):
        diff = _bits(got) != _bits(torch.from_numpy(want))
        assert not diff.any(), f"{case.name}: {int(diff.sum())} {what} differ from the composition, first at {tuple(diff.nonzero()[0].tolist())}"
    valid = np.stack([s["valid"] for s in steps])
    print(f"{case.name}: {case.rays} rays equal in bits; {valid.mean():.3f} of the probes valid, "
          f"{(valid.any(0) & ~valid.all(0)).mean():.3f} of the rays with both kinds")
    # a second launch gives the same bits
    d2, l2, f2, _ = _run(case, dev, want_points=False)
    assert torch.equal(_bits(d), _bits(d2)) and torch.equal(_bits(l), _bits(l2)) and torch.equal(f, f2)


@pytest.mark.parametrize("case", [VS.CASES[1], VS.CROSSING, VS.CASES[5]], ids=lambda c: c.name)
def test_list_form_at_pixel_centres_is_the_grid_form(case):
    feat, rays, cams, prior, m, dev = _setup(case)
    grid = _run(case, dev)
    listed = _run(case, dev, listed=True)
    for a, b in zip(grid, listed):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("case", [VS.CASES[1], VS.CROSSING, VS.LISTED], ids=lambda c: c.name)
def test_points_and_optional_outputs(case):
    """World points within the derived bound of ray_search_ref.points_reference at the kernel's own depth - and bitwise the exactly rounded
    expression; optional outputs passed as NULL change nothing else, and every output's guard bytes survive (checked by every read)."""
    feat, rays, cams, prior, m, dev = _setup(case)
    d, l, f, p = _run(case, dev)
    ref, tol = VS.points_reference(rays, d, cams)
    _hold(p, ref, tol, f"{case.name} world points")
    assert torch.equal(_bits(p), _bits(_points32(rays, d.numpy(), cams)))
    back = torch.linalg.inv(cams[1].double())  # the live camera's z of the point is the depth: the query is the z-depth in the LIVE camera
    zc = (p.double() @ back[:, :3, :3].transpose(1, 2) + back[:, None, :3, 3])[..., 2]
    assert (zc - d.double()).abs().max().item() < 1e-4
    for kw in (dict(want_flags=False), dict(want_points=False), dict(want_flags=False, want_points=False)):
        d2, l2, f2, p2 = _run(case, dev, **kw)
        assert torch.equal(_bits(d2), _bits(d)) and torch.equal(_bits(l2), _bits(l))
        assert (f2 is None) == (not kw.get("want_flags", True)) and (p2 is None) == (not kw.get("want_points", True))
        assert f2 is None or torch.equal(f2, f)
        assert p2 is None or torch.equal(_bits(p2), _bits(p))


def test_search_reproduces_the_references_modules():
    """tests/golden/view_search.npz: depths equal where the reference's smallest per-step |logit - thr| exceeds the logit tolerance used
    for view_query.npz (scale-relative TOL), as hot_helpers.search_agrees for the dense search."""
    g = load_golden("view_search")
    case = VS.GOLDEN_CASE
    feat, cams = VS.golden_inputs()
    m = VS.golden_net()
    dev = VS.Device(case, m, feat, VS.pixel_centres(case.B, case.h, case.w), cams, None)
    d, _, f, _ = _run(case, dev, want_points=False)
    gold = torch.from_numpy(g["search_depths"]).view(case.shape)
    sure = torch.from_numpy(g["search_margin"]).view(case.shape) > TOL * float(g["logit_scale"])
    agree = d == gold
    print(f"golden: {agree.float().mean().item():.2%} of the depths equal, {sure.float().mean().item():.2%} with a margin above the tolerance")
    assert sure.float().mean().item() > 0.5 and bool(agree[sure].all())


# ---- through the layers ---------------------------------------------------------------------------------------------
def _thresholder():
    from implicit_depth_amd.metrics import Thresholder

    return Thresholder(torch.tensor([1.5 + 0.5 * i for i in range(8)]), torch.tensor([0.3, 0.35, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7]))


def _compose_public(query_view, B, size, th, iters=12, lo=0.5, hi=8.0):
    """What a caller had at the parent commit: twelve dense occlusion queries on rendered = q_n with the rule in torch between them.
    ``query_view(rendered)`` -> the dictionary of HotPath.query_view."""
    h, w = size
    lo_t, hi_t = torch.full((B, 1, h, w), lo, device="cuda"), torch.full((B, 1, h, w), hi, device="cuda")
    sd = (hi_t - lo_t) * 0.5
    flags = torch.zeros(B, 1, h, w, dtype=torch.uint8, device="cuda")
    if th is not None:
        bins = th.bins.cuda().float()
        tl = torch.log(th.thresholds.cuda().float() / (1 - th.thresholds.cuda().float()))
    for _ in range(iters):
        v = query_view(sd)
        logit, z = v["view_pred"], v["view_depth"]
        if th is not None:
            t = tl[(bins.view(1, 1, 1, 1, -1) < z.unsqueeze(-1)).sum(-1).clamp(max=bins.numel() - 1)]
        else:
            t = torch.zeros_like(sd)  # logit(0.5)
        vis = logit < t
        hi_t, lo_t = torch.where(vis, sd, hi_t), torch.where(vis, lo_t, sd)
        flags |= (torch.where(vis, 1, 2) | torch.where(v["view_valid"], 0, 4)).to(torch.uint8)
        sd = (hi_t + lo_t) * 0.5
    return sd, logit, flags


@pytest.mark.parametrize("thr", [False, True])
def test_query_view_depths_is_the_twelve_call_composition(thr):
    from implicit_depth_amd._lib import IdhError

    B, K, H, W, D = 2, 2, 16, 24, 16
    model, d, pyr, rd = _build(B, K, H, W, D, 1, use_prior=True)
    Hs, Ws, h, w = 2 * H, 2 * W, 15, 20
    iK, wTc, cTw, K0, pcTw, _ = (t.cuda() for t in V.cameras("moved", B, Hs, Ws, h, w))
    prior_pred = torch.sigmoid(syn.randn((B, 1, Hs, Ws), 8, "pp")).cuda()
    with pytest.raises(IdhError, match="no forward"):
        model.query_view_depths(iK, wTc, cTw, K0, size=(h, w))
    _fwd(model, d, pyr, rendered_depth=rd)
    th = _thresholder() if thr else None
    fill = -4.5
    for pi in (None, {"prior_prediction": prior_pred, "prior_cam_T_world": pcTw}):
        got = model.query_view_depths(iK, wTc, cTw, K0, size=(h, w), prior_inputs=pi, thresholder=th, fill=fill, return_points=True)
        assert set(got) == {"view_search_depths", "view_search_logits", "view_search_flags", "view_search_points"}
        sd, logit, flags = _compose_public(lambda r: model.query_view(r, iK, wTc, cTw, K0, prior_inputs=pi, fill=fill), B, (h, w), th)
        assert got["view_search_depths"].shape == (B, 1, h, w) and got["view_search_points"].shape == (B, 1, h, w, 3)
        assert torch.equal(got["view_search_depths"], sd) and torch.equal(got["view_search_logits"], logit) and torch.equal(got["view_search_flags"], flags)
        fl = got["view_search_flags"]
        assert bool((fl & 4).bool().any()) and bool(((fl & 4) == 0).any()) and bool(((fl & 3) == 3).any())
        # the list form: the pixel centres give the grid's bits; off-centre rays and rays outside the live image are legal
        centres = VS.pixel_centres(B, h, w).cuda()
        lst = model.query_view_depths(iK, wTc, cTw, K0, rays=centres, prior_inputs=pi, thresholder=th, fill=fill, return_points=True)
        assert lst["view_search_depths"].shape == (B, h * w) and lst["view_search_points"].shape == (B, h * w, 3)
        for k in got:
            assert torch.equal(lst[k].reshape(-1), got[k].reshape(-1)), k
        rays = (torch.rand((B, 45, 2), generator=torch.Generator().manual_seed(5)) * torch.tensor([w + 8.0, h + 8.0]) - 4.0).cuda()
        off = model.query_view_depths(iK, wTc, cTw, K0, rays=rays, prior_inputs=pi, thresholder=th, fill=fill, return_points=True)
        ref, tol = S.points_reference(rays.cpu(), off["view_search_depths"].cpu(), iK.cpu(), wTc.cpu())
        _hold(off["view_search_points"], ref, tol, "query_view_depths world points at off-centre rays")
        assert model.query_view_depths(iK, wTc, cTw, K0, rays=rays, prior_inputs=pi, thresholder=th, fill=fill)["view_search_points"] is None
    # fill = -inf / +inf: a probe outside the keyframe's view counts as visible / hidden
    for f_inf, bit in ((float("-inf"), 1), (float("inf"), 2)):
        g = model.query_view_depths(iK, wTc, cTw, K0, size=(h, w), fill=f_inf)
        never = (g["view_search_flags"] & 4).bool() & (g["view_search_logits"] == f_inf)
        assert bool(never.any()) and bool(torch.isfinite(g["view_search_depths"]).all())
        sd, logit, flags = _compose_public(lambda r: model.query_view(r, iK, wTc, cTw, K0, fill=f_inf), B, (h, w), None)
        assert torch.equal(g["view_search_depths"], sd) and torch.equal(g["view_search_flags"], flags)
    with pytest.raises(IdhError, match="batch size"):
        model.query_view_depths(iK[:1], wTc[:1], cTw[:1], K0[:1], size=(h, w))
    model.binary_mlp.mlp_math = "f16x3"
    with pytest.raises(IdhError, match="fp32 only"):
        model.query_view_depths(iK, wTc, cTw, K0, size=(h, w))


def _identity_agreement(w, feat, cams, depth_view, depth_ray, what):
    """The keyframe's own camera at the s0 size, no prior, threshold 0.5: up to the last bit, (u, v) reproduce the pixel centres and z the
    query, so the view search and the ray search at the pixel-centre rays follow the same path wherever, at every step of the fp64
    simulation, both paths' fp64 logits lie further from the threshold than their derived bounds, on the same side.  Those rays must
    agree bitwise; the share is reported, not asserted."""
    B, C, Hs, Ws = feat.shape
    case = VS.ViewSearchCase(C, B, Hs, Ws, Hs, Ws, "identity", None, "wide")
    rays = VS.pixel_centres(B, Hs, Ws)
    lo = np.full(case.shape, case.lo, dtype=np.float32)
    hi = np.full(case.shape, case.hi, dtype=np.float32)
    q = np.full(case.shape, R.first_query(case), dtype=np.float32)
    safe = np.ones(case.shape, bool)
    for _ in range(case.iters):
        ref_v, ch = VS.step64(case, w, feat, rays, cams, None, q)
        assert ch["valid"].all() and not ch["near"].any()
        _, tol_v = V.view_bound(w, feat, ch)
        ref_r, tol_r = Q.ray_bound(w, feat, rays, torch.from_numpy(q).unsqueeze(-1), None, (Hs, Ws))
        ref_r, tol_r = ref_r[..., 0], tol_r[..., 0]
        safe &= ((ref_v.abs() > tol_v) & (ref_r.abs() > tol_r) & ((ref_v < 0) == (ref_r < 0))).numpy()  # thr = logit(0.5) = 0
        lo, hi, q = R.search_step(case, lo, hi, q, ref_v.numpy(), np.zeros(case.shape))
    dv, dr = depth_view.reshape(case.shape).cpu(), depth_ray.reshape(case.shape).cpu()
    same = (dv == dr).numpy()
    print(f"{what}: the view search equals the ray search on {same.mean():.2%} of {same.size} rays; {safe.mean():.2%} are decided beyond "
          f"both bounds at every step, {same[safe].mean():.2%} of those agree")
    assert safe.any() and same[safe].all() and (dv.numpy()[safe] == q[safe]).all()


def test_identity_camera_agrees_with_query_ray_depths():
    B, K, H, W, D = 1, 2, 16, 24, 16
    model, d, pyr, rd = _build(B, K, H, W, D, 1)
    Hs, Ws = 2 * H, 2 * W
    cams = V.cameras("identity", B, Hs, Ws, Hs, Ws)
    iK, wTc, cTw, K0 = (t.cuda() for t in cams[:4])
    out = _fwd(model, d, pyr, rendered_depth=rd, return_features=True)
    v = model.query_view_depths(iK, wTc, cTw, K0, size=(Hs, Ws))
    r = model.query_ray_depths(VS.pixel_centres(B, Hs, Ws).cuda())
    assert not bool((v["view_search_flags"] & 4).any())
    _identity_agreement(R.weights64(model.binary_mlp), out["feature_s0_b1hw"].cpu(), cams, v["view_search_depths"], r["ray_depth"], "identity camera")


# ---- streaming --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_prior", [False, True])
def test_streaming_depth_for_view_and_raycast_view(use_prior):
    """On a frame where step() returned None the session answers in the LIVE camera with the bits of twelve occlusion_for_view calls and
    the rule between them (with use_prior: the carried prior, sampled per probe); raycast_view at the pixel centres is depth_for_view; at
    the keyframe's own pose and pixel centres it agrees with raycast under the identity camera's criterion."""
    from implicit_depth_amd import pipeline
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    session = StreamingSession(_model("mlp", 3, use_prior=use_prior), buffer_size=BUFFER)
    Hs, Ws, h, w = IMG_H // 2, IMG_W // 2, 30, 40
    invK = torch.linalg.inv(syn.intrinsics(w, h)).float()
    invK[:2, :3] *= 2.0  # a lens half as long as the keyframe's: the border of the live image looks past the keyframe's
    invK = invK.cuda()
    with pytest.raises(IdhError, match="no prediction"):
        session.depth_for_view(poses[0], invK, (h, w))
    with pytest.raises(IdhError, match="no prediction"):
        session.raycast_view(VS.pixel_centres(1, h, w).cuda(), poses[0], invK)
    key, done = None, False
    for t in range(12):
        if not np.isfinite(poses[t]).all():
            break
        frame = _frame(t, poses)
        out, code = session.step(frame, world_T_cam=poses[t], dist_to_last_valid=dists[t])
        if out is not None:
            key = frame
            continue
        if key is None:
            continue
        fill = -6.0
        got = session.depth_for_view(poses[t], invK, (h, w), fill=fill)
        sd, logit, flags = _compose_public(lambda r: session.occlusion_for_view(r, poses[t], invK, fill=fill), 1, (h, w), None)
        assert torch.equal(got["view_search_depths"], sd) and torch.equal(got["view_search_logits"], logit) and torch.equal(got["view_search_flags"], flags)
        assert got["view_search_points"].shape == (1, 1, h, w, 3) and bool(torch.isfinite(got["view_search_points"]).all())
        fl = got["view_search_flags"]
        print(f"frame {t}: flags " + " ".join(f"{v}:{(fl == v).float().mean().item():.2f}" for v in range(1, 8)))  # (the mix is the trajectory's: reported, not asserted)
        live = torch.from_numpy(poses[t].astype(np.float32))[None]
        ref, tol = S.points_reference(VS.pixel_centres(1, h, w), got["view_search_depths"].view(1, -1).cpu(), invK[None].cpu(), live)
        _hold(got["view_search_points"].view(1, -1, 3), ref, tol, f"depth_for_view world points (frame {t})")
        cast = session.raycast_view(VS.pixel_centres(1, h, w).cuda(), poses[t], invK, fill=fill)
        for k in got:
            assert torch.equal(cast[k].reshape(-1), got[k].reshape(-1)), k
        if use_prior:  # the prior path is taken: the constant -1 gives other logits (as test_view_query_gpu.py checks for occlusion_for_view)
            assert session._prior is not None
            const = session.hot.query_view_depths(invK[None], live.cuda(), key["cam_T_world_b44"], key["K_s0_b44"], size=(h, w), fill=fill)
            assert not torch.equal(const["view_search_logits"], got["view_search_logits"])
        else:  # the keyframe's own camera: the hit test from the live screen is the keyframe's hit test
            centres = VS.pixel_centres(1, Hs, Ws).cuda()
            own = session.raycast_view(centres, key["world_T_cam_b44"][0], key["invK_s0_b44"])
            ray = session.raycast(centres)
            feat = pipeline._export(session.hot._last["final"][0]).cpu()
            cams = tuple(key[k].cpu() for k in ("invK_s0_b44", "world_T_cam_b44", "cam_T_world_b44", "K_s0_b44")) * 2
            _identity_agreement(R.weights64(session.hot.binary_mlp), feat, cams[:6], own["view_search_depths"], ray["ray_depth"], f"raycast_view vs raycast (frame {t})")
        done = True
        break
    assert done, "the sequence has no frame between keyframes after the first prediction"
