"""Occlusion and depth in a moving camera against several remembered keyframes on the GPU: idh_binary_mlp_view_keys_fwd and
idh_binary_mlp_view_keys_search_fwd called by hand on a hostile ring (tests/view_keys_ref.py: case table, fp64 first-valid reference,
device calls), against the compositions they replace - M launches of idh_binary_mlp_view_fwd and a per-pixel select; for the search the
twelve-step host loop over that - and through mlp / PredictionRing / HotPath.remember / query_view_keys / query_view_depths_keys /
StreamingSession(query_keyframes=3)."""
import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import view_keys_ref as VK
from test_ray_query_gpu import _build, _frame, _fwd, _model, BUFFER
from test_view_search_gpu import _bits, _compose_public, _points32, _thresholder

V, VS, Q, R, S = VK.V, VK.VS, VK.Q, VK.R, VK.S
pytestmark = pytest.mark.gpu
_CACHE = {}


def _lib():
    from implicit_depth_amd import _lib as L

    return L.lib()


def _setup(case):
    """Inputs, network and device buffers of a case, built once and shared by the tests."""
    if case.name not in _CACHE:
        feats, third, cams, prior = VK.case_inputs(case)
        m = VK.search_net(case) if isinstance(case, VK.KeysSearchCase) else R.make_net(case.cf, case.has_prior, R._seed(case.name))
        _CACHE[case.name] = (feats, third, cams, prior, m, VK.Device(case, m, feats, third, cams, prior))
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


def _run(case, dev, **kw):
    """(logits, key, depth, points) of one dense launch as CPU tensors (B,N) / (B,N,3); guard bytes checked."""
    rc, *outs = VK.run_keys(_lib(), case, dev, **kw)
    assert rc == VK.OK
    l, k, d, p = _read(outs)
    B = case.B
    return l.view(B, -1), None if k is None else k.view(B, -1), None if d is None else d.view(B, -1), None if p is None else p.view(B, -1, 3)


def _run_search(case, dev, **kw):
    rc, *outs = VK.run_keys_search(_lib(), case, dev, **kw)
    assert rc == VK.OK
    d, l, f, p, k = _read(outs)
    sh = case.shape
    return d.view(sh), l.view(sh), None if f is None else f.view(sh), None if p is None else p.view(*sh, 3), None if k is None else k.view(sh)


def _same(got, want, what):
    diff = _bits(got) != _bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.numel()} differ in bits, first at {tuple(diff.nonzero()[0].tolist())}"


# ---- 1. the dense form is the composition, bit for bit --------------------------------------------------------------------------
def _composition(case, feats, rd, cams, prior, m):
    """M launches of idh_binary_mlp_view_fwd, one per key in key_slots order on that key's own map, and the torch first-valid select."""
    B = case.B
    per_key = [VK.run_single(_lib(), case, m, feats, rd, cams, prior, s) for s in case.slots]
    logit, key, depth = VK.first_valid([r[0].view(B, -1) for r in per_key], [r[1].view(B, -1) for r in per_key], [r[2].view(B, -1) for r in per_key],
                                       float(np.float32(case.fill)))
    for r in per_key[1:]:
        assert torch.equal(_bits(r[3]), _bits(per_key[0][3]))  # the world point does not depend on the key
    return logit, key, depth, per_key[0][3].view(B, -1, 3), per_key


@pytest.mark.parametrize("case", VK.CASES, ids=lambda c: c.name)
def test_dense_bit_identity_with_the_composition(case):
    feats, rd, cams, prior, m, dev = _setup(case)
    logit, key, depth, points, per_key = _composition(case, feats, rd, cams, prior, m)
    l, k, d, p = _run(case, dev)
    _same(l, logit, f"{case.name} logits")
    assert torch.equal(k, key), f"{case.name}: {int((k != key).sum())} key indices differ"
    _same(d, depth, f"{case.name} view_depth")
    _same(p, points, f"{case.name} view_points")
    shares = [(k == i).float().mean().item() for i in range(case.M)] + [(k == VK.NONE).float().mean().item()]
    print(f"{case.name}: {case.rays} pixels equal in bits; key shares " + " ".join(f"{s:.3f}" for s in shares[:-1]) + f", none {shares[-1]:.3f}")
    if case.M == 1:  # all four outputs are idh_binary_mlp_view_fwd's
        gl, gv, gz, gp = per_key[0]
        _same(l.view(-1), gl, "M = 1 logits")
        _same(d.view(-1), gz, "M = 1 view_depth")
        _same(p.view(-1), gp, "M = 1 view_points")
        assert torch.equal(k.view(-1) == 0, gv == 1) and torch.equal(k.view(-1) == VK.NONE, gv == 0)
    if case.pose == "behind":
        assert bool((k == VK.NONE).all()) and bool((l == np.float32(case.fill)).all())
    l2, k2, d2, p2 = _run(case, dev)  # a second launch gives the same bits
    assert torch.equal(_bits(l), _bits(l2)) and torch.equal(k, k2) and torch.equal(_bits(d), _bits(d2)) and torch.equal(_bits(p), _bits(p2))


# ---- 2. derived bounds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", VK.CASES, ids=lambda c: c.name)
def test_dense_within_the_derived_bound(case):
    """Kept pixels (outside the margin of every boundary up to the selected key): the key is the fp64 chain's, the logit lies within
    view_query_ref.view_bound of the fp64 chain for that key, `fill` is exact where no key is valid or d is bad, view_depth within the
    chain's bound.  Guard bytes around every output survive (every read checks them); NULL optional outputs change nothing."""
    feats, rd, cams, prior, m, dev = _setup(case)
    w = R.weights64(m)
    ref, sel, near, ch, chains = VK.reference(case, w, feats, rd, cams, prior)
    l, k, d, p = _run(case, dev)
    keep = ~near
    assert near.float().mean().item() <= VK.NEAR_CAP
    assert torch.equal(k.long()[keep], sel[keep]), "a kept pixel selected another key than the fp64 chain"
    none = keep & (sel == VK.NONE)
    assert bool((l[none] == np.float32(case.fill)).all())
    assert bool((l[~ch["dok"]] == np.float32(case.fill)).all()) and bool((d[~ch["dok"]] == 0).all()) and bool((p[~ch["dok"]] == 0).all())
    on = keep & (sel != VK.NONE)
    ref_b, tol = VK.bound(case, w, feats, chains, sel)
    if on.any():
        err = (l.double() - ref_b).abs()[on]
        ratio = (err / tol[on]).max().item()
        print(f"{case.name}: worst err / bound {ratio:.3g} over {int(on.sum())} pixels, {near.float().mean().item():.4f} left out")
        assert bool(torch.isfinite(l[on]).all()) and ratio <= 1.0, (case.name, ratio)
        assert torch.allclose(ref_b[on], ref.view(case.B, -1)[on], rtol=1e-9, atol=1e-9)
    zk = keep & ch["dok"]
    assert bool(((d.double() - ch["z"]).abs()[zk] <= ch["e_z"][zk]).all())
    assert bool(((p.double() - ch["points"]).abs()[ch["dok"]] <= ch["e_points"][ch["dok"]]).all())
    for outputs in ((False, True, True), (True, False, False), (False, False, False)):
        l2, k2, d2, p2 = _run(case, dev, outputs=outputs)
        assert torch.equal(_bits(l2), _bits(l))
        assert [x is None for x in (k2, d2, p2)] == [not o for o in outputs]
        assert (k2 is None or torch.equal(k2, k)) and (d2 is None or torch.equal(_bits(d2), _bits(d))) and (p2 is None or torch.equal(_bits(p2), _bits(p)))


# ---- 3. the search ------------------------------------------------------------------------------------------------------------
def _probe(case, feats, rays, cams, prior, m, dev, keys):
    """probe(q, n) of view_search_ref.compose: one step as a caller composes it.  Grid form: idh_binary_mlp_view_keys_fwd on rendered = q.
    Ray list, whose rays no depth map expresses: idh_project_points_fwd + idh_binary_mlp_rays_fwd per key on the probes' exactly rounded
    world points - the bits idh_binary_mlp_view_fwd is documented to carry - and the first-valid select.  ``keys`` collects the key per step."""
    B, N = case.shape
    if not case.listed:
        def grid(q, n):
            rd = torch.as_tensor(q).view(B, 1, case.h, case.w).cuda()
            l, k, d, _ = _run(case, dev, rendered=rd, outputs=(True, True, False))
            keys.append(k.numpy().copy())
            return l.numpy(), d.numpy(), (k != VK.NONE).numpy()
        return grid

    def listed(q, n):
        pts = _points32(rays, q, cams)
        per = [VS.probe_by_points(_lib(), VK._Block(case), m, feats[s], VK.key_cams(cams, s), None if prior is None else prior[s], pts) for s in case.slots]
        l, k, z = VK.first_valid([torch.from_numpy(x[0]) for x in per], [torch.from_numpy(x[2]) for x in per], [torch.from_numpy(x[1]) for x in per],
                                 float(np.float32(case.fill)))
        keys.append(k.numpy().copy())
        return l.numpy(), z.numpy(), (k != VK.NONE).numpy()
    return listed


@pytest.mark.parametrize("case", VK.SEARCH_CASES, ids=lambda c: c.name)
def test_search_bit_identity_with_the_host_composition(case):
    """depth, last logit, flags and the last step's key equal `iters` single-step launches with view_search_ref's fp32 rule between them;
    flag bit 2 is set exactly on the rays some step of which selected no key; the world points are the exactly rounded expression."""
    feats, rays, cams, prior, m, dev = _setup(case)
    keys = []
    depth, logit, flags, steps = VS.compose(case, _probe(case, feats, rays, cams, prior, m, dev, keys))
    d, l, f, p, k = _run_search(case, dev)
    _same(d, torch.from_numpy(depth), f"{case.name} depth")
    _same(l, torch.from_numpy(logit), f"{case.name} last logit")
    assert torch.equal(f, torch.from_numpy(flags)), f"{case.name}: {int((f != torch.from_numpy(flags)).sum())} flags differ"
    keys = np.stack(keys)
    assert np.array_equal(k.numpy(), keys[-1]), f"{case.name}: the key of the last step differs"
    assert np.array_equal((f.numpy() & 4) != 0, (keys == VK.NONE).any(0))
    assert torch.equal(_bits(p), _bits(_points32(rays, d.numpy(), cams)))
    moved = (keys != keys[0]).any(0).mean()
    print(f"{case.name}: {case.rays} rays equal in bits; {(keys != VK.NONE).mean():.3f} of the probes have a key, {moved:.3f} of the rays change it")
    if case.pose == "behind":
        assert (keys == VK.NONE).all() and (f.numpy() == (5 if case.fill < 0 else 6)).all()
    for kw in (dict(want_flags=False), dict(want_points=False, want_key=False), dict(want_flags=False, want_points=False, want_key=False)):
        d2, l2, f2, p2, k2 = _run_search(case, dev, **kw)  # NULL optional outputs change nothing else
        assert torch.equal(_bits(d2), _bits(d)) and torch.equal(_bits(l2), _bits(l))
        assert (f2 is None or torch.equal(f2, f)) and (p2 is None or torch.equal(_bits(p2), _bits(p))) and (k2 is None or torch.equal(k2, k))


@pytest.mark.parametrize("case", [VK.SEARCH_CASES[0], VK.SEARCH_CASES[3], VK.SEARCH_CASES[5]], ids=lambda c: c.name)
def test_search_list_form_at_pixel_centres_is_the_grid_form(case):
    feats, rays, cams, prior, m, dev = _setup(case)
    for a, b in zip(_run_search(case, dev), _run_search(case, dev, listed=True)):
        assert torch.equal(_bits(a), _bits(b))


def test_search_with_one_key_is_the_single_key_search():
    case = next(c for c in VK.SEARCH_CASES if c.M == 1)
    feats, rays, cams, prior, m, dev = _setup(case)
    slot = case.slots[0]
    one = VS.Device(VK._Block(case), m, feats[slot], rays, VK.key_cams(cams, slot), None if prior is None else prior[slot])
    rc, *outs = VS.run_view_search(_lib(), VK._Block(case), one)
    assert rc == VK.OK
    d1, l1, f1, p1 = _read(outs)
    d, l, f, p, k = _run_search(case, dev)
    _same(d.view(-1), d1, "M = 1 depth")
    _same(l.view(-1), l1, "M = 1 last logit")
    assert torch.equal(f.view(-1), f1)
    _same(p.view(-1), p1, "M = 1 points")


# ---- 4. no read from a key that is not selected ----------------------------------------------------------------------------------
def _poisoned(case, dev, feats, prior, m_pos):
    """The device inputs with the feature block and the prior map of key ``m_pos`` (a position in key_slots) replaced by NaN."""
    slot = case.slots[m_pos]
    f2 = feats.clone()
    f2[slot] = R.NAN
    buf = VK.ring_buffer(case, f2)[0].cuda()
    pr = None
    if prior is not None:
        pr = dev.prior.clone()
        pr[slot] = R.NAN
    return buf, pr


@pytest.mark.parametrize("case", [VK.CASES[0], VK.CASES[3], VK.CASES[5]], ids=lambda c: c.name)
def test_dense_reads_nothing_from_unselected_keys(case):
    """With key m's features and prior map all NaN, every pixel that selected another key - or none - keeps its bits: no corner and no
    texel of a key is read for a pixel that did not select it.  (The pixels that selected key m turn NaN: the poison is in reach.)"""
    feats, rd, cams, prior, m, dev = _setup(case)
    l, k, d, p = _run(case, dev)
    for pos in range(case.M):
        buf, pr = _poisoned(case, dev, feats, prior, pos)
        keep = dev.prior
        dev.prior = pr
        try:
            l2, k2, d2, p2 = _run(case, dev, fbuf=buf)
        finally:
            dev.prior = keep
        other = k != pos
        assert torch.equal(k2, k) and torch.equal(_bits(d2), _bits(d)) and torch.equal(_bits(p2), _bits(p))
        assert torch.equal(_bits(l2)[other], _bits(l)[other]), f"{case.name}: a pixel that did not select key {pos} read it"
        assert bool(torch.isnan(l2[~other]).all()) and bool((~other).any())


def test_search_reads_nothing_from_unselected_keys():
    case = VK.SEARCH_CASES[3]
    feats, rays, cams, prior, m, dev = _setup(case)
    d, l, f, p, k = _run_search(case, dev)
    hist = np.stack([_run_search(case, dev, iters=n, want_flags=False, want_points=False)[4].numpy() for n in range(1, case.iters + 1)])
    for pos in range(case.M):
        buf, pr = _poisoned(case, dev, feats, prior, pos)
        keep = dev.prior
        dev.prior = pr
        try:
            d2, l2, f2, p2, k2 = _run_search(case, dev, fbuf=buf)
        finally:
            dev.prior = keep
        never = torch.from_numpy(~(hist == pos).any(0))  # rays no step of which selected key `pos`
        assert bool(never.any()) and bool((~never).any())
        for a, b in ((d, d2), (l, l2), (f, f2), (k, k2)):
            assert torch.equal(_bits(a)[never], _bits(b)[never]), f"{case.name}: a ray that never selected key {pos} read it"


# ---- 5. the public API ----------------------------------------------------------------------------------------------------------
def _select_public(per_key, fill):
    """query_view dictionaries, in priority order -> (view_pred, view_key, view_depth) of the first valid one."""
    return VK.first_valid([v["view_pred"] for v in per_key], [v["view_valid"] for v in per_key], [v["view_depth"] for v in per_key], fill)


@pytest.mark.parametrize("use_prior", [False, True])
def test_remember_and_query_view_keys_are_the_composition(use_prior):
    from implicit_depth_amd._lib import IdhError

    B, K, H, W, D = 2, 2, 16, 24, 16
    model, d0, pyr0, rd = _build(B, K, H, W, D, 1, use_prior=use_prior)
    Hs, Ws, h, w = 2 * H, 2 * W, 15, 20
    case = VK.KeysCase(64, B, Hs, Ws, 1, h, w, None, "wide")
    iK, wTc, cTw_ring, K_ring, pcTw_ring, _ = (t.cuda() for t in VK.cameras(case))
    rendered = V.rendered_map(B, 2, h, w, 7).cuda()
    fill = -4.5
    with pytest.raises(IdhError, match="no forward"):
        model.remember(cTw_ring[0], K_ring[0])
    singles, singles_d, slots = [], [], []
    th = _thresholder()
    for s in range(3):  # three forwards on different inputs, each remembered with its own camera (and prior)
        d = {k: v.cuda() for k, v in syn.cost_volume_inputs(B, K, 16, H, W, seed=s, behind_view=K - 1).items()}
        pyr = [t.cuda() for t in syn.encoder_pyramid(B, H * 4, W * 4, seed=s)]
        _fwd(model, d, pyr, rendered_depth=rd)
        pi = None
        if use_prior:
            pi = {"prior_prediction": torch.sigmoid(syn.randn((B, 1, Hs, Ws), 8 + s, "pp")).cuda(), "prior_cam_T_world": pcTw_ring[s]}
        slots.append(model.remember(cTw_ring[s], K_ring[s], prior_inputs=pi, capacity=4))
        # the single-key answers, right after their own forward
        singles.append(model.query_view(rendered, iK, wTc, cTw_ring[s], K_ring[s], prior_inputs=pi, fill=fill, return_points=True))
        singles_d.append((cTw_ring[s], K_ring[s], pi))
    assert slots == [0, 1, 2] and model._ring.slots_newest_first() == [2, 1, 0]

    def check():
        for order in (None, [0, 2, 1], [1]):
            got = model.query_view_keys(rendered, iK, wTc, order=order, fill=fill, return_points=True)
            assert set(got) == {"view_pred", "view_valid", "view_depth", "view_points", "view_key"}
            pri = [2, 1, 0] if order is None else order
            pred, key, depth = _select_public([singles[s] for s in pri], fill)
            assert torch.equal(got["view_pred"], pred) and torch.equal(got["view_key"], key) and torch.equal(got["view_depth"], depth)
            assert torch.equal(got["view_valid"], key != VK.NONE) and torch.equal(got["view_points"], singles[0]["view_points"])
            if order is None:
                shares = [(key == i).float().mean().item() for i in range(3)] + [(key == VK.NONE).float().mean().item()]
                assert min(shares) > 0.02, shares  # every remembered prediction answers somewhere, and somewhere none does
        return model.query_view_depths_keys(iK, wTc, size=(h, w), thresholder=th, fill=fill, return_points=True)

    first = check()
    assert set(first) == {"view_search_depths", "view_search_logits", "view_search_flags", "view_search_points", "view_search_key"}
    # a fourth forward overwrites the plan's buffers, not the ring: the answers stay (the copy is real)
    d = {k: v.cuda() for k, v in syn.cost_volume_inputs(B, K, 16, H, W, seed=3, behind_view=K - 1).items()}
    _fwd(model, d, [t.cuda() for t in syn.encoder_pyramid(B, H * 4, W * 4, seed=3)], rendered_depth=rd)
    changed = model.query_view(rendered, iK, wTc, cTw_ring[2], K_ring[2], prior_inputs=singles_d[2][2], fill=fill)
    assert not torch.equal(changed["view_pred"], singles[2]["view_pred"])  # the last forward's own buffers did change
    again = check()
    for k in first:
        assert torch.equal(first[k], again[k]), k
    # the search through the ring is the twelve-call composition of query_view_keys
    sd, logit, flags = _compose_public(lambda r: model.query_view_keys(r, iK, wTc, fill=fill), B, (h, w), th)
    assert torch.equal(first["view_search_depths"], sd) and torch.equal(first["view_search_logits"], logit) and torch.equal(first["view_search_flags"], flags)
    lst = model.query_view_depths_keys(iK, wTc, rays=VS.pixel_centres(B, h, w).cuda(), thresholder=th, fill=fill, return_points=True)
    for k in first:
        assert torch.equal(lst[k].reshape(-1), first[k].reshape(-1)), k
    # a fifth remember wraps the ring of four: the oldest prediction leaves
    assert model.remember(cTw_ring[0], K_ring[0], prior_inputs=singles_d[0][2], capacity=4) == 3
    assert model.remember(cTw_ring[0], K_ring[0], prior_inputs=singles_d[0][2], capacity=4) == 0
    assert model._ring.slots_newest_first() == [0, 3, 2, 1]
    with pytest.raises(IdhError, match="batch size"):
        model.query_view_keys(rendered[:1], iK[:1], wTc[:1])
    model.forget()
    with pytest.raises(IdhError, match="nothing is remembered"):
        model.query_view_keys(rendered, iK, wTc)
    model.binary_mlp.mlp_math = "f16x3"
    model.remember(cTw_ring[0], K_ring[0], capacity=4)
    with pytest.raises(IdhError, match="fp32 only"):
        model.query_view_keys(rendered, iK, wTc)


# ---- 6. streaming ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_prior", [False, True])
def test_streaming_session_asks_three_keyframes(use_prior):
    """A short pan (synthetic 'stream12': a keyframe every frame, frame 6 repeats frame 5).  On frame 6, where step() returned None, the
    session with query_keyframes = 3 answers occlusion_for_view / depth_for_view / raycast_view with the bits of the composition of the
    public single-key calls.  Those calls see the last prediction only, so a second session with the default query_keyframes = 1 runs
    the same frames and is asked right after each of the last three predictions, its answers kept; the composition is the first-valid
    select in the order nearest pose first, and for the depth the twelve-step rule over that, step by step: the single-key sessions are
    asked at the fused search's own queries q_n (its depths after n steps), and the rule on their selected answers must give q_n+1."""
    from implicit_depth_amd.streaming import StreamingSession, nearest_keys_first

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    multi = StreamingSession(_model("mlp", 3, use_prior=use_prior), buffer_size=BUFFER, query_keyframes=3)
    h, w, iters = 30, 40, 12
    invK = torch.linalg.inv(syn.intrinsics(w, h)).float()
    invK[:2, :3] *= 2.0  # a lens half as long as the keyframe's: the live image looks past every keyframe's
    invK = invK.cuda()
    predicted, slot_of = [], {}
    for t in range(7):
        out, code = multi.step(_frame(t, poses), world_T_cam=poses[t], dist_to_last_valid=dists[t])
        if out is not None:
            predicted.append(t)
            slot_of[t] = multi.hot._ring.slots_newest_first()[0]
    assert out is None and len(predicted) >= 3, predicted  # frame 6 is no keyframe; at least three predictions before it
    last3 = predicted[-3:]
    live = poses[6]
    newest_first = last3[::-1]
    order = [newest_first[i] for i in nearest_keys_first(live, [poses[t] for t in newest_first])]
    assert sorted(order) == sorted(last3)
    fill = -6.0
    rd = V.rendered_map(1, 2, h, w, 11, hostile=False).cuda()
    got = multi.occlusion_for_view(rd, live, invK, fill=fill)
    dv = multi.depth_for_view(live, invK, (h, w), fill=fill)
    T = torch.from_numpy(live.astype(np.float32))[None].cuda()
    # the fused search's own queries: q_0, then the depths after n = 1 .. 11 steps; twelve steps are depth_for_view's
    by_steps = lambda n: multi.hot.query_view_depths_keys(invK[None], T, size=(h, w), order=[slot_of[t] for t in order], iters=n, fill=fill)
    queries = [torch.full((1, 1, h, w), 3.75, device="cuda")] + [by_steps(n)["view_search_depths"] for n in range(1, iters)]
    assert torch.equal(by_steps(iters)["view_search_depths"], dv["view_search_depths"])  # the session asked the keys in that order

    # the parent commit's code path: a session that keeps the last prediction only, asked right after each of the last three predictions
    single = StreamingSession(_model("mlp", 3, use_prior=use_prior), buffer_size=BUFFER)
    occ, probes = {}, {}
    for t in range(last3[-1] + 1):
        out, _ = single.step(_frame(t, poses), world_T_cam=poses[t], dist_to_last_valid=dists[t])
        assert (out is not None) == (t in predicted)
        if t in last3:
            occ[t] = single.occlusion_for_view(rd, live, invK, fill=fill)
            probes[t] = [single.occlusion_for_view(q, live, invK, fill=fill) for q in queries]
    assert single.hot._ring is None and single.query_keyframes == 1
    # ... whose answers are those of its unchanged code path: HotPath.query_view on the last prediction
    k1 = single._key
    pi = {"prior_prediction": single._prior[0][:, :1], "prior_cam_T_world": single._prior[1]} if use_prior else None
    direct = single.hot.query_view(rd, invK[None], T, k1["cam_T_world_b44"], k1["K_s0_b44"], prior_inputs=pi, fill=fill)
    assert set(direct) == set(occ[last3[-1]]) and all(torch.equal(direct[k], occ[last3[-1]][k]) for k in ("view_pred", "view_valid", "view_depth"))

    pred, key, depth = _select_public([occ[t] for t in order], fill)
    assert torch.equal(got["view_pred"], pred) and torch.equal(got["view_key"], key) and torch.equal(got["view_depth"], depth)
    assert torch.equal(got["view_valid"], key != VK.NONE)
    # under the pan three keys see strictly more of the live view than the last key alone
    share3, share1 = got["view_valid"].float().mean().item(), occ[last3[-1]]["view_valid"].float().mean().item()
    print(f"valid share with three keys {share3:.3f}, with the last key alone {share1:.3f}; keys asked in the order {order}; "
          "key shares " + " ".join(f"{(key == i).float().mean().item():.3f}" for i in range(3)))
    assert share3 > share1

    # depth_for_view: the rule of bd_model.py:286-290 on the selected single-key answers, step by step (thr = logit(0.5) = 0)
    lo_t, hi_t = torch.full((1, 1, h, w), 0.5, device="cuda"), torch.full((1, 1, h, w), 8.0, device="cuda")
    flags = torch.zeros(1, 1, h, w, dtype=torch.uint8, device="cuda")
    for n in range(iters):
        sd = queries[n]
        logit, k, _ = _select_public([probes[t][n] for t in order], fill)
        vis = logit < 0
        hi_t, lo_t = torch.where(vis, sd, hi_t), torch.where(vis, lo_t, sd)
        flags |= (torch.where(vis, 1, 2) | torch.where(k != VK.NONE, 0, 4)).to(torch.uint8)
        nxt = (hi_t + lo_t) * 0.5
        assert torch.equal(nxt, queries[n + 1] if n + 1 < iters else dv["view_search_depths"]), f"step {n}"
    assert torch.equal(dv["view_search_logits"], logit) and torch.equal(dv["view_search_flags"], flags) and torch.equal(dv["view_search_key"], k)
    assert dv["view_search_points"].shape == (1, 1, h, w, 3)
    cast = multi.raycast_view(VS.pixel_centres(1, h, w).cuda(), live, invK, fill=fill)
    for name in dv:
        assert torch.equal(cast[name].reshape(-1), dv[name].reshape(-1)), name
    # reset() empties the ring
    multi.reset()
    assert len(multi.hot._ring) == 0 and multi._ring_poses == {}
