"""Occlusion and depth in a moving camera against several remembered keyframes, without a GPU: the case table, the selection shares and
the margin rule on the fp64 first-valid chain alone (tests/view_keys_ref.py), that chain against per-key calls of view_query_ref, the
session's key order, and every refusal of idh_binary_mlp_view_keys_fwd / idh_binary_mlp_view_keys_search_fwd, mlp.view_keys_logits /
view_keys_depths, PredictionRing, HotPath.remember / query_view_keys / query_view_depths_keys and StreamingSession(query_keyframes=...)
that is decided on the host."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import view_keys_ref as VK

V, VS, Q, R = VK.V, VK.VS, VK.Q, VK.R
_DENSE, _SIM = {}, {}


def _lib():
    from implicit_depth_amd import _lib as L

    return L.lib()


def _dense(case):
    if case.name not in _DENSE:
        feats, rd, cams, prior = VK.case_inputs(case)
        w = R.weights64(R.make_net(case.cf, case.has_prior, R._seed(case.name)))
        _DENSE[case.name] = (feats, rd, cams, prior, w, VK.reference(case, w, feats, rd, cams, prior))
    return _DENSE[case.name]


def _sim(case):
    if case.name not in _SIM:
        feats, rays, cams, prior = VK.case_inputs(case)
        w = R.weights64(VK.search_net(case))
        _SIM[case.name] = (feats, rays, cams, prior, w, VK.simulate(case, w, feats, rays, cams, prior))
    return _SIM[case.name]


# ---- the case table, the selection and the margin rule, on the fp64 chain alone ----------------------------------------------
def test_case_table_covers_the_issue():
    for cs, dense in ((VK.CASES, True), (VK.SEARCH_CASES, False)):
        assert any(c.B == 2 and c.M == 3 and (c.h, c.w) == (7, 9) and (not dense or c.P == 3) and c.rays % 16 for c in cs)
        assert any(c.rays == 15 for c in cs) and any(c.M == 1 for c in cs)
        assert any(c.n_slots == 4 and c.M == 3 and c.slots != tuple(sorted(c.slots)) for c in cs)
        assert any(c.pose == "behind" for c in cs)
        assert {c.layout for c in cs} == set(Q.LAYOUTS) and {c.cf for c in cs} == {64, 128}
        assert {"map", None} <= {c.prior for c in cs} and any(isinstance(c.prior, float) for c in cs)
        assert {(c.H, c.W) for c in cs} == {(12, 16), (24, 32)}
        large = [c for c in cs if c in VK.LARGE]
        assert len(large) == 1 and (large[0].rays + 15) // 16 > 1024 and large[0].M == 2  # the persistent 12-wave form
    assert sum(c.listed for c in VK.SEARCH_CASES) == 1 and VK.LISTED.listed
    assert any(c.stride_pad is not None and c.stride_pad % 4 for c in VK.CASES)  # rows 16-byte aligned, the key stride not
    assert VK.KEY_YAW[:3] == (-0.5, 0.0, 0.5)


@pytest.mark.parametrize("case", VK.CASES, ids=lambda c: c.name)
def test_selection_and_margin_of_each_dense_case(case):
    feats, rd, cams, prior, w, (ref, sel, near, ch, chains) = _dense(case)
    share = near.float().mean().item()
    shares = [(sel == m).float().mean().item() for m in range(case.M)] + [(sel == VK.NONE).float().mean().item()]
    print(f"{case.name}: key shares " + " ".join(f"{s:.3f}" for s in shares[:-1]) + f", none {shares[-1]:.3f}, within the margin {share:.4f}")
    assert share <= VK.NEAR_CAP, (case.name, share)
    if case.rays < 100:  # (63 pixels: one pixel is more than the cap)
        assert not bool(near.any())
    if case.pose == "behind":
        assert bool((sel == VK.NONE).all()) and bool((ref == case.fill).all())
    if case.main:
        assert min(shares) >= VK.MIN_SHARE, (case.name, shares)
    # the fp32 chain cannot carry a kept pixel across a boundary of any key: its error is below the margin wherever a key's decision is open
    # (in front of that camera, within a pixel of its image; further out the pixel is invalid on both sides)
    for c in chains:
        u, v = c["uv"][..., 0], c["uv"][..., 1]
        open_ = c["dok"] & (c["cz"] > 0) & (u > -1) & (u < case.W + 1) & (v > -1) & (v < case.H + 1)
        assert float(c["e_cz"][c["dok"]].max()) < VK.PROJ_MARGIN / 2
        assert not open_.any() or float(c["e_uv"][open_].max()) < VK.PROJ_MARGIN / 2


@pytest.mark.parametrize("case", VK.SEARCH_CASES, ids=lambda c: c.name)
def test_selection_and_margin_of_each_search_case(case):
    feats, rays, cams, prior, w, (depth, flags, steps) = _sim(case)
    assert len(steps) == case.iters
    for n, st in enumerate(steps):
        share = st["near"].mean()
        assert share <= VK.NEAR_CAP, (case.name, n, share)
        if case.rays < 100:  # (63 rays: one ray is more than the cap)
            assert not st["near"].any()
    sels = np.stack([st["sel"] for st in steps])
    shares = [(sels == m).mean() for m in range(case.M)] + [(sels == VK.NONE).mean()]
    moved = (sels != sels[0]).any(0).mean()
    print(f"{case.name}: key shares over the probes " + " ".join(f"{s:.3f}" for s in shares[:-1]) + f", none {shares[-1]:.3f}; "
          f"{moved:.3f} of the rays change their key along the search; flags " + " ".join(f"{v}:{(flags == v).mean():.2f}" for v in range(1, 8)))
    assert np.isfinite(depth).all() and (depth >= np.float32(case.lo)).all() and (depth <= np.float32(case.hi)).all()
    assert (((flags & 4) != 0) == (sels == VK.NONE).any(0)).all()  # bit 2: some step had no key
    if case.pose == "behind":
        assert (sels == VK.NONE).all() and (flags == (5 if case.fill < 0 else 6)).all()
    if case.main:
        first = [(sels[0] == m).mean() for m in range(case.M)] + [(sels[0] == VK.NONE).mean()]
        assert min(first) >= VK.MIN_SHARE, (case.name, first)
    if case in VK.LARGE:
        assert moved > 0.001  # every step selects its own key: some rays cross from one key's image into another's


@pytest.mark.parametrize("case", [c for c in VK.CASES if c not in VK.LARGE], ids=lambda c: c.name)
def test_first_valid_reference_is_the_per_key_chain_and_select(case):
    """The reference (one MLP pass on the selected key's inputs) against M direct calls of view_query_ref.reference - chain64 and the MLP per
    key - followed by the select; with M = 1 it IS view_query_ref.reference."""
    feats, rd, cams, prior, w, (ref, sel, near, ch, chains) = _dense(case)
    per_key = [V.reference(w, feats[s], rd, VK.key_cams(cams, s), None if prior is None else prior[s], VK.prior_const(case), case.fill) for s in case.slots]
    valid = [c["valid"] for _, c in per_key]
    want, key, z = VK.first_valid([l.view(case.B, -1) for l, _ in per_key], valid, [c["z"] for _, c in per_key], case.fill)
    assert torch.equal(key.long(), sel)
    assert torch.equal(z, ch["z"])
    assert torch.allclose(ref.view(case.B, -1), want, rtol=1e-12, atol=1e-12)
    for m, c in enumerate(chains):
        for k in ("uv", "z", "valid", "near"):
            assert torch.equal(c[k], per_key[m][1][k])
    if case.M == 1:
        assert torch.equal(ref, per_key[0][0]) and torch.equal(near, per_key[0][1]["near"])


def test_search_chain_list_form_is_the_grid_form_at_pixel_centres():
    case = VK.SEARCH_CASES[0]
    feats, rays, cams, prior = VK.case_inputs(case)
    w = R.weights64(VK.search_net(case))
    listed = VK.KeysSearchCase(case.cf, case.B, case.H, case.W, case.h, case.w, case.prior, case.layout, slots=case.slots, thr=case.thr, fill=case.fill,
                               listed=True, list_n=case.N)
    q = 0.5 + 7.5 * torch.rand(case.shape, generator=torch.Generator().manual_seed(3))
    a = VK.step64(case, w, feats, rays, cams, prior, q)
    b = VK.step64(listed, w, feats, rays, cams, prior, q)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_session_key_order():
    """Nearest pose first by keyframes.pose_distance; equal distances go to the newer key (the list is newest first)."""
    from implicit_depth_amd import keyframes
    from implicit_depth_amd.streaming import nearest_keys_first

    def pose(x, yaw=0.0):
        T = np.eye(4)
        c, s = np.cos(yaw), np.sin(yaw)
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = c, s, -s, c
        T[0, 3] = x
        return T

    live = pose(0.0)
    keys = [pose(0.5), pose(0.1), pose(-0.3), pose(0.0, yaw=0.2)]  # newest first
    order = nearest_keys_first(live, keys)
    d = [keyframes.pose_distance(live, k)[0] for k in keys]
    assert order == sorted(range(4), key=lambda i: d[i]) == [1, 3, 2, 0]
    assert nearest_keys_first(live, [pose(0.2), pose(-0.2), pose(0.1), pose(-0.2)]) == [2, 0, 1, 3]  # ties: the newer key first
    assert nearest_keys_first(live, [pose(1.0)]) == [0] and nearest_keys_first(live, []) == []
    assert nearest_keys_first(live.astype(np.float32), [k.astype(np.float32) for k in keys]) == order


# ---- refusals of the C entry points, decided before the device is touched ------------------------------------------------------------
P = 0x1000  # a non-null, 16-byte-aligned address that is never dereferenced: every call below must return before any launch
_SLOTS = {}


def _slots(*s):
    """A live host array: key_slots is read on the host."""
    if s not in _SLOTS:
        _SLOTS[s] = (C.c_int * max(len(s), 1))(*s)
    return _SLOTS[s]


DENSE_ARGS = dict(feat=P, feat_cs=64, Cf=64, B=2, H=5, W=7, key_stride=2 * 5 * 7 * 64, n_slots=4, key_slots=(0, 1, 2), M=3, rendered=P, P=2, h=3, w=4,
                  invK=P, world_T_cam=P, key_cam_T_world=P, key_K=P, prior_pred=None, prior_cam_T_world=None, prior_K=None, has_prior=0,
                  prior_const=0.0, w1f=P, w2=P, vecs=P, fill=0.0, logits=P, key=None, view_depth=None, view_points=None, stream=None)
SEARCH_ARGS = dict(feat=P, feat_cs=64, Cf=64, B=2, H=5, W=7, key_stride=2 * 5 * 7 * 64, n_slots=4, key_slots=(0, 1, 2), M=3, h=3, w=4, rays=None, N=0,
                   invK=P, world_T_cam=P, key_cam_T_world=P, key_K=P, prior_pred=None, prior_cam_T_world=None, prior_K=None, has_prior=0,
                   prior_const=0.0, w1f=P, w2=P, vecs=P, iters=12, lo=0.5, hi=8.0, threshold=0.5, bins=None, thr_logits=None, n_bins=0, fill=0.0,
                   depth=P, last_logits=P, flags=None, points=None, key=None, stream=None)
INF, NAN = float("inf"), float("nan")


def _key_rows(add):
    """The conditions both entry points add to their parents'."""
    add(VK.EINVAL, M=0)
    add(VK.EINVAL, M=-1)
    add(VK.EINVAL, key_slots=None)
    add(VK.EINVAL, key_slots=(0, 4, 1))  # outside [0, n_slots)
    add(VK.EINVAL, key_slots=(0, -1, 1))
    add(VK.EINVAL, key_slots=(0, 1, 0))  # a duplicate
    add(VK.EINVAL, n_slots=0)
    add(VK.EINVAL, key_stride=2 * 5 * 7 * 64 - 1)  # blocks of a ring of several slots overlap
    add(VK.EINVAL, key_stride=-4)
    add(VK.OK, key_stride=0, n_slots=1, key_slots=(0,), M=1, B=0)  # (a one-slot ring has no stride to check; B = 0: no launch)
    add(VK.EINVAL, key_stride=0, n_slots=1, key_slots=(0,), M=1, feat=None)  # ... and the call gets as far as the NULL feat
    add(VK.EUNSUPPORTED, n_slots=17, key_slots=tuple(range(17)), M=17)
    add(VK.EUNSUPPORTED, B=43, key_stride=43 * 5 * 7 * 64)  # M * B = 129 cameras
    add(VK.EUNSUPPORTED, n_slots=1 << 26, key_stride=1 << 40)  # n_slots * B * H * W >= 2^31
    add(VK.EINVAL, feat=P + 2)
    add(VK.EINVAL, key_cam_T_world=None)
    add(VK.EINVAL, key_K=P + 2)
    for k in ("H", "W", "Cf"):
        add(VK.EINVAL, **{k: 0})
    add(VK.EINVAL, Cf=62)
    add(VK.EINVAL, feat_cs=60)
    prior = dict(prior_pred=P, prior_cam_T_world=P, prior_K=P, has_prior=1)
    for k in ("prior_cam_T_world", "prior_K"):
        add(VK.EINVAL, **dict(prior, **{k: None}))
    add(VK.EINVAL, **dict(prior, has_prior=0))
    add(VK.EUNSUPPORTED, B=129, M=1, key_slots=(0,), key_stride=129 * 5 * 7 * 64)
    # which rule wins: the keys are looked at after the pointers and before the sizes, and each of their rules in its own order
    add(VK.EINVAL, B=0, Cf=62)
    add(VK.EINVAL, **dict(prior, has_prior=0, B=0))
    add(VK.EINVAL, key_slots=None, B=129)
    add(VK.EINVAL, n_slots=17, key_slots=tuple(range(17)), M=17, feat=P + 2)
    add(VK.EINVAL, n_slots=17, key_slots=tuple(range(17)), M=17, key_stride=-4)
    add(VK.EUNSUPPORTED, n_slots=17, key_slots=(0, 0) + tuple(range(2, 17)), M=17)  # too many keys, before they are read
    add(VK.EINVAL, key_slots=(0, 1, 0), B=43, key_stride=43 * 5 * 7 * 64)
    add(VK.EINVAL, key_stride=129 * 5 * 7 * 64 - 1, B=129)  # overlapping blocks, before M * B


def _dense_rows():
    rs = []
    add = lambda code, **kw: rs.append((kw, code))
    _key_rows(add)
    for k in ("feat", "rendered", "invK", "world_T_cam", "key_K", "w1f", "w2", "vecs", "logits"):
        add(VK.EINVAL, **{k: None})
    for k in ("B", "P", "h", "w"):
        add(VK.EINVAL, **{k: -1})
        add(VK.OK, **{k: 0})
        add(VK.OK, **{k: 0, "feat": None, "logits": None, "key_slots": None, "M": 0})  # an empty map: no launch, nothing is read, M is not looked at
    for k in ("rendered", "logits", "view_depth", "view_points"):
        add(VK.EINVAL, **{k: P + 2})
    add(VK.EUNSUPPORTED, B=8, P=1, h=1 << 14, w=1 << 14, key_stride=8 * 5 * 7 * 64)  # B * P * h * w >= 2^31
    add(VK.EUNSUPPORTED, B=1, P=1 << 16, h=1 << 16, w=4, key_stride=5 * 7 * 64)
    return rs


def _search_rows():
    rs = []
    add = lambda code, **kw: rs.append((kw, code))
    _key_rows(add)
    for k in ("feat", "invK", "world_T_cam", "w1f", "w2", "vecs", "depth", "last_logits"):
        add(VK.EINVAL, **{k: None})
    for k in ("B", "h", "w"):
        add(VK.EINVAL, **{k: -1})
        add(VK.OK, **{k: 0})
        add(VK.OK, **{k: 0, "feat": None, "depth": None, "key_slots": None, "M": 0})
    add(VK.EINVAL, rays=P, N=-1)
    add(VK.OK, rays=P, N=0, feat=None)
    add(VK.EINVAL, rays=P + 2, N=5)
    for k in ("depth", "last_logits", "points"):
        add(VK.EINVAL, **{k: P + 2})
    add(VK.EINVAL, iters=0)
    add(VK.EINVAL, n_bins=-1)
    for t in (0.0, 1.0, NAN):
        add(VK.EINVAL, threshold=t)
    add(VK.EINVAL, n_bins=3, bins=None, thr_logits=P)
    add(VK.EINVAL, n_bins=3, bins=P, thr_logits=None)
    for lo, hi in ((0.0, 8.0), (2.0, 2.0), (NAN, 8.0), (0.5, INF)):
        add(VK.EINVAL, lo=lo, hi=hi)
    add(VK.EUNSUPPORTED, B=8, h=1 << 14, w=1 << 14, key_stride=8 * 5 * 7 * 64)
    add(VK.EUNSUPPORTED, B=4, rays=P, N=1 << 29, key_stride=4 * 5 * 7 * 64)
    return rs


def _call(fn, base, over):
    args = dict(base)
    assert set(over) <= set(args)
    args.update(over)
    if args["key_slots"] is not None:
        args["key_slots"] = _slots(*args["key_slots"])
    return fn(*args.values())


_ids = lambda r: f"{'-'.join(f'{k}={v}' for k, v in r[0].items())}-{r[1]}"[:120]


@pytest.mark.parametrize("row", _dense_rows(), ids=_ids)
def test_dense_refusals_and_their_codes(row):
    assert _call(_lib().idh_binary_mlp_view_keys_fwd, DENSE_ARGS, row[0]) == row[1]


@pytest.mark.parametrize("row", _search_rows(), ids=_ids)
def test_search_refusals_and_their_codes(row):
    assert _call(_lib().idh_binary_mlp_view_keys_search_fwd, SEARCH_ARGS, row[0]) == row[1]


def test_library_and_header_declare_both_entry_points():
    from implicit_depth_amd import _lib as L

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "idh.h")).read()
    for name in ("idh_binary_mlp_view_keys_fwd", "idh_binary_mlp_view_keys_search_fwd"):
        assert callable(getattr(_lib(), name)) and name in L.declared_symbols()
        assert f"int {name}(" in header


# ---- Python-level refusals -------------------------------------------------------------------------------------------
def _hot(use_prior=False):
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from implicit_depth_amd.pipeline import HotPath

    cve = net.CVEncoder(8, [48, 64, 160, 256], [64, 128, 256, 384])
    dec = net.BDDecoderPP([24] + cve.num_ch_enc)
    return HotPath(CostVolumeManager(16, 24, 8), cve, dec, net.BinaryMLPNetwork(dec.num_ch_dec, use_prior=use_prior))


EYE = torch.eye(4)[None]


def test_wrappers_refuse_f16x3_and_bad_rings():
    from implicit_depth_amd import mlp
    from implicit_depth_amd._lib import IdhError

    hot = _hot()
    ring, cams = torch.zeros(2, 1, 4, 4, 64), EYE.expand(2, 1, 4, 4)
    rd = torch.ones(1, 1, 3, 3)
    with pytest.raises(IdhError, match="CPU tensor"):
        mlp.view_keys_logits(hot.binary_mlp, ring, 0, 64, [0, 1], rd, EYE, EYE, cams, cams)
    with pytest.raises(IdhError, match="CPU tensor"):
        mlp.view_keys_depths(hot.binary_mlp, ring, 0, 64, [0, 1], EYE, EYE, cams, cams, size=(2, 2))
    hot.binary_mlp.mlp_math = "f16x3"
    with pytest.raises(IdhError, match="fp32 only.*idh_binary_mlp_view_keys_fwd"):
        mlp.view_keys_logits(hot.binary_mlp, ring, 0, 64, [0, 1], rd, EYE, EYE, cams, cams)
    with pytest.raises(IdhError, match="fp32 only.*idh_binary_mlp_view_keys_search_fwd"):
        mlp.view_keys_depths(hot.binary_mlp, ring, 0, 64, [0, 1], EYE, EYE, cams, cams, size=(2, 2))


def test_ring_and_hot_path_refusals():
    from implicit_depth_amd import pipeline
    from implicit_depth_amd._lib import IdhError

    for cap in (0, 17, -1):
        with pytest.raises(IdhError, match="capacity"):
            pipeline.PredictionRing(cap)
    ring = pipeline.PredictionRing(3)
    assert len(ring) == 0 and ring.slots_newest_first() == [] and ring.B is None
    hot = _hot()
    rd = torch.ones(1, 1, 3, 3)
    with pytest.raises(IdhError, match="no forward"):
        hot.remember(EYE, EYE)
    with pytest.raises(IdhError, match="nothing is remembered"):
        hot.query_view_keys(rd, EYE, EYE)
    with pytest.raises(IdhError, match="exactly one"):
        hot.query_view_depths_keys(EYE, EYE)
    with pytest.raises(IdhError, match="nothing is remembered"):
        hot.query_view_depths_keys(EYE, EYE, size=(3, 3))
    # a ring that holds predictions of batch size 1 (its storage is only looked at for its shape here)
    ring.feat, ring.cam_T_world, ring.K = torch.zeros(3, 1, 4, 4, 64), EYE.expand(3, 1, 4, 4), EYE.expand(3, 1, 4, 4)
    ring._next, ring._count = 2, 2
    assert ring.slots_newest_first() == [1, 0] and ring.B == 1
    ring._next, ring._count = 1, 3  # wrapped: slot 0 is the newest, slot 1 the oldest
    assert ring.slots_newest_first() == [0, 2, 1]
    hot._ring = ring
    E2 = EYE.expand(2, 4, 4)
    with pytest.raises(IdhError, match="batch size"):
        hot.query_view_keys(torch.ones(2, 1, 3, 3), E2, E2)
    with pytest.raises(IdhError, match="batch size"):
        hot.query_view_depths_keys(E2, E2, size=(3, 3))
    ring._next, ring._count = 2, 2
    with pytest.raises(IdhError, match="holds no prediction"):
        hot.query_view_keys(rd, EYE, EYE, order=[0, 2])
    with pytest.raises(IdhError, match="CPU tensor"):
        hot.query_view_keys(rd, EYE, EYE)
    hot.forget()
    with pytest.raises(IdhError, match="nothing is remembered"):
        hot.query_view_keys(rd, EYE, EYE)


def test_session_refuses_query_keyframes_out_of_range():
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    for n in (0, -1, 17):
        with pytest.raises(IdhError, match="query_keyframes"):
            StreamingSession(_hot(), query_keyframes=n)
