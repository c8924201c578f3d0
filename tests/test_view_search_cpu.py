"""Depth in a moving camera without a GPU: the case table and the margin rule on the fp64 simulation alone (tests/view_search_ref.py), the
simulation against mutants and against the reference's own modules (tests/golden/view_search.npz), and every refusal of
idh_binary_mlp_view_search_fwd, mlp.view_depths, HotPath.query_view_depths and StreamingSession.depth_for_view / raycast_view that is
decided on the host."""
import numpy as np
import pytest
import torch

import view_search_ref as VS
from conftest import TOL, load_golden

V, Q, R = VS.V, VS.Q, VS.R
_SIM = {}


def _lib():
    from implicit_depth_amd import _lib as L

    return L.lib()


def _sim(case):
    """The fp64 simulation of a case, computed once and shared."""
    if case.name not in _SIM:
        feat, rays, cams, prior = VS.case_inputs(case)
        w = R.weights64(VS.search_net(case))
        _SIM[case.name] = (feat, rays, cams, prior, w, VS.simulate(case, w, feat, rays, cams, prior))
    return _SIM[case.name]


# ---- the case table and the margin rule, on the simulation alone ---------------------------------------------------------
def test_case_table_covers_the_issue():
    cs = VS.CASES
    grids = {(c.B, c.h, c.w) for c in cs if not c.listed}
    assert (1, 5, 3) in grids and (2, 7, 9) in grids and (1, 101, 163) in grids
    assert {c.layout for c in cs} == set(Q.LAYOUTS) and {c.cf for c in cs} == {64, 128}
    assert any(c.camera == "behind" for c in cs) and any(c.iters == 1 for c in cs)
    assert any((c.lo, c.hi, c.thr) == (1.0, 3.0, "clamp") for c in cs)
    assert any(c.B == 2 and c.camera == "moved" and c.prior == "map" and c.table and c.layout == "base1" and (c.h * c.w) % 16 for c in cs)
    assert sum(c.listed for c in cs) == 1 and VS.LISTED.N == 37
    assert len(VS.LARGE) == 1 and (VS.LARGE[0].rays + 15) // 16 == 1029  # more tiles than 256 workgroups x 4 waves: the persistent form
    _, rays, _, _ = VS.case_inputs(VS.LISTED)
    x, y = rays[..., 0], rays[..., 1]
    centre = ((x - 0.5) == torch.floor(x)) & ((y - 0.5) == torch.floor(y))
    outside = (x < 0) | (x > VS.LISTED.w) | (y < 0) | (y > VS.LISTED.h)
    assert centre.sum() >= 12 and outside.sum() >= 12 and (~centre & ~outside).sum() >= 12


@pytest.mark.parametrize("case", VS.SMALL, ids=lambda c: c.name)
def test_margin_rule_and_mix_of_each_case(case):
    """Per case and step, on the fp64 simulation alone: at most NEAR_CAP of the probes lie within PROJ_MARGIN of a validity or prior-texel
    boundary; and the probes are the mix the case promises."""
    feat, rays, cams, prior, w, (depth, flags, steps) = _sim(case)
    assert len(steps) == case.iters
    for n, st in enumerate(steps):
        share = st["near"].mean()
        assert share <= VS.NEAR_CAP, (case.name, n, share)
    valid = np.stack([st["valid"] for st in steps])  # iters, B, N
    print(f"{case.name}: {valid.mean():.3f} of the probes valid, flags " + " ".join(f"{v}:{(flags == v).mean():.2f}" for v in range(1, 8)))
    assert np.isfinite(depth).all() and (depth >= np.float32(case.lo)).all() and (depth <= np.float32(case.hi)).all()
    if case.camera == "behind":
        want = 5 if case.fill < 0 else 6  # thr = logit(0.5) = 0: fill < 0 reads as visible at every step
        assert not valid.any() and (flags == want).all()
        return
    assert valid.any()
    if valid[0].sum() > 8:
        first = steps[0]["vis"][valid[0]]
        assert 0.25 <= first.mean() <= 0.75  # search_net's shift: the first decisions split
    if case is VS.CROSSING:
        mixed = valid.any(0) & ~valid.all(0)
        assert mixed.sum() > 20 and ((flags & 7) == 7).sum() > 5  # valid and invalid probes on the same ray; rays that come back from outside
        tiles = np.pad(valid.reshape(case.iters, -1), ((0, 0), (0, -case.rays % 16))).reshape(case.iters, -1, 16).any(-1)  # iters, tiles
        assert (tiles.any(0) & ~tiles.all(0)).any()  # a tile with no valid probe at some steps but not at others
    if case.table:
        idx = np.stack([st["idx"] for st in steps])
        assert len(np.unique(idx)) > 1
        if case.thr == "clamp":
            assert (idx >= len(case.table[0])).any()  # the count reaches n_bins and is clamped


def test_list_chain_is_the_grid_chain_at_pixel_centres():
    case = VS.CASES[1]
    feat, rays, cams, prior = VS.case_inputs(case)
    q = 0.5 + 7.5 * torch.rand(case.shape, generator=torch.Generator().manual_seed(3))
    a = V.chain64(q.view(case.B, 1, case.h, case.w), cams, case.H, case.W, prior)
    b = VS.chain64_rays(rays, q, cams, case.H, case.W, prior)
    for k in a:
        assert torch.equal(a[k], b[k]), k


MUTANTS = ("no_half_pixel", "transposed_pose")


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_simulation_discriminates(mutant):
    """A mutant of the chain - pixel corners instead of centres, the view pose's rotation transposed - changes the simulated depth on a
    clear majority of the rays whose search the true chain brackets."""
    for case in (VS.CASES[1], VS.CROSSING):
        feat, rays, cams, prior, w, (depth, flags, _) = _sim(case)
        if mutant == "no_half_pixel":
            mrays, mcams = rays - 0.5, cams
        else:
            T = cams[1].clone()
            T[:, :3, :3] = T[:, :3, :3].transpose(1, 2)
            mrays, mcams = rays, (cams[0], T) + tuple(cams[2:])
        listed = VS.ViewSearchCase(case.cf, case.B, case.H, case.W, case.h, case.w, case.camera, case.prior, case.layout, case.thr, case.lo, case.hi,
                                   case.fill, case.iters, listed=True, list_n=case.N)  # the grid's rays as a list
        mdepth, _, _ = VS.simulate(listed, w, feat, mrays, mcams, prior)
        same, _, _ = VS.simulate(listed, w, feat, rays, cams, prior)
        assert np.array_equal(same, depth)  # the list form of the simulation is the grid form's
        keep = (flags & 3) == 3
        changed = (mdepth != depth)[keep].mean()
        print(f"{case.name}: {mutant} changes {changed:.2f} of {int(keep.sum())} bracketed rays")
        assert keep.sum() > 10 and changed > 0.5, (case.name, mutant, changed)


def test_simulation_reproduces_the_references_search():
    """tests/golden/view_search.npz: BackprojectDepth, Project3D, F.grid_sample, BinaryMLPNetwork and the loop of bd_model.py:279-290 from
    the reference's own modules.  Depths agree where the reference's smallest per-step |logit - thr| exceeds the logit tolerance."""
    g = load_golden("view_search")
    feat, cams = VS.golden_inputs()
    for k, t in zip(("invK", "world_T_cam", "key_cam_T_world", "key_K"), cams[:4]):
        assert np.array_equal(g[k], t.numpy()), k  # the seeds still give the generator's inputs
    fd = feat.double()
    assert np.array_equal(g["feat_chk"], np.array([fd.sum().item(), fd.abs().sum().item(), (fd * fd).sum().item()]))
    case = VS.GOLDEN_CASE
    w = R.weights64(VS.golden_net())
    depth, flags, steps = VS.simulate(case, w, feat, VS.pixel_centres(case.B, case.h, case.w), cams, None)
    scale = float(g["logit_scale"])
    sure = g["search_margin"].reshape(case.shape) > TOL * scale
    agree = depth == g["search_depths"].reshape(case.shape)
    print(f"golden: {agree.mean():.2%} of the depths equal, {sure.mean():.2%} with a margin above the tolerance")
    assert sure.mean() > 0.5 and agree[sure].all()
    assert len(np.unique(depth)) > 8


# ---- refusals, decided before the device is touched -----------------------------------------------------------------------
P = 0x1000  # a non-null, 16-byte-aligned address that is never dereferenced: every call below must return before any launch
OK_ARGS = dict(feat=P, feat_cs=64, Cf=64, B=2, H=5, W=7, h=3, w=4, rays=None, N=0, invK=P, world_T_cam=P, key_cam_T_world=P, key_K=P, prior_pred=None,
               prior_cam_T_world=None, prior_K=None, has_prior=0, prior_const=0.0, w1f=P, w2=P, vecs=P, iters=12, lo=0.5, hi=8.0, threshold=0.5,
               bins=None, thr_logits=None, n_bins=0, fill=0.0, depth=P, last_logits=P, flags=None, points=None, stream=None)
INF, NAN = float("inf"), float("nan")


def _rows():
    rs = []
    add = lambda code, **kw: rs.append((kw, code))
    for k in ("feat", "invK", "world_T_cam", "key_cam_T_world", "key_K", "w1f", "w2", "vecs", "depth", "last_logits"):
        add(VS.V.EINVAL, **{k: None})
    for k in ("B", "h", "w"):
        add(V.EINVAL, **{k: -1})
        add(V.OK, **{k: 0})
        add(V.OK, **{k: 0, "feat": None, "depth": None})  # B == 0 or an empty grid: no launch, nothing is read
    add(V.EINVAL, rays=P, N=-1)
    add(V.OK, rays=P, N=0, feat=None)  # an empty list
    add(V.EINVAL, rays=P, N=5, h=-1, w=-1, feat=None)  # h and w are ignored with a list: the call gets as far as the NULL feat
    add(V.EINVAL, rays=P + 2, N=5)
    for k in ("H", "W", "Cf"):
        add(V.EINVAL, **{k: 0})
        add(V.EINVAL, **{k: -3})
    add(V.EINVAL, Cf=62)
    add(V.EINVAL, feat_cs=60)
    for k in ("feat", "invK", "world_T_cam", "key_cam_T_world", "key_K", "depth", "last_logits", "points"):
        add(V.EINVAL, **{k: P + 2})  # not 4-byte aligned
    prior = dict(prior_pred=P, prior_cam_T_world=P, prior_K=P, has_prior=1)
    for k in ("prior_cam_T_world", "prior_K"):
        add(V.EINVAL, **dict(prior, **{k: None}))
    add(V.EINVAL, **dict(prior, has_prior=0))
    add(V.EINVAL, **dict(prior, prior_pred=P + 2))
    # the search's own
    add(V.EINVAL, iters=0)
    add(V.EINVAL, n_bins=-1)
    for t in (0.0, 1.0, -0.1, NAN):
        add(V.EINVAL, threshold=t)
    add(V.EINVAL, n_bins=3, bins=None, thr_logits=P)
    add(V.EINVAL, n_bins=3, bins=P, thr_logits=None)
    add(V.EINVAL, n_bins=3, bins=P + 2, thr_logits=P)
    for lo, hi in ((0.0, 8.0), (-1.0, 8.0), (2.0, 2.0), (3.0, 1.0), (NAN, 8.0), (0.5, NAN), (0.5, INF), (INF, INF)):
        add(V.EINVAL, lo=lo, hi=hi)
    add(V.EUNSUPPORTED, B=8, h=1 << 14, w=1 << 14)  # B * h * w >= 2^31
    add(V.EUNSUPPORTED, B=1, h=1 << 16, w=1 << 16)
    add(V.EUNSUPPORTED, B=4, rays=P, N=1 << 29)
    add(V.EUNSUPPORTED, B=1 << 12, H=1 << 10, W=1 << 10)  # B * H * W >= 2^31
    add(V.EUNSUPPORTED, B=129)  # the cameras of one launch sit in LDS
    # which rule wins: argument errors, then the empty call, then the pointers, then the sizes
    add(V.EINVAL, B=0, iters=0)
    add(V.EINVAL, h=0, threshold=1.0)
    add(V.EINVAL, w=0, lo=0.0)
    add(V.EINVAL, **dict(prior, has_prior=0, B=0))
    add(V.EINVAL, rays=P, N=0, n_bins=3)
    add(V.OK, h=0, B=129)
    add(V.OK, B=0, depth=P + 2)
    add(V.EINVAL, feat=None, B=129)
    add(V.EINVAL, points=P + 2, B=8, h=1 << 14, w=1 << 14)
    add(V.EINVAL, hi=INF, B=1 << 12, H=1 << 10, W=1 << 10)
    return rs


@pytest.mark.parametrize("row", _rows(), ids=lambda r: f"{'-'.join(f'{k}={v}' for k, v in r[0].items())}-{r[1]}")
def test_refusals_and_their_codes(row):
    over, code = row
    args = dict(OK_ARGS)
    assert set(over) <= set(args)
    args.update(over)
    assert _lib().idh_binary_mlp_view_search_fwd(*args.values()) == code


def test_library_exports_the_new_entry_point():
    import os

    from implicit_depth_amd import _lib as L

    assert callable(_lib().idh_binary_mlp_view_search_fwd) and "idh_binary_mlp_view_search_fwd" in L.declared_symbols()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "idh.h")).read()
    assert "int idh_binary_mlp_view_search_fwd(" in header


# ---- Python-level refusals ----------------------------------------------------------------------------------------
def _hot(use_prior=False):
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from implicit_depth_amd.pipeline import HotPath

    cve = net.CVEncoder(8, [48, 64, 160, 256], [64, 128, 256, 384])
    dec = net.BDDecoderPP([24] + cve.num_ch_enc)
    return HotPath(CostVolumeManager(16, 24, 8), cve, dec, net.BinaryMLPNetwork(dec.num_ch_dec, use_prior=use_prior))


EYE = torch.eye(4)[None]


def test_query_view_depths_refusals():
    from implicit_depth_amd._lib import IdhError

    hot = _hot()
    with pytest.raises(IdhError, match="no forward"):
        hot.query_view_depths(EYE, EYE, EYE, EYE, size=(4, 4))
    hot._last = {"ent": None, "final": {0: None}, "B": 1}  # as after a forward that built scale 0
    with pytest.raises(IdhError, match="exactly one"):
        hot.query_view_depths(EYE, EYE, EYE, EYE)
    with pytest.raises(IdhError, match="exactly one"):
        hot.query_view_depths(EYE, EYE, EYE, EYE, size=(4, 4), rays=torch.zeros(1, 3, 2))
    with pytest.raises(IdhError, match="CPU tensor"):
        hot.query_view_depths(EYE, EYE, EYE, EYE, size=(4, 4))
    E2 = EYE.expand(2, 4, 4)
    with pytest.raises(IdhError, match="batch size"):
        hot.query_view_depths(E2, E2, E2, E2, size=(4, 4))


def test_f16x3_is_refused_and_session_needs_a_prediction():
    from implicit_depth_amd import mlp, nhwc
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    hot = _hot()
    view = nhwc.View(torch.zeros(1, 4, 4, 64), 0, 64)
    with pytest.raises(IdhError, match="exactly one"):
        mlp.view_depths(hot.binary_mlp, view, EYE, EYE, EYE, EYE)
    with pytest.raises(IdhError, match="exactly one"):
        mlp.view_depths(hot.binary_mlp, view, EYE, EYE, EYE, EYE, size=(2, 2), rays=torch.zeros(1, 3, 2))
    with pytest.raises(IdhError, match="CPU tensor"):
        mlp.view_depths(hot.binary_mlp, view, EYE, EYE, EYE, EYE, size=(2, 2))
    hot.binary_mlp.mlp_math = "f16x3"
    with pytest.raises(IdhError, match="fp32 only"):
        mlp.view_depths(hot.binary_mlp, view, EYE, EYE, EYE, EYE, size=(2, 2))
    s = StreamingSession.__new__(StreamingSession)
    s._key = None
    with pytest.raises(IdhError, match="no prediction"):
        s.depth_for_view(np.eye(4), EYE, (4, 4))
    with pytest.raises(IdhError, match="no prediction"):
        s.raycast_view(torch.zeros(1, 3, 2), np.eye(4), EYE)
