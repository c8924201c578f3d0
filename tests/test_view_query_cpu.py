"""Dense occlusion in a moving camera without a GPU: the 1 % cap on the pixels the margin rule leaves out (on the float64 reference alone),
the fp64 restatement against the reference's own modules (tests/golden/view_query.npz), the derived bound against mutants, and every
refusal of idh_binary_mlp_view_fwd, mlp.view_logits, HotPath.query_view and StreamingSession.occlusion_for_view that is decided on the host."""
import numpy as np
import pytest
import torch

import view_query_ref as V
from conftest import TOL, load_golden

Q, R = V.Q, V.R
SMALL = [c for c in V.VIEW_CASES if c not in V.LARGE]


def _lib():
    from implicit_depth_amd import _lib as L

    return L.lib()


def _const(case):
    return float(case.prior) if isinstance(case.prior, float) else None


# ---- the case table and the margin rule, on the reference alone -----------------------------------------------------------
def test_case_table_covers_the_issue():
    cs = V.VIEW_CASES
    assert {(c.H, c.W) for c in cs} == {(12, 16), (24, 32)} and {c.cf for c in cs} == {64, 128}
    assert {c.layout for c in cs} == set(Q.LAYOUTS) and {c.camera for c in cs} == set(V.CAMERAS)
    assert {c.prior for c in cs} == {None, "map", -1.0}
    assert (2, 3, 7, 9) in {(c.B, c.P, c.h, c.w) for c in cs} and (1, 1, 5, 3) in {(c.B, c.P, c.h, c.w) for c in cs}
    assert any(c.rays % 16 for c in cs) and any((c.h * c.w) % 16 and c.B * c.P > 1 for c in cs)  # tiles straddle plane and batch boundaries
    assert any((c.h, c.w) != (c.H, c.W) and c.camera == "own" for c in cs)
    assert len(V.LARGE) == 1 and V.LARGE[0].rays > 49152 and (V.LARGE[0].rays + 15) // 16 > Q.LAUNCHED_WAVES


@pytest.mark.parametrize("case", V.VIEW_CASES, ids=lambda c: c.name)
def test_margin_rule_leaves_out_at_most_one_percent(case):
    """The share of pixels within PROJ_MARGIN of a validity or rounding boundary, the fp32 chain's error against that margin, and the
    mix of pixels each camera promises - all from the float64 chain."""
    feat, rendered, cams, prior = V.case_inputs(case)
    ch = V.chain64(rendered, cams, case.H, case.W, prior)
    share = ch["near"].double().mean().item()
    print(f"{case.name}: {share:.4f} of {case.rays} pixels within the margin, {ch['valid'].double().mean().item():.3f} valid")
    assert share <= V.NEAR_CAP, (case.name, share)
    front = ch["dok"] & (ch["cz"] > 0)
    # the fp32 chain cannot carry a pixel that is kept across a boundary: its error is below the margin
    assert float(ch["e_cz"].max()) < V.PROJ_MARGIN / 2
    if front.any():
        assert float(ch["e_uv"][front].max()) < V.PROJ_MARGIN / 2
    if prior is not None:
        pu, pv = ch["prior_uv"][..., 0], ch["prior_uv"][..., 1]  # (a projection more than a texel outside the prior map is -1 on both sides)
        pf = ch["valid"] & (ch["prior_cz"] > 0) & (pu > -1) & (pu < case.W + 1) & (pv > -1) & (pv < case.H + 1)
        assert float(ch["e_prior_cz"].max()) < V.PROJ_MARGIN / 2 and (not pf.any() or float(ch["e_prior_uv"][pf].max()) < V.PROJ_MARGIN / 2)
    d = rendered.view(case.B, -1)
    assert (d == 0).any() and (d < 0).any() and torch.isinf(d).any() and torch.isnan(d).any()  # holes, negative, inf, NaN
    assert not ch["valid"][~ch["dok"]].any()
    u, v = ch["uv"][..., 0], ch["uv"][..., 1]
    if case.camera == "behind":
        assert not ch["valid"].any() and (ch["cz"][ch["dok"]] < 0).all()
    elif case.camera == "identity":
        assert torch.equal(ch["valid"], ch["dok"])
    else:
        out = front & ((u < 0) | (u >= case.W) | (v < 0) | (v >= case.H))
        assert ch["valid"].any() and (out.any() or case.rays < 64)  # part of the view leaves the keyframe's image
    if case.prior == "map" and ch["valid"].any():
        assert (ch["prior"][ch["valid"]] >= 0).any()
    if case.prior == "map" and case.camera == "moved":
        assert (ch["prior"][ch["valid"]] == -1).any()


# ---- the restatement against the reference's modules ------------------------------------------------------------------------
def test_restatement_reproduces_the_reference():
    g = load_golden("view_query")
    w = R.weights64(Q.golden_net())
    for cam in V.GOLDEN_CAMERAS:
        feat, rendered, cams = V.golden_inputs(cam)
        for k, t in zip(("rendered", "invK", "world_T_cam", "key_cam_T_world", "key_K"), (rendered,) + cams[:4]):
            assert np.array_equal(g[f"{cam}_{k}"], t.numpy()), (cam, k)  # the seeds still give the generator's inputs
        ref, ch = V.reference(w, feat, rendered, cams)
        keep = (ch["valid"] & ~ch["near"]).view(rendered.shape)
        assert ch["near"].double().mean().item() <= V.NEAR_CAP and keep.double().mean().item() > 0.25
        gold = torch.from_numpy(g[f"{cam}_pred"]).double()
        err = ((ref - gold).abs()[keep].max() / gold[keep].abs().max()).item()
        print(f"{cam}: fp64 restatement vs the reference's fp32 modules on {int(keep.sum())} pixels, scale-relative error {err:.3g}")
        assert err < TOL


MUTANTS = ("no_half_pixel", "transposed_pose")


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_bound_discriminates(mutant):
    """A mutant of the chain, evaluated in float64, leaves the bound on at least half of the valid pixels: pixel corners instead of
    centres, and the view pose's rotation transposed."""
    for case in SMALL:
        if case.camera in ("behind", "identity"):
            continue
        feat, rendered, cams, prior = V.case_inputs(case)
        w = R.weights64(R.make_net(case.cf, case.has_prior, R._seed(case.name), depth_gain=4.0))
        ref, ch = V.reference(w, feat, rendered, cams, prior, _const(case))
        logit, tol = V.view_bound(w, feat, ch, _const(case))
        keep = ch["valid"] & ~ch["near"]
        assert (logit - ref.view(case.B, -1))[ch["valid"]].abs().max() < 1e-12 * (1 + logit.abs().max())  # the bound's logits are the restatement's
        if mutant == "no_half_pixel":
            iK = cams[0].double().clone()
            iK[:, :3, 2] -= 0.5 * (iK[:, :3, 0] + iK[:, :3, 1])  # invK (x - 0.5, y - 0.5, 1)
            mch = V.chain64(rendered, (iK.float(),) + tuple(cams[1:]), case.H, case.W, prior)
        else:
            T = cams[1].clone()
            T[:, :3, :3] = T[:, :3, :3].transpose(1, 2)
            mch = V.chain64(rendered, (cams[0], T) + tuple(cams[2:]), case.H, case.W, prior)
        mut, _ = V.view_bound(w, feat, mch, _const(case))
        caught = ((mut - logit).abs() > tol)[keep].double().mean().item()
        print(f"{case.name}: {mutant} caught on {caught:.2f} of {int(keep.sum())} kept pixels")
        assert caught >= 0.5, (case.name, mutant, caught)


# ---- refusals, decided before the device is touched -----------------------------------------------------------------------
P = 0x1000  # a non-null, 16-byte-aligned address that is never dereferenced: every call below must return before any launch
VIEW_OK = dict(feat=P, feat_cs=64, Cf=64, B=2, H=5, W=7, rendered=P, P=2, h=3, w=4, invK=P, world_T_cam=P, key_cam_T_world=P, key_K=P, prior_pred=None,
               prior_cam_T_world=None, prior_K=None, has_prior=0, prior_const=0.0, w1f=P, w2=P, vecs=P, fill=0.0, logits=P, valid=None, view_depth=None,
               view_points=None, stream=None)


def _rows():
    rs = []
    add = lambda code, **kw: rs.append((kw, code))
    for k in ("feat", "rendered", "invK", "world_T_cam", "key_cam_T_world", "key_K", "w1f", "w2", "vecs", "logits"):
        add(V.EINVAL, **{k: None})
    for k in ("B", "P", "h", "w"):
        add(V.EINVAL, **{k: -1})
        add(V.OK, **{k: 0})
        add(V.OK, **{k: 0, "feat": None, "logits": None})  # B == 0 or an empty map: no launch, nothing is read
    for k in ("H", "W", "Cf"):
        add(V.EINVAL, **{k: 0})
        add(V.EINVAL, **{k: -3})
    add(V.EINVAL, Cf=62)  # Cf % 4
    add(V.EINVAL, feat_cs=60)  # feat_cs < Cf
    for k in ("feat", "rendered", "invK", "world_T_cam", "key_cam_T_world", "key_K", "logits", "view_depth", "view_points"):
        add(V.EINVAL, **{k: P + 2})  # not 4-byte aligned
    prior = dict(prior_pred=P, prior_cam_T_world=P, prior_K=P, has_prior=1)
    for k in ("prior_cam_T_world", "prior_K"):
        add(V.EINVAL, **dict(prior, **{k: None}))
    add(V.EINVAL, **dict(prior, has_prior=0))  # a prior map for a network without a prior column
    add(V.EINVAL, **dict(prior, prior_pred=P + 2))
    add(V.EUNSUPPORTED, B=8, P=1 << 8, h=1 << 10, w=1 << 10)  # B * P * h * w >= 2^31
    add(V.EUNSUPPORTED, B=1 << 12, H=1 << 10, W=1 << 10)  # B * H * W >= 2^31
    add(V.EUNSUPPORTED, B=129)  # the cameras of one launch sit in LDS
    # which rule wins: shapes and the prior rule, then the empty call, then the pointers, then the sizes
    add(V.EINVAL, B=0, Cf=62)
    add(V.EINVAL, **dict(prior, has_prior=0, h=0))
    add(V.OK, w=0, B=129)
    add(V.OK, P=0, rendered=P + 2)
    add(V.OK, P=1 << 16, h=1 << 16, w=0)
    add(V.EINVAL, feat=None, B=129)
    add(V.EINVAL, logits=P + 2, B=1, P=1 << 16, h=1 << 16)
    add(V.EINVAL, H=0, B=129)
    return rs


@pytest.mark.parametrize("row", _rows(), ids=lambda r: f"{'-'.join(f'{k}={v}' for k, v in r[0].items())}-{r[1]}")
def test_refusals_and_their_codes(row):
    over, code = row
    args = dict(VIEW_OK)
    assert set(over) <= set(args)
    args.update(over)
    assert _lib().idh_binary_mlp_view_fwd(*args.values()) == code


def test_library_exports_the_new_entry_point():
    from implicit_depth_amd import _lib as L

    assert callable(_lib().idh_binary_mlp_view_fwd) and "idh_binary_mlp_view_fwd" in L.declared_symbols()


# ---- Python-level refusals ----------------------------------------------------------------------------------------
def _hot(use_prior=False):
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from implicit_depth_amd.pipeline import HotPath

    cve = net.CVEncoder(8, [48, 64, 160, 256], [64, 128, 256, 384])
    dec = net.BDDecoderPP([24] + cve.num_ch_enc)
    return HotPath(CostVolumeManager(16, 24, 8), cve, dec, net.BinaryMLPNetwork(dec.num_ch_dec, use_prior=use_prior))


EYE = torch.eye(4)[None]


def test_query_view_before_a_forward_cpu_tensors_and_wrong_batch():
    from implicit_depth_amd._lib import IdhError

    hot = _hot()
    with pytest.raises(IdhError, match="no forward"):
        hot.query_view(torch.ones(1, 1, 4, 4), EYE, EYE, EYE, EYE)
    hot._last = {"ent": None, "final": {0: None}, "B": 1}  # as after a forward that built scale 0
    with pytest.raises(IdhError, match="CPU tensor"):
        hot.query_view(torch.ones(1, 1, 4, 4), EYE, EYE, EYE, EYE)
    with pytest.raises(IdhError, match="batch size"):
        hot.query_view(torch.ones(2, 1, 4, 4), EYE.expand(2, 4, 4), EYE.expand(2, 4, 4), EYE.expand(2, 4, 4), EYE.expand(2, 4, 4))


def test_f16x3_is_refused_and_session_needs_a_prediction():
    from implicit_depth_amd import mlp, nhwc
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    hot = _hot()
    hot.binary_mlp.mlp_math = "f16x3"
    view = nhwc.View(torch.zeros(1, 4, 4, 64), 0, 64)
    with pytest.raises(IdhError, match="fp32 only"):
        mlp.view_logits(hot.binary_mlp, view, torch.ones(1, 1, 4, 4), EYE, EYE, EYE, EYE)
    s = StreamingSession.__new__(StreamingSession)
    s._key = None
    with pytest.raises(IdhError, match="no prediction"):
        s.occlusion_for_view(torch.ones(1, 1, 4, 4), np.eye(4), EYE)


def test_view_logits_refuses_cpu_tensors_before_anything_else():
    from implicit_depth_amd import mlp, nhwc
    from implicit_depth_amd._lib import IdhError

    hot = _hot()
    view = nhwc.View(torch.zeros(1, 4, 4, 64), 0, 64)
    with pytest.raises(IdhError, match="CPU tensor"):
        mlp.view_logits(hot.binary_mlp, view, torch.ones(1, 1, 4, 4), EYE, EYE, EYE, EYE)
