"""First-hit depth in a moving camera without a GPU: the case table and the conditions on the inputs on the fp64 chain alone
(tests/view_march_ref.py), the vectorised rule against a ray-by-ray Python loop, the sample builders, and every refusal of
idh_binary_mlp_view_march_fwd / idh_binary_mlp_view_keys_march_fwd and of their wrappers that is decided on the host."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import view_march_ref as VM

V, VS, VK, R = VM.V, VM.VS, VM.VK, VM.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SIM = {}


def _lib():
    from implicit_depth_amd import _lib as L

    return L.lib()


def _sim(case):
    """The fp64 simulation of a case and its table of every ray at every shared sample, computed once and shared."""
    if case.name not in _SIM:
        inputs = VM.case_inputs(case)
        w = R.weights64(VM.march_net(case))
        _SIM[case.name] = (inputs, w, VM.simulate(case, w, inputs), VM.sample_table(case, w, inputs))
    return _SIM[case.name]


# ---- the case table and the conditions on the inputs -------------------------------------------------------------------------
def test_case_table_covers_the_issue():
    cs, ks = VM.CASES, VM.KEYS_CASES
    a, b = VM.A, VM.B
    assert (a.B, a.H, a.W, a.h, a.w, a.camera, a.prior, a.layout, a.thr, a.zoom, a.fill, a.n_march, a.refine) == \
        (2, 12, 16, 7, 9, "moved", "map", "base1", "edge", 2.0, 7.5, 9, 6)
    assert (b.B, b.H, b.W, b.h, b.w, b.camera, b.prior, b.layout, b.fill, b.n_march, b.refine) == (2, 96, 128, 15, 16, "moved", None, "wide", 6.0, 9, 6)
    assert np.array_equal(VM.samples(a), np.linspace(0.5, 8.0, 9).astype(np.float32))  # 0.9375 apart: exact in fp32
    assert VM.A_NEG.fill == -7.5 and VM.A_NEG.name.replace("fill-7.5", "fill7.5") == a.name
    assert any(c.rays == 15 for c in cs) and any(c.cf == 128 for c in cs) and any(c.layout == "odd" for c in cs)
    assert any(c.camera == "behind" and c.fill > 0 for c in cs) and VM.LISTED.listed and VM.LISTED.N == 37
    assert any(c.n_march == 1 for c in cs) and any(c.refine == 0 for c in cs) and any(c.spacing == "inverse" for c in cs)
    assert {"clamp", "one", "edge"} <= {c.thr for c in cs}
    big = [c for c in cs if c.rays > 4096]
    assert len(big) == 1 and (big[0].h, big[0].w, big[0].n_march, big[0].refine) == (101, 163, 5, 3) and (big[0].rays + 15) // 16 == 1029
    assert any(c.M == 3 and c.pose == "pan" for c in ks) and any(c.rays == 15 for c in ks) and any(c.M == 1 for c in ks)
    assert any(c.n_slots == 4 and c.M == 3 and c.slots != tuple(sorted(c.slots)) for c in ks)
    kb = [c for c in ks if c.rays > 4096]
    assert len(kb) == 1 and (kb[0].h, kb[0].w, kb[0].M, kb[0].n_march, kb[0].refine) == (201, 245, 2, 4, 2)
    ring = next(c for c in ks if c.n_slots == 4)
    feats = VM.case_inputs(ring)[0]
    assert bool(torch.isnan(feats[3]).all())  # the slot no key names holds NaN


@pytest.mark.parametrize("case", [VM.A, VM.B], ids=lambda c: c.name)
def test_main_cases_meet_the_conditions(case):
    """On the fp64 chain alone: enough rays bracketed, without a hit, (B) hit at the first sample, and in front again after their first hit."""
    inputs, w, (mc, steps), table = _sim(case)
    br, none, first = VM.shares(mc.hit, mc.flags)
    re = VM.recross(table, mc.hit).mean()
    print(f"{case.name}: bracketed {br:.2f}, none {none:.2f}, s* = 0 {first:.2f}, re-cross {re:.2f}")
    assert br >= VM.MIN_BRACKETED and none >= VM.MIN_NONE and re >= VM.MIN_RECROSS
    if case is VM.B:
        assert first >= VM.MIN_FIRST
    rays, sure, _ = VM.decided_recross(case, w, inputs)  # what the GPU test of the first crossing is asserted on
    print(f"{case.name}: {int(rays.sum())} of {case.rays} rays cross again and are decided beyond the bounds ({sure.mean():.2f} decided)")
    assert rays.sum() >= VM.MIN_DECIDED_RECROSS * case.rays


@pytest.mark.parametrize("case", [c for c in VM.SMALL], ids=lambda c: c.name)
def test_margin_rule_of_each_case(case):
    """Per case and global step, at most NEAR_CAP of the EVALUATED probes lie within PROJ_MARGIN of a validity or prior-texel boundary."""
    inputs, w, (mc, steps), table = _sim(case)
    assert 1 <= len(steps) <= case.n_march + case.refine
    for st in steps:
        a = st["active"]
        assert a.any()
        share = (st["near"] & a).sum() / a.sum()  # of the probes evaluated at this step
        assert share <= VM.NEAR_CAP, (case.name, st["it"], share)
    assert np.isfinite(mc.sd).all() and (mc.sd >= np.float32(case.lo)).all() and (mc.sd <= np.float32(case.hi)).all()
    assert not mc.active.any()
    q_s = VM.samples(case)
    if getattr(case, "camera", None) == "behind" or getattr(case, "pose", None) == "behind":
        assert (mc.flags == 6).all() and (mc.hit == VM.NONE).all() and (mc.sd == q_s[-1]).all() and len(steps) == case.n_march
    if case is VM.A_NEG:  # "outside the keyframe's view" is a hit: most rays are done after one or two samples
        assert (mc.hit <= 1).mean() > 0.5


@pytest.mark.parametrize("case", [VM.A, VM.B, VM.A_NEG, VM.LISTED, VM.KEYS_CASES[0]], ids=lambda c: c.name)
def test_vectorised_rule_is_the_ray_by_ray_loop(case):
    inputs, w, (mc, steps), table = _sim(case)
    probe = VM.probe64(case, w, inputs)
    flat = {k: table[k].reshape(case.n_march, -1) for k in ("behind", "valid")}

    def refine_probe(q):
        p = probe(q.reshape(case.shape))
        thr = R.thresholds_at(case, p["z"].astype(np.float32))[0]
        return (p["logit"] < thr).reshape(-1), p["valid"].reshape(-1)

    depth, flags, hit = VM.brute_force(case, VM.samples(case), flat, refine_probe)
    assert np.array_equal(depth.view(np.int32), mc.sd.reshape(-1).view(np.int32))
    assert np.array_equal(flags, mc.flags.reshape(-1)) and np.array_equal(hit, mc.hit.reshape(-1))
    bracketed = (flags & 3) == 3
    q_s, hb = VM.samples(case), hit[bracketed].astype(int)
    assert (hb >= 1).all() and ((depth[bracketed] > q_s[hb - 1]) & (depth[bracketed] < q_s[hb])).all()


def test_chain64_rays_is_reused_at_pixel_centres():
    """The list form of a grid case gives the grid form's simulation: view_search_ref.chain64_rays under the march."""
    case = VM.A
    inputs, w, (mc, _), _ = _sim(case)
    listed = VM.MarchCase(case.cf, case.B, case.H, case.W, case.h, case.w, case.camera, case.prior, case.layout, case.thr, case.lo, case.hi,
                          case.fill, listed=True, list_n=case.N, zoom=case.zoom, n_march=case.n_march, refine=case.refine)
    ml, _ = VM.simulate(listed, w, inputs)
    assert np.array_equal(ml.sd, mc.sd) and np.array_equal(ml.flags, mc.flags) and np.array_equal(ml.hit, mc.hit)


def test_simulation_reproduces_the_references_modules():
    """tests/golden/view_march.npz: BackprojectDepth, Project3D, F.grid_sample and BinaryMLPNetwork from the reference's own modules inside
    the march rule.  hit_step and depth agree where the reference's smallest |logit - thr| over the evaluated probes exceeds the tolerance."""
    from conftest import TOL, load_golden

    g = load_golden("view_march")
    feat, cams = VS.golden_inputs()
    for k, t in zip(("invK", "world_T_cam", "key_cam_T_world", "key_K"), cams[:4]):
        assert np.array_equal(g[k], t.numpy()), k  # the seeds still give the generator's inputs
    fd = feat.double()
    assert np.array_equal(g["feat_chk"], np.array([fd.sum().item(), fd.abs().sum().item(), (fd * fd).sum().item()]))
    case = VM.GOLDEN_CASE
    assert np.array_equal(g["samples"], VM.samples(case)) and g["sample_margin"].shape == (case.n_march, case.B, 1, case.h, case.w)
    w = R.weights64(VM.golden_net())
    mc, _ = VM.simulate(case, w, (feat, VS.pixel_centres(case.B, case.h, case.w), cams, None))
    sure = g["march_margin"].reshape(case.shape) > TOL * float(g["logit_scale"])
    same_d, same_h = mc.sd == g["march_depths"].reshape(case.shape), mc.hit == g["hit_step"].reshape(case.shape)
    print(f"golden: {same_d.mean():.2%} of the depths equal, {sure.mean():.2%} of the rays with a margin above the tolerance")
    assert sure.mean() > 0.5 and same_d[sure].all() and same_h[sure].all()
    assert len(np.unique(mc.hit)) > 3 and len(np.unique(mc.sd)) > 8


# ---- the sample builders --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", ["linear", "inverse"])
@pytest.mark.parametrize("n,lo,hi", [(9, 0.5, 8.0), (16, 0.5, 8.0), (1, 0.7, 8.0), (2, 1.0, 3.0), (255, 0.25, 80.0), (7, 0.3, 5.1)])
def test_sample_builder_is_numpy_fp32(spacing, n, lo, hi):
    from implicit_depth_amd import mlp

    want = VM.samples(types.SimpleNamespace(n_march=n, spacing=spacing, lo=lo, hi=hi))
    got = mlp.march_samples(n, lo, hi, spacing)
    assert got.dtype == torch.float32 and got.device.type == "cpu"
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    assert got[0].item() == np.float32(lo) and (n == 1 or got[-1].item() == np.float32(hi))


def test_wrapper_rejects_bad_samples():
    from implicit_depth_amd import mlp
    from implicit_depth_amd._lib import IdhError

    for bad in ([1.0, 1.0], [2.0, 1.0], [0.0, 1.0], [-1.0, 1.0], [1.0, float("nan")], [1.0, float("inf")], [], [[1.0, 2.0]]):
        with pytest.raises(IdhError, match="march samples"):
            mlp._march_depths(torch.tensor(bad, dtype=torch.float32), 0.5, 8.0, "linear", "cpu")
    with pytest.raises(IdhError, match="march samples"):
        mlp._march_depths(torch.arange(1, 257, dtype=torch.float32), 0.5, 8.0, "linear", "cpu")
    with pytest.raises(IdhError, match="float32"):
        mlp._march_depths(torch.tensor([1.0, 2.0], dtype=torch.float64), 0.5, 8.0, "linear", "cpu")
    for n in (0, 256, -1):
        with pytest.raises(IdhError, match="1 to 255"):
            mlp.march_samples(n)
    for lo, hi in ((0.0, 8.0), (-1.0, 8.0), (2.0, 2.0), (3.0, 1.0), (float("nan"), 8.0), (0.5, float("inf"))):
        with pytest.raises(IdhError, match="0 < lo < hi"):
            mlp.march_samples(4, lo, hi)
    with pytest.raises(IdhError, match="spacing"):
        mlp.march_samples(4, spacing="log")
    for bad in ([0.5, 1.0], np.array([0.5, 1.0], dtype=np.float32), 4.0, "4", True, None):
        with pytest.raises(IdhError, match="float32 tensor or an integer"):
            mlp._march_depths(bad, 0.5, 8.0, "linear", "cpu")
    for i in range(3 * mlp._MARCH_CACHE_MAX):  # a caller sweeping the range does not grow the table of uploaded settings
        mlp._march_depths(4, 0.5, 8.0 + i, "linear", "cpu")
    assert len(mlp._march_cache) <= mlp._MARCH_CACHE_MAX
    good = mlp._march_depths(torch.tensor([0.5, 1.0, 4.0]), 0.5, 8.0, "linear", "cpu")
    assert good.tolist() == [0.5, 1.0, 4.0]


# ---- refusals, decided before the device is touched -----------------------------------------------------------------------
P = 0x1000  # a non-null, 16-byte-aligned address that is never dereferenced: every call below must return before any launch
OK_ARGS = dict(feat=P, feat_cs=64, Cf=64, B=2, H=5, W=7, h=3, w=4, rays=None, N=0, invK=P, world_T_cam=P, key_cam_T_world=P, key_K=P, prior_pred=None,
               prior_cam_T_world=None, prior_K=None, has_prior=0, prior_const=0.0, w1f=P, w2=P, vecs=P, march_depths=P, n_march=9, refine=6,
               threshold=0.5, bins=None, thr_logits=None, n_bins=0, fill=0.0, depth=P, last_logits=P, flags=None, hit_step=None, points=None,
               stream=None)
SLOTS3 = (0, 1, 2)
KEYS_EXTRA = dict(key_stride=1 << 50, n_slots=3, key_slots=SLOTS3, M=3)
NAN = float("nan")


def _rows():
    rs = []
    add = lambda code, **kw: rs.append((kw, code))
    # the march's own
    for n in (0, -1, 256, 1 << 20):
        add(V.EINVAL, n_march=n)
    add(V.EINVAL, refine=-1)
    add(V.EINVAL, march_depths=None)
    add(V.EINVAL, march_depths=P + 2)
    add(V.EINVAL, B=0, march_depths=None)  # as a NULL Thresholder table: an argument error is reported even where nothing would be launched
    add(V.OK, B=0)
    add(V.OK, n_march=1, refine=0, B=0)
    add(V.OK, n_march=255, refine=0, h=0)
    # which rule wins: shapes, the march, the thresholds and the prior rule, then the empty call, then the pointers, then the sizes
    add(V.EUNSUPPORTED, refine=(1 << 30) + 1)
    add(V.EUNSUPPORTED, refine=(1 << 30) + 1, threshold=0.0)
    add(V.EUNSUPPORTED, refine=(1 << 30) + 1, B=0)
    add(V.EINVAL, refine=(1 << 30) + 1, n_bins=-1)
    add(V.EINVAL, refine=(1 << 30) + 1, n_march=0)
    add(V.EINVAL, B=0, threshold=0.0)
    add(V.EINVAL, h=0, prior_pred=P, prior_cam_T_world=P, prior_K=P, has_prior=0)
    add(V.OK, h=0, B=129)
    add(V.OK, w=0, depth=P + 2)
    add(V.EINVAL, feat=None, B=129)
    add(V.EINVAL, points=P + 2, B=8, h=1 << 14, w=1 << 14)
    # the parents' that apply
    for k in ("feat", "invK", "world_T_cam", "key_cam_T_world", "key_K", "w1f", "w2", "vecs", "depth", "last_logits"):
        add(V.EINVAL, **{k: None})
    for k in ("B", "h", "w"):
        add(V.EINVAL, **{k: -1})
        add(V.OK, **{k: 0})
        add(V.OK, **{k: 0, "feat": None, "depth": None})
    add(V.EINVAL, rays=P, N=-1)
    add(V.OK, rays=P, N=0, feat=None)
    add(V.EINVAL, rays=P, N=5, h=-1, w=-1, feat=None)
    add(V.EINVAL, rays=P + 2, N=5)
    for k in ("H", "W", "Cf"):
        add(V.EINVAL, **{k: 0})
        add(V.EINVAL, **{k: -3})
    add(V.EINVAL, Cf=62)
    add(V.EINVAL, feat_cs=60)
    for k in ("feat", "invK", "world_T_cam", "key_cam_T_world", "key_K", "depth", "last_logits", "points"):
        add(V.EINVAL, **{k: P + 2})
    prior = dict(prior_pred=P, prior_cam_T_world=P, prior_K=P, has_prior=1)
    for k in ("prior_cam_T_world", "prior_K"):
        add(V.EINVAL, **dict(prior, **{k: None}))
    add(V.EINVAL, **dict(prior, has_prior=0))
    add(V.EINVAL, **dict(prior, prior_pred=P + 2))
    add(V.EINVAL, n_bins=-1)
    for t in (0.0, 1.0, -0.1, NAN):
        add(V.EINVAL, threshold=t)
    add(V.EINVAL, n_bins=3, bins=None, thr_logits=P)
    add(V.EINVAL, n_bins=3, bins=P, thr_logits=None)
    add(V.EINVAL, n_bins=3, bins=P + 2, thr_logits=P)
    add(V.EUNSUPPORTED, B=8, h=1 << 14, w=1 << 14)
    add(V.EUNSUPPORTED, B=1, h=1 << 16, w=1 << 16)
    add(V.EUNSUPPORTED, B=4, rays=P, N=1 << 29)
    add(V.EUNSUPPORTED, B=1 << 12, H=1 << 10, W=1 << 10)
    add(V.EUNSUPPORTED, B=129)
    return rs


def _keys_rows():
    rs = []
    add = lambda code, **kw: rs.append((kw, code))
    add(V.EINVAL, key_slots=None)
    add(V.EINVAL, M=0)
    add(V.EINVAL, n_slots=0)
    add(V.EINVAL, key_stride=-1)
    add(V.EINVAL, key_stride=2 * 5 * 7 * 64 - 1)
    add(V.EINVAL, key_slots=(0, 1, 3))
    add(V.EINVAL, key_slots=(0, 1, 1))
    add(V.EINVAL, key_slots=(0, -1, 1))
    add(V.EUNSUPPORTED, key_slots=tuple(range(17)), M=17, n_slots=17)
    add(V.EUNSUPPORTED, key_slots=tuple(range(16)), M=16, n_slots=16, B=9)  # M * B > 128
    add(V.OK, key_slots=None, B=0)
    add(V.EINVAL, key_slots=None, B=129)  # the keys are looked at before the sizes ...
    add(V.EINVAL, key_slots=tuple(range(17)), M=17, n_slots=17, feat=P + 2)  # ... and after the pointers
    add(V.EUNSUPPORTED, key_slots=None, refine=(1 << 30) + 1)
    return rs


def _id(r):
    return f"{'-'.join(f'{k}={v}' for k, v in r[0].items())}-{r[1]}"[:120]


@pytest.mark.parametrize("row", _rows(), ids=_id)
def test_refusals_and_their_codes(row):
    over, code = row
    args = dict(OK_ARGS)
    assert set(over) <= set(args)
    args.update(over)
    assert _lib().idh_binary_mlp_view_march_fwd(*args.values()) == code
    assert _keys_call(args, {}) == code  # the multi-key entry point refuses the same, with the same code


def _keys_call(args, over):
    import ctypes as C

    a = dict(args)
    extra = dict(KEYS_EXTRA)
    extra.update({k: over[k] for k in over if k in extra})
    a.update({k: over[k] for k in over if k in a})
    ks = extra["key_slots"]
    slots = None if ks is None else (C.c_int * len(ks))(*ks)
    vals = list(a.values())
    head, tail = vals[:6], vals[6:-1]  # (feat .. W), (h .. points)
    return _lib().idh_binary_mlp_view_keys_march_fwd(*head, extra["key_stride"], extra["n_slots"], slots, extra["M"], *tail, None, a["stream"])


@pytest.mark.parametrize("row", _keys_rows(), ids=_id)
def test_keys_refusals_and_their_codes(row):
    over, code = row
    assert _keys_call(dict(OK_ARGS), over) == code


def test_library_exports_both_entry_points():
    from implicit_depth_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "idh.h")).read()
    for name in ("idh_binary_mlp_view_march_fwd", "idh_binary_mlp_view_keys_march_fwd"):
        assert callable(getattr(_lib(), name)) and name in L.declared_symbols() and f"int {name}(" in header


def test_ray_kernels_use_no_scratch():
    """Both new kernels and the six they share ray_body with stay spill-free (tools/kernel_resources.py, as test_abi.py runs it)."""
    names = ("ray_mlp_k", "ray_search_k", "view_mlp_k", "view_search_k", "view_keys_k", "view_keys_search_k", "view_march_k", "view_keys_march_k")
    src = os.path.join(ROOT, "implicit-depth_amd", "csrc", "mlp_rays.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), src, "--max-scratch"] + [f"{n}=0" for n in names],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()[1:] if ln.split()}
    for n in names:
        assert n in rows and int(rows[n][4]) == 0, (n, rows.get(n))


# ---- Python-level refusals ----------------------------------------------------------------------------------------
EYE = torch.eye(4)[None]


def _hot():
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from implicit_depth_amd.pipeline import HotPath

    cve = net.CVEncoder(8, [48, 64, 160, 256], [64, 128, 256, 384])
    dec = net.BDDecoderPP([24] + cve.num_ch_enc)
    return HotPath(CostVolumeManager(16, 24, 8), cve, dec, net.BinaryMLPNetwork(dec.num_ch_dec))


def test_public_refusals():
    from implicit_depth_amd import mlp, nhwc
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    hot = _hot()
    with pytest.raises(IdhError, match="no forward"):
        hot.query_view_first_hit(EYE, EYE, EYE, EYE, size=(4, 4))
    with pytest.raises(IdhError, match="nothing is remembered"):
        hot.query_view_first_hit_keys(EYE, EYE, size=(4, 4))
    hot._last = {"ent": None, "final": {0: None}, "B": 1}  # as after a forward that built scale 0
    for call in (lambda **k: hot.query_view_first_hit(EYE, EYE, EYE, EYE, **k), lambda **k: hot.query_view_first_hit_keys(EYE, EYE, **k)):
        with pytest.raises(IdhError, match="exactly one"):
            call()
        with pytest.raises(IdhError, match="exactly one"):
            call(size=(4, 4), rays=torch.zeros(1, 3, 2))
    with pytest.raises(IdhError, match="CPU tensor"):
        hot.query_view_first_hit(EYE, EYE, EYE, EYE, size=(4, 4))
    E2 = EYE.expand(2, 4, 4)
    with pytest.raises(IdhError, match="batch size"):
        hot.query_view_first_hit(E2, E2, E2, E2, size=(4, 4))
    view = nhwc.View(torch.zeros(1, 4, 4, 64), 0, 64)
    with pytest.raises(IdhError, match="exactly one"):
        mlp.view_march_depths(hot.binary_mlp, view, EYE, EYE, EYE, EYE)
    with pytest.raises(IdhError, match="refine"):
        mlp.view_march_depths(hot.binary_mlp, view, EYE, EYE, EYE, EYE, size=(2, 2), refine=-1)
    with pytest.raises(IdhError, match="CPU tensor"):
        mlp.view_march_depths(hot.binary_mlp, view, EYE, EYE, EYE, EYE, size=(2, 2))
    hot.binary_mlp.mlp_math = "f16x3"
    with pytest.raises(IdhError, match="fp32 only"):
        mlp.view_march_depths(hot.binary_mlp, view, EYE, EYE, EYE, EYE, size=(2, 2))
    with pytest.raises(IdhError, match="fp32 only"):
        mlp.view_keys_march_depths(hot.binary_mlp, torch.zeros(1, 1, 4, 4, 64), 0, 64, [0], EYE, EYE, EYE[None], EYE[None], size=(2, 2))
    s = StreamingSession.__new__(StreamingSession)
    s._key = None
    with pytest.raises(IdhError, match="no prediction"):
        s.first_hit_for_view(np.eye(4), EYE, (4, 4))
    with pytest.raises(IdhError, match="no prediction"):
        s.raycast_first_hit(torch.zeros(1, 3, 2), np.eye(4), EYE)
