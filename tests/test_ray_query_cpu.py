"""Sparse occlusion queries without a GPU: the fp64 restatement against the reference's own run_mlp_train (tests/golden/ray_query.npz), the
derived bound against three mutants, ray_step against the reference's slicing, and every refusal of idh_binary_mlp_rays_fwd /
idh_project_points_fwd and of HotPath.query_rays / query_points that is decided on the host."""
import numpy as np
import pytest
import torch

import ray_query_ref as Q
from conftest import TOL, load_golden, rel_err

SMALL = [c for c in Q.RAY_CASES if not c.large]


def _lib():
    from implicit_depth_amd import _lib as L

    return L.lib()


@pytest.fixture(scope="module")
def golden():
    g = load_golden("ray_query")
    feats, rays, depths = Q.golden_inputs()
    assert np.array_equal(g["rays"], rays.numpy()) and np.array_equal(g["depths"], depths.numpy())  # the seeds still give the generator's inputs
    return g, feats, rays, depths, Q.R.weights64(Q.golden_net())


def test_restatement_reproduces_the_reference(golden):
    g, feats, rays, depths, w = golden
    for s in range(4):
        ref = Q.reference(w, feats[s], rays, depths, None, Q.GOLDEN_GRID, step=s + 1, scale=s)
        assert g[f"pred_{s}"].shape == (Q.GOLDEN_B, 1, (Q.GOLDEN_N + s) // (s + 1), Q.GOLDEN_S)
        err = rel_err(ref.unsqueeze(1), g[f"pred_{s}"])
        print(f"pred_{s}: fp64 restatement vs reference fp32, scale-relative error {err:.3g}")
        assert err < TOL


def test_golden_rays_reach_outside_the_grid(golden):
    _, _, rays, _, _ = golden
    gh, gw = Q.GOLDEN_GRID
    assert rays[..., 0].min() < -1 and rays[..., 0].max() > gw + 1 and rays[..., 1].min() < -1 and rays[..., 1].max() > gh + 1


def test_ray_step_is_the_references_slicing(golden):
    g, feats, rays, depths, w = golden
    for s in range(1, 4):
        full = Q.reference(w, feats[s], rays, depths, None, Q.GOLDEN_GRID, step=1, scale=s)
        stepped = Q.reference(w, feats[s], rays, depths, None, Q.GOLDEN_GRID, step=s + 1, scale=s)
        assert torch.equal(full[:, ::s + 1], stepped)
        assert stepped.shape[1] == g[f"pred_{s}"].shape[2] == -(-Q.GOLDEN_N // (s + 1))
        assert rel_err(full[:, ::s + 1].unsqueeze(1), g[f"pred_{s}"]) < TOL


def test_case_table_covers_the_issue():
    cs = Q.RAY_CASES
    assert {(c.H, c.W) for c in cs} == {(5, 7), (12, 16)}
    assert {c.cf for c in cs} == {4, 20, 64, 68, 128, 256}
    assert {c.B for c in cs} == {1, 3} and {c.N for c in SMALL} == {1, 15, 16, 17, 37} and {c.S for c in cs} == {1, 3}
    assert {c.step for c in cs} == {1, 2, 3, 4} and {c.prior for c in cs} == {None, "tensor", -1.0}
    assert {c.layout for c in cs} == {"wide", "base1", "odd"} and {c.grid_mul for c in cs} == {1, 2}
    big = [c for c in cs if c.large]
    assert len(big) == 1 and big[0].S == 1 and (big[0].B * big[0].N + 15) // 16 > Q.LAUNCHED_WAVES


@pytest.mark.parametrize("case", [c for c in SMALL if c.N >= 15], ids=lambda c: c.name)
def test_case_rays_mix_every_kind(case):
    """The float64 sample coordinates of the case's fp32 rays are of the kinds the table promises."""
    rays = Q.case_rays(case)
    gh, gw = case.grid
    ix = rays[..., 0].double() * case.W / gw - 0.5
    iy = rays[..., 1].double() * case.H / gh - 0.5
    kind = np.array(Q.KINDS)[np.arange(case.N) % len(Q.KINDS)]
    sel = lambda k: torch.from_numpy(kind == k).expand(case.B, case.N)
    assert (ix[sel("centre")] == torch.round(ix[sel("centre")])).all() and (iy[sel("centre")] == torch.round(iy[sel("centre")])).all()
    assert (rays[..., 0][sel("edge0")] == 0).all() and (rays[..., 0][sel("edgeW")] == gw).all()
    assert ((ix[sel("band1")] > -0.5) & (ix[sel("band1")] < 0)).all()
    assert ((ix[sel("band2")] < 0) & (iy[sel("band2")] < 0) & (ix[sel("band2")] > -0.5) & (iy[sel("band2")] > -0.5)).all()
    assert ((ix[sel("far")] < -1.5) | (ix[sel("far")] > case.W + 0.5)).all()
    assert (ix[sel("cell")] == torch.round(ix[sel("cell")])).all() and Q.corners_in_range(case, rays, case.grid)[sel("cell")].all()
    assert Q.corners_in_range(case, rays, case.grid)[sel("generic")].all()
    feat = torch.ones(case.B, 1, case.H, case.W)
    assert (Q.sample64(feat, rays, case.grid)[:, 0][sel("far")] == 0).all()


MUTANTS = {"align_corners": dict(align_corners=True), "nearest": dict(mode="nearest"), "shift": None}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_bound_discriminates(mutant):
    """Each mutant of the sampling, evaluated in float64, leaves the bound on at least half of the rays whose four corners are in range."""
    for case in SMALL:
        feat, rays, depths, prior = Q.case_inputs(case)
        w = Q.R.weights64(Q.R.make_net(case.cf, case.has_prior, Q.R._seed(case.name)))
        p = prior if prior is not None else case.prior
        ref, tol = Q.ray_bound(w, feat, rays, depths, p, case.grid, case.step)
        if mutant == "shift":
            m = case.grid_mul  # half a pixel of the MAP
            mut = Q.reference(w, feat, rays + 0.5 * m, depths, p, case.grid, case.step)
        else:
            mut = Q.reference(w, feat, rays, depths, p, case.grid, case.step, **MUTANTS[mutant])
        inr = Q.corners_in_range(case, rays[:, ::case.step], case.grid)
        assert inr.any(), case.name
        caught = ((mut - ref).abs() > tol).any(-1)  # any depth sample of the ray
        share = caught[inr].double().mean().item()
        print(f"{case.name}: {mutant} caught on {share:.2f} of {int(inr.sum())} in-range rays")
        assert share >= 0.5, (case.name, share)
        # the bound's own logits are the restatement's (the layer-1 sum is split there: float64 rounding only)
        assert (Q.reference(w, feat, rays, depths, p, case.grid, case.step) - ref).abs().max() < 1e-12 * (1 + ref.abs().max())


# ---- refusals, decided before the device is touched --------------------------------------------------------------
P = 0x1000  # a non-null, 16-byte-aligned address that is never dereferenced: every call below must return before any launch
RAYS_OK = dict(feat=P, feat_cs=64, Cf=64, B=2, H=5, W=7, rays=P, depth=P, prior=None, has_prior=0, prior_const=0.0, N=9, S=3, ray_step=1, grid_w=7,
               grid_h=5, w1f=P, w2=P, vecs=P, out=P, stream=None)
PROJ_OK = dict(points=P, cam_T_world=P, K=P, B=2, N=9, H=5, W=7, rays=P, depth=P, valid=P, prior_pred=None, prior_cam_T_world=None, prior_K=None,
               prior=None, stream=None)


def _rows():
    rs = []
    add = lambda fn, code, **kw: rs.append((fn, kw, code))
    for k in ("feat", "rays", "depth", "w1f", "w2", "vecs", "out"):
        add("rays", Q.EINVAL, **{k: None})
    for k in ("B", "N"):
        add("rays", Q.EINVAL, **{k: -1})
        add("rays", Q.OK, **{k: 0})
        add("rays", Q.OK, **{k: 0, "feat": None, "out": None})  # zero-size: no launch, nothing is read
    for k in ("S", "H", "W", "Cf", "grid_w", "grid_h"):
        add("rays", Q.EINVAL, **{k: 0})
        add("rays", Q.EINVAL, **{k: -3})
    add("rays", Q.EINVAL, ray_step=0)
    add("rays", Q.EINVAL, ray_step=-1)
    add("rays", Q.EINVAL, Cf=62)  # Cf % 4
    add("rays", Q.EINVAL, feat_cs=60)  # feat_cs < Cf
    for k in ("depth", "out", "rays", "feat", "prior"):
        add("rays", Q.EINVAL, **{k: P + 2})  # not 4-byte aligned
    add("rays", Q.EUNSUPPORTED, B=1 << 16, N=1 << 16)  # B * Nq >= 2^31
    add("rays", Q.EUNSUPPORTED, B=1 << 12, H=1 << 10, W=1 << 10)  # B * H * W >= 2^31
    add("rays", Q.EUNSUPPORTED, B=1 << 10, N=1 << 20, S=1 << 20)  # B * Nq fits, the work items of the launch do not
    # which rule wins: shapes, then the empty call, then the pointers, then the sizes
    add("rays", Q.EINVAL, B=0, Cf=62)
    add("rays", Q.EINVAL, N=0, S=0)
    add("rays", Q.OK, B=0, rays=P + 2)
    add("rays", Q.OK, N=0, B=1 << 12, H=1 << 10, W=1 << 10)
    add("rays", Q.EINVAL, feat=None, B=1 << 16, N=1 << 16)
    add("rays", Q.EINVAL, out=P + 2, B=1 << 12, H=1 << 10, W=1 << 10)
    add("rays", Q.EINVAL, ray_step=0, B=1 << 16, N=1 << 16)
    for k in ("points", "cam_T_world", "K", "rays", "depth", "valid"):
        add("proj", Q.EINVAL, **{k: None})
    for k in ("B", "N"):
        add("proj", Q.EINVAL, **{k: -1})
        add("proj", Q.OK, **{k: 0})
    for k in ("H", "W"):
        add("proj", Q.EINVAL, **{k: 0})
    add("proj", Q.EINVAL, B=65536)
    for k in ("prior_cam_T_world", "prior_K", "prior"):
        add("proj", Q.EINVAL, **dict(dict(prior_pred=P, prior_cam_T_world=P, prior_K=P, prior=P), **{k: None}))
    return rs


REFUSALS = _rows()


@pytest.mark.parametrize("row", REFUSALS, ids=lambda r: f"{r[0]}-{'-'.join(f'{k}={v}' for k, v in r[1].items())}-{r[2]}")
def test_refusals_and_their_codes(row):
    fn, over, code = row
    args = dict(RAYS_OK if fn == "rays" else PROJ_OK)
    assert set(over) <= set(args)
    args.update(over)
    f = _lib().idh_binary_mlp_rays_fwd if fn == "rays" else _lib().idh_project_points_fwd
    assert f(*args.values()) == code


def test_library_exports_the_new_entry_points():
    """Additive entry points: idh_version() is unchanged, the binding resolves both by name when it loads the library."""
    from implicit_depth_amd import _lib as L

    assert callable(_lib().idh_binary_mlp_rays_fwd) and callable(_lib().idh_project_points_fwd)
    assert {"idh_binary_mlp_rays_fwd", "idh_project_points_fwd"} <= set(L.declared_symbols())


# ---- Python-level refusals ----------------------------------------------------------------------------------------
def _hot(use_prior=False):
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from implicit_depth_amd.pipeline import HotPath

    cve = net.CVEncoder(8, [48, 64, 160, 256], [64, 128, 256, 384])
    dec = net.BDDecoderPP([24] + cve.num_ch_enc)
    return HotPath(CostVolumeManager(16, 24, 8), cve, dec, net.BinaryMLPNetwork(dec.num_ch_dec, use_prior=use_prior))


def test_queries_before_a_forward_raise():
    from implicit_depth_amd._lib import IdhError

    hot = _hot()
    with pytest.raises(IdhError, match="no forward"):
        hot.query_rays(torch.zeros(1, 4, 2), torch.ones(1, 4, 1))
    with pytest.raises(IdhError, match="no forward"):
        hot.query_points(torch.zeros(1, 4, 3), torch.eye(4)[None], torch.eye(4)[None])


def test_queries_refuse_cpu_tensors_wrong_batch_and_missing_scales():
    from implicit_depth_amd._lib import IdhError

    hot = _hot()
    hot._last = {"ent": None, "final": {0: None}, "B": 1}  # as after a forward that built scale 0 only
    with pytest.raises(IdhError, match="CPU tensor"):
        hot.query_rays(torch.zeros(1, 4, 2), torch.ones(1, 4, 1))
    with pytest.raises(IdhError, match="CPU tensor"):
        hot.query_points(torch.zeros(1, 4, 3), torch.eye(4)[None], torch.eye(4)[None])
    with pytest.raises(IdhError, match="batch size"):
        hot.query_rays(torch.zeros(2, 4, 2), torch.ones(2, 4, 1))
    with pytest.raises(IdhError, match="scales"):
        hot.query_rays(torch.zeros(1, 4, 2), torch.ones(1, 4, 1), scales=(0, 2))
    with pytest.raises(IdhError, match="query_scales"):
        hot.query_rays(torch.zeros(1, 4, 2), torch.ones(1, 4, 1), scales=(4,))


def test_full_plan_only_when_a_coarse_scale_is_queried():
    from implicit_depth_amd import nhwc

    hot = _hot()
    assert hot._scales(False) == 0b0001 and hot._scales(False, (0,)) == 0b0001
    assert hot._scales(False, (0, 2)) == nhwc.ALL_SCALES and hot._scales(True) == nhwc.ALL_SCALES


def test_f16x3_is_refused_and_session_needs_a_prediction():
    from implicit_depth_amd import mlp, nhwc
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    hot = _hot()
    hot.binary_mlp.mlp_math = "f16x3"
    view = nhwc.View(torch.zeros(1, 4, 4, 64), 0, 64)
    with pytest.raises(IdhError, match="fp32 only"):
        mlp.ray_logits(hot.binary_mlp, view, torch.zeros(1, 4, 2), torch.ones(1, 4, 1))
    s = StreamingSession.__new__(StreamingSession)
    s._key = None
    with pytest.raises(IdhError, match="no prediction"):
        s.query_points(torch.zeros(1, 4, 3))


def test_projection_table_keeps_clear_of_every_boundary():
    pts, cTw, K, prior, pcTw, pK = Q.projection_inputs()
    ref = Q.projection_reference(pts, cTw, K, Q.PROJ_H, Q.PROJ_W)
    val, sx, sy, pcz = Q.prior_nearest_reference(pts, pcTw, pK, prior, Q.PROJ_H, Q.PROJ_W)
    assert Q.near_boundary_share(ref, sx, sy, pcz, Q.PROJ_H, Q.PROJ_W) == 0.0
    front = ref["cz"] > 0  # (behind the camera u, v are c_xy / 1e-5 and decide nothing)
    assert float(ref["e_rays"][front].max()) < Q.PROJ_MARGIN / 10 and float(ref["e_cz"].max()) < Q.PROJ_MARGIN / 10  # the fp32 chain cannot cross a boundary
    pref = Q.projection_reference(pts, pcTw, pK, Q.PROJ_H, Q.PROJ_W)
    assert float(pref["e_rays"][pcz > 0].max()) < Q.PROJ_MARGIN / 10 and float(pref["e_cz"].max()) < Q.PROJ_MARGIN / 10
    u, v, cz = ref["rays"][..., 0], ref["rays"][..., 1], ref["cz"]
    valid = (cz > 0) & (u >= 0) & (u < Q.PROJ_W) & (v >= 0) & (v < Q.PROJ_H)
    assert (cz < 0).any() and (u < 0)[cz > 0].any() and (u > Q.PROJ_W)[cz > 0].any() and (v < 0)[cz > 0].any() and (v > Q.PROJ_H)[cz > 0].any()
    assert ((u.abs() < 0.02) & (cz > 0)).any() and (((v - Q.PROJ_H).abs() < 0.02) & (cz > 0)).any()  # points on the image edge, both sides
    assert 0.3 < valid.double().mean() < 0.9 and (val == -1).any() and (val >= 0).any()
