"""Multi-view depth consistency without a GPU: the fp64 restatement of tests/mv_consistency_ref.py against the reference's own
MVDepthLoss (tests/golden/mv_depth_loss.npz, made by tests/golden/gen_mv_depth_loss.py), the share of ambiguous pixels of the fixtures,
the argument checks of the C entry points that return before anything is launched, and the weighted TSDF reference at weight 1."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import mv_consistency_ref as R
import tsdf_ref

from conftest import ROOT


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "mv_depth_loss.npz"))


def inputs(name):
    g = golden()
    return {k: g[f"{name}/{k}"] for k in ("pred", "cur", "invK", "world_T_cam", "src_depth", "src_K", "src_cam_T_world")}


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_fixtures_are_the_goldens_inputs_and_hardly_ambiguous(name):
    fx, made = inputs(name), R.fixture(name)
    for k in fx:
        assert np.array_equal(fx[k], made[k], equal_nan=True), k
    h, w, B, K, _ = R.CASES[name]
    assert fx["pred"].shape == (B, 1, h, w) and fx["src_depth"].shape == (B, K, 1, h, w)
    share = R.ambiguous_share(fx)
    print(f"{name}: {100 * share:.2f} % of the pixels are ambiguous")
    assert share <= R.CAP


@pytest.mark.parametrize("name", sorted(R.CASES))
@pytest.mark.parametrize("self_gate", [False, True])
def test_restatement_matches_the_reference_in_fp64(name, self_gate):
    g, fx = golden(), inputs(name)
    got = R.check(*R._args(fx, not self_gate))
    pre = f"{name}/f64/self_" if self_gate else f"{name}/f64/"
    mask, err, loss = g[pre + "mask"], g[pre + "err"], float(g[pre + "loss"])
    ok = ~got["ambiguous"]
    assert np.array_equal(got["visible"][ok], mask[ok])
    assert mask.mean() > 0.1
    if not self_gate:
        assert np.array_equal(got["sampled"][ok], g[f"{name}/f64/sampled"][ok], equal_nan=True)
    both = ok & mask
    with np.errstate(invalid="ignore"):  # inf - inf where a tap is infinite
        diff = np.abs(got["err"] - err)[both & np.isfinite(err)]
    assert np.array_equal(np.isfinite(got["err"][both]), np.isfinite(err[both]))
    assert diff.max() < 1e-12
    print(f"{name} self_gate={self_gate}: loss {got['loss']!r} against {loss!r}, max per-pixel difference {diff.max():.1e}")
    if np.isfinite(loss):
        assert abs(got["loss"] - loss) <= 1e-12
    else:
        assert (np.isnan(loss) and np.isnan(got["loss"])) or got["loss"] == loss
    # the sums behind the loss are what it is made of
    with np.errstate(all="ignore"):
        assert np.array_equal(np.float64(got["loss"]), np.mean(got["loss_sum"] / got["loss_count"]), equal_nan=True)


def test_counts_rules_on_a_hand_made_pixel():
    """One pixel, identity cameras, K = 3: a source that agrees, one whose surface is far behind (conflict), one in front (occluded)."""
    eye = np.eye(4, dtype=np.float32)[None]
    K = np.array([[4, 0, 2, 0], [0, 4, 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    d = np.full((1, 1, 4, 4), 2.0, np.float32)
    src = np.stack([np.full((1, 4, 4), v, np.float32) for v in (2.02, 3.0, 1.0)])[None]
    out = R.check(d, np.linalg.inv(K)[None], eye, src, np.repeat(K[None, None], 3, 1), np.repeat(eye[None], 3, 1), min_consistent=1, max_conflict=0)
    assert (out["counts"][0, 0] == 2).all() and (out["counts"][0, 1] == 1).all() and (out["counts"][0, 2] == 1).all()
    assert (out["weight"] == 0).all() and (out["filtered_depth"] == 0).all()  # one conflict is more than max_conflict = 0
    out = R.check(d, np.linalg.inv(K)[None], eye, src, np.repeat(K[None, None], 3, 1), np.repeat(eye[None], 3, 1), min_consistent=1, max_conflict=1)
    assert (out["weight"] == 2).all() and (out["filtered_depth"] == 2).all()
    assert not out["ambiguous"].any()


def test_struct_sizes_and_argument_checks_without_a_gpu():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert L.idh_sizeof_mv_consistency_args() == C.sizeof(_lib.MvConsistencyArgs)
    assert L.idh_sizeof_tsdf_integrate_weighted_args() == C.sizeof(_lib.TsdfIntegrateWeightedArgs)
    assert L.idh_mv_consistency_workspace_bytes(1, 7, 192, 256) == 16 * 7 * 192
    assert L.idh_mv_consistency_workspace_bytes(3, 16, 13, 19) == 16 * 16 * 3 and L.idh_mv_consistency_workspace_bytes(0, 1, 2, 2) == 0
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
    assert b"workspace" in L.idh_error_string(EWORKSPACE)

    def args(**kw):
        a = _lib.MvConsistencyArgs()
        for f in ("depth_b1hw", "invK_b44", "world_T_cam_b44", "src_depth_bk1hw", "src_K_bk44", "src_cam_T_world_bk44"):
            setattr(a, f, 64)  # never dereferenced: every call below returns before a launch
        a.ratio, a.log_tol, a.min_consistent, a.max_conflict = 1.05, 0.05, 1, 0
        a.B, a.K, a.h, a.w, a.src_h, a.src_w = 1, 3, 13, 19, 13, 19
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: L.idh_mv_consistency_fwd(a, None)
    assert L.idh_mv_consistency_fwd(None, None) == EINVAL
    assert call(args(struct_size=C.sizeof(_lib.MvConsistencyArgs) - 8)) == EINVAL
    for bad in (dict(B=-1), dict(K=0), dict(h=0), dict(w=-2), dict(src_h=0), dict(ratio=float("nan")), dict(ratio=0.0), dict(log_tol=0.0),
                dict(log_tol=float("inf")), dict(min_consistent=-1), dict(max_conflict=-1), dict(depth_b1hw=None), dict(invK_b44=None),
                dict(world_T_cam_b44=None), dict(src_depth_bk1hw=None), dict(src_K_bk44=None), dict(src_cam_T_world_bk44=None),
                dict(loss_sum_k=64), dict(loss_count_k=64), dict(loss=64, workspace=68, workspace_bytes=1 << 20)):
        assert call(args(**bad)) == EINVAL, bad
    for bad in (dict(K=17), dict(B=129), dict(src_h=12), dict(src_w=20), dict(B=128, K=16, h=1024, w=1024, src_h=1024, src_w=1024)):
        assert call(args(**bad)) == EUNSUPPORTED, bad
    assert call(args(K=17, log_tol=-1.0)) == EINVAL  # the house order: invalid before unsupported
    assert call(args(loss=64)) == EWORKSPACE and call(args(loss=64, workspace=64, workspace_bytes=16 * 3 - 1)) == EWORKSPACE
    assert call(args(B=0)) == 0  # nothing to launch

    def wargs(**kw):
        a = _lib.TsdfIntegrateWeightedArgs()
        a.depth_m1hw = a.K_m44 = a.cam_T_world_m44 = a.weight_m1hw = 64
        a.max_weight, a.M, a.h, a.w = 64.0, 1, 8, 8
        for k, v in kw.items():
            setattr(a, k, v)
        return a  # (the volume is empty: a call that passes the checks before the volume's stops at the volume's, still before a launch)

    wcall = lambda a: L.idh_tsdf_integrate_weighted_fwd(a, None)
    assert L.idh_tsdf_integrate_weighted_fwd(None, None) == EINVAL
    for bad in (dict(struct_size=8), dict(M=0), dict(max_weight=0.5), dict(weight_m1hw=None), dict(depth_m1hw=None),
                dict(colors_zyx4=64), dict(colors_zyx4=64, color_mhw3=64, color_K_m44=64), dict(colors_zyx4=72, color_mhw3=64, color_K_m44=64, hc=4, wc=4)):
        assert wcall(wargs(**bad)) == EINVAL, bad
    assert wcall(wargs()) == EINVAL  # the volume's own conditions (no dims), reached with the colour pointers NULL


def test_weighted_reference_at_weight_one_is_the_unweighted_reference():
    name = sorted(tsdf_ref.SCENES)[0]
    dims, v, origin, depth, K, E = tsdf_ref.scene_inputs(name)
    plain = tsdf_ref.integrate(tsdf_ref.empty_volume(dims), depth, K, E, origin, v)
    ones = R.integrate_weighted(tsdf_ref.empty_volume(dims), depth, np.ones_like(depth), K, E, origin, v)
    assert plain["touched"].sum() > 100
    for k in ("T", "W", "touched", "ambiguous"):
        assert np.array_equal(plain[k], ones[k]), k
    # a zero or NaN weight is a hole: the same as a hole in the depth
    g = np.ones_like(depth)
    g[:, :, ::2] = 0.0
    g[:, :, 1::4] = np.nan
    holes = tsdf_ref.integrate(tsdf_ref.empty_volume(dims), np.where(g > 0, depth, 0.0).astype(np.float32), K, E, origin, v)
    skipped = R.integrate_weighted(tsdf_ref.empty_volume(dims), depth, g, K, E, origin, v)
    for k in ("T", "W", "touched"):
        assert np.array_equal(holes[k], skipped[k]), k
