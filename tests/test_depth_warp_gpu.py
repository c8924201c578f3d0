"""Depth reprojection on the GPU (csrc/depth_warp.hip, raster.warp_depth) against the fp64 brute force of tests/warp_ref.py, which also
defines what counts as ambiguous; test_depth_warp_cpu.py checks that the committed scenes stay under the 1 % cap and hold what they are
there for (faces through the queue, faces across z = 0, torn faces, invalid taps).

Error bars.  Depth: the 1e-4 relative of the raster tests (fp32 vertices, a ray / plane intersection per pixel).  Coverage: no mismatch
outside ambiguous pixels.  Everything that compares two GPU results compares bits."""
import functools

import numpy as np
import pytest
import torch

import warp_ref as WR

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _warp(depth_mhw, invK_m44, T_bm44, K_b44, H, W, **kw):
    from implicit_depth_amd import raster

    out = raster.warp_depth(_t(depth_mhw)[:, None], _t(invK_m44), _t(T_bm44), _t(K_b44), H, W, **kw)
    torch.cuda.synchronize()
    assert tuple(out["depth"].shape) == (len(T_bm44), 1, H, W)
    return out


def _scene(name, **kw):
    depth, invK, T, K, H, W = WR.scene_inputs(name)
    return _warp(depth, invK, T[None], K[None], H, W, **kw)


def _hold(what, got, ref, empty_depth=-1.0):
    wrong, err, empties = WR.compare(got, ref, empty_depth)
    print(f"{what}: ambiguous {ref['ambiguous'].mean():.4%}, coverage mismatches {wrong}, depth err {err:.2e}, empties exact {empties}")
    assert wrong == 0 and err < RTOL and empties, (what, wrong, err, empties)


# ---- brute force ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WR.TARGETS))
def test_scenes_match_the_brute_force(name):
    ref = WR.scene_reference(name)
    out = _scene(name, return_source=True)
    got = out["depth"][0, 0].cpu().numpy()
    _hold(name, got, ref)
    assert torch.equal(out["source"][0] == -1, out["depth"][0, 0] == -1.0)
    # another fill value moves the empties and nothing else
    far = _scene(name, empty_depth=1e4)["depth"][0, 0]
    empty = out["depth"][0, 0] == -1.0
    assert 0 < int(empty.sum()) < empty.numel()
    assert (far[empty] == 1e4).all() and torch.equal(far[~empty], out["depth"][0, 0][~empty])
    _hold(name + " (empty_depth 1e4)", far.cpu().numpy(), ref, empty_depth=1e4)


# ---- a plane ----------------------------------------------------------------------------------------------------------
def test_a_tilted_plane_lands_on_the_closed_form_without_holes():
    depth, invK, T, K, H, W, want, inside = WR.plane_case()
    got = _warp(depth, invK, T[None], K[None], H, W)["depth"][0, 0].cpu().numpy().astype(np.float64)
    cov = got > 0
    err = float((np.abs(got[cov] - want[cov]) / want[cov]).max())
    print(f"plane: covered {cov.mean():.3f}, must be covered {inside.mean():.3f}, holes among them {int((inside & ~cov).sum())}, depth err {err:.2e}")
    assert inside.mean() > 0.3 and cov[inside].all()
    assert err < RTOL
    assert (got[~cov] == -1.0).all() and 0 < (~cov).sum()


# ---- tears ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["48x64", "24x32"])
def test_the_gap_behind_the_box_is_empty_when_torn_and_covered_by_the_rubber_sheet(name):
    torn_ref, sheet_ref = WR.scene_reference(name), WR.scene_reference(name, float("inf"))
    clear = ~torn_ref["ambiguous"] & ~sheet_ref["ambiguous"]
    gap = clear & (sheet_ref["depth"] > 0) & (torn_ref["depth"] < 0)
    assert gap.sum() >= 5, gap.sum()
    torn = _scene(name)["depth"][0, 0].cpu().numpy()
    sheet = _scene(name, tear_ratio=float("inf"))["depth"][0, 0].cpu().numpy()
    print(f"{name}: {int(gap.sum())} pixels see the gap")
    assert (torn[gap] == -1.0).all() and (sheet[gap] > 0).all()
    _hold(name + " torn", torn, torn_ref)
    _hold(name + " rubber sheet", sheet, sheet_ref)
    # a ratio the whole scene stays under is the rubber sheet
    assert np.array_equal(_scene(name, tear_ratio=4.0)["depth"][0, 0].cpu().numpy(), sheet)


# ---- invalid maps -----------------------------------------------------------------------------------------------------
def test_invalid_taps_remove_exactly_their_faces():
    _, invK, T, K, H, W = WR.scene_inputs("30x44")
    whole = WR.source_depth(holes=False)
    for bad in (0.0, float("nan"), -2.0, float("inf"), float("-inf")):
        out = _warp(np.full_like(whole, bad)[None], invK, T[None], K[None], H, W, return_source=True)
        assert (out["depth"] == -1.0).all() and (out["source"] == -1).all(), bad
    holed = whole.copy()
    taps = [(3, 5, 0.0), (3, 6, np.nan), (12, 14, -1.5), (20, 4, np.inf), (0, 0, np.nan), (23, 31, 0.0), (9, 9, -np.inf)]
    for i, j, v in taps:
        holed[i, j] = v
    a = _warp(whole[None], invK, T[None], K[None], H, W, return_source=True)
    b = _warp(holed[None], invK, T[None], K[None], H, W, return_source=True)
    _, faces, draws, _ = WR.build(holed, invK[0], T[0])
    _, _, draws_whole, _ = WR.build(whole, invK[0], T[0])
    removed = draws_whole & ~draws
    touched = np.zeros(len(faces), bool)
    for i, j, _ in taps:
        touched |= (faces == i * WR.SRC_W + j).any(1)
    assert (removed == (touched & draws_whole)).all() and removed.sum() > 0
    src_a, src_b = a["source"][0].cpu().numpy(), b["source"][0].cpu().numpy()
    lost = (src_a >= 0) & removed[np.maximum(src_a, 0)]
    assert lost.sum() > 0
    # a pixel whose winner is still drawn keeps its bits; a pixel whose winner was removed has another winner or none
    assert torch.equal(a["depth"][0, 0][_t(~lost)], b["depth"][0, 0][_t(~lost)]) and (src_a[~lost] == src_b[~lost]).all()
    assert (src_b[lost] != src_a[lost]).all()
    assert not removed[src_b[src_b >= 0]].any() and draws[src_b[src_b >= 0]].all()
    _hold("holed", b["depth"][0, 0].cpu().numpy(), WR.render(holed[None], invK, T, K, H, W))


# ---- several sources and targets ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_by_two():
    """Two sources (their own depth maps, poses and intrinsics) and two targets: the inputs and the four single-source references."""
    from implicit_depth_amd import raster

    depths = np.stack([WR.source_depth(0), WR.source_depth(3, box=False) + np.float32(0.13)])
    Ks = [WR.source_K(), WR._pinhole(27.1, 29.3, 16.4, 11.2)]
    invK = np.stack([np.linalg.inv(k) for k in Ks]).astype(np.float32)
    world_T_src = [np.eye(4), WR._pose(-0.06, 0.03, -0.04, (0.1, 0.02, -0.03))]
    world_T_cam = [np.linalg.inv(WR.GENERIC_POSE), WR._pose(0.05, 0.06, 0.1, (-0.08, 0.05, 0.1))]
    T = raster.relative_poses(world_T_cam, world_T_src).numpy()
    H, W = 30, 44
    K = np.stack([WR.TARGETS["30x44"][2], WR._pinhole(35.0, 37.2, 20.3, 16.6)]).astype(np.float32)
    refs = [[WR.render(depths[m:m + 1], invK[m:m + 1], T[b, m:m + 1], K[b], H, W) for m in range(2)] for b in range(2)]
    return depths, invK, T, K, H, W, refs


def test_two_sources_in_two_targets_are_the_minimum_of_the_single_source_calls():
    depths, invK, T, K, H, W, refs = _two_by_two()
    F = 2 * (WR.SRC_H - 1) * (WR.SRC_W - 1)
    both = _warp(depths, invK, T, K, H, W, return_source=True)
    again = _warp(depths, invK, T, K, H, W, return_source=True)
    assert torch.equal(both["depth"], again["depth"]) and torch.equal(both["source"], again["source"])
    one = [_warp(depths[m:m + 1], invK[m:m + 1], T[:, m:m + 1], K, H, W, return_source=True) for m in range(2)]
    d0, d1 = one[0]["depth"], one[1]["depth"]
    inf = torch.full_like(d0, float("inf"))
    z0, z1 = torch.where(d0 == -1.0, inf, d0), torch.where(d1 == -1.0, inf, d1)
    zmin = torch.minimum(z0, z1)
    assert torch.equal(both["depth"], torch.where(zmin == inf, torch.full_like(zmin, -1.0), zmin))
    want_src = torch.where(z0 <= z1, one[0]["source"][:, None], one[1]["source"][:, None] + F)  # among equal depths the lowest id
    want_src = torch.where(zmin == inf, torch.full_like(want_src, -1), want_src)
    assert torch.equal(both["source"][:, None], want_src)
    assert bool((z1 < z0).any()) and bool((z0 < z1).any())  # both sources win somewhere
    # a target's result does not depend on its place in the batch
    for b in range(2):
        alone = _warp(depths, invK, T[b:b + 1], K[b:b + 1], H, W, return_source=True)
        assert torch.equal(alone["depth"][0], both["depth"][b]) and torch.equal(alone["source"][0], both["source"][b]), b
    swapped = _warp(depths, invK, T[::-1], K[::-1], H, W)
    assert torch.equal(swapped["depth"][0], both["depth"][1]) and torch.equal(swapped["depth"][1], both["depth"][0])
    # and each single-source call is the brute force's
    for b in range(2):
        for m in range(2):
            _hold(f"target {b} source {m}", one[m]["depth"][b, 0].cpu().numpy(), refs[b][m])


# ---- source ids -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["30x44", "closeup"])
def test_the_named_face_gives_the_returned_depth(name):
    from implicit_depth_amd import raster

    depth, invK, T, K, H, W = WR.scene_inputs(name)
    ref = WR.scene_reference(name)
    out = _scene(name, return_source=True)
    got, src = out["depth"][0, 0].cpu().numpy().astype(np.float64), out["source"][0].cpu().numpy()
    own = WR.face_depth(depth, invK, T, K, H, W, src)
    m = ~ref["ambiguous"] & (src >= 0)
    err = float((np.abs(own[m] - got[m]) / got[m]).max())
    print(f"{name}: the named faces' own depth vs the returned one {err:.2e} over {int(m.sum())} pixels")
    assert m.sum() > 100 and err < RTOL
    _, _, draws, _ = WR.build(depth[0], invK[0], T[0])
    assert draws[src[src >= 0]].all()  # only faces that draw are ever named
    mm, ii, jj, up = raster.decode_source(out["source"], WR.SRC_H, WR.SRC_W)
    cov = out["source"] >= 0
    assert (mm[cov] == 0).all() and (mm[~cov] == -1).all() and int(ii.max()) <= WR.SRC_H - 2 and int(jj.max()) <= WR.SRC_W - 2
    assert torch.equal(WR.source_id(mm, ii, jj, up, WR.SRC_H, WR.SRC_W)[cov], out["source"].long()[cov])


def test_the_source_map_is_right_with_two_sources():
    from implicit_depth_amd import raster

    depths, invK, T, K, H, W, refs = _two_by_two()
    out = _warp(depths, invK, T, K, H, W, return_source=True)
    for b in range(2):
        src = out["source"][b].cpu().numpy()
        got = out["depth"][b, 0].cpu().numpy().astype(np.float64)
        own = WR.face_depth(depths, invK, T[b], K[b], H, W, src)
        clear = ~refs[b][0]["ambiguous"] & ~refs[b][1]["ambiguous"]
        sel = clear & (src >= 0)
        assert float((np.abs(own[sel] - got[sel]) / got[sel]).max()) < RTOL
        z = [np.where(r["depth"] > 0, r["depth"], np.inf) for r in refs[b]]
        with np.errstate(invalid="ignore"):
            decided = clear & np.isfinite(np.minimum(z[0], z[1])) & ~(np.abs(z[0] - z[1]) <= 1e-3 * np.minimum(z[0], z[1]))
        m = raster.decode_source(src, WR.SRC_H, WR.SRC_W)[0]
        want = np.where(z[1] < z[0], 1, 0)
        print(f"target {b}: source 1 wins {int((want[decided] == 1).sum())} of {int(decided.sum())} decided pixels")
        assert (m[decided] == want[decided]).all() and 0 < (want[decided] == 1).sum() < decided.sum()


# ---- the identity pose ------------------------------------------------------------------------------------------------
def test_identity_pose_returns_the_source_depth_where_it_is_covered():
    """Pixel centres fall exactly on mesh vertices and all edge functions round to noise there: coverage is decided by rounding.  The
    share of empty interior pixels is printed (DESIGN.md §4.20 records it); only the covered pixels' depth is asserted."""
    depth = WR.source_depth()
    Ks = WR.source_K()
    invK = np.linalg.inv(Ks).astype(np.float32)
    K = np.linalg.inv(invK.astype(np.float64)).astype(np.float32)
    for tear in (1.1, float("inf")):
        got = _warp(depth[None], invK[None], np.eye(4, dtype=np.float32)[None, None], K[None], WR.SRC_H, WR.SRC_W, tear_ratio=tear)["depth"][0, 0].cpu().numpy()
        _, faces, draws, valid = WR.build(depth, invK, np.eye(4), tear)
        has_face = np.zeros(WR.SRC_H * WR.SRC_W, bool)
        has_face[faces[draws].reshape(-1)] = True
        interior = has_face.reshape(WR.SRC_H, WR.SRC_W).copy()
        interior[0], interior[-1], interior[:, 0], interior[:, -1] = False, False, False, False
        cov = got > 0
        print(f"identity pose, tear_ratio {tear}: {int((interior & ~cov).sum())} of {int(interior.sum())} interior pixels with a drawn face "
              f"at their vertex are empty ({(interior & ~cov).sum() / interior.sum():.2%})")
        assert cov.sum() > 0 and (got[~cov] == -1.0).all() and not cov[~has_face.reshape(WR.SRC_H, WR.SRC_W)].any()
        assert float((np.abs(got[cov] - depth[cov]) / depth[cov]).max()) < RTOL


# ---- arguments --------------------------------------------------------------------------------------------------------
def test_python_checks_its_arguments():
    from implicit_depth_amd import raster
    from implicit_depth_amd._lib import IdhError

    depth, invK, T, K, H, W = WR.scene_inputs("24x32")
    d, iK, Tb, Kb = _t(depth)[:, None], _t(invK), _t(T[None]), _t(K[None])
    for kw in (dict(tear_ratio=0.9), dict(tear_ratio=float("nan"))):
        with pytest.raises(IdhError):
            raster.warp_depth(d, iK, Tb, Kb, H, W, **kw)
    for args in ((d[:, 0], iK, Tb, Kb, H, W), (d, iK[0], Tb, Kb, H, W), (d, iK, Tb[0], Kb, H, W), (d, iK, Tb, Kb[0], H, W), (d, iK, Tb, Kb, 0, W),
                 (d, iK, Tb, Kb, H, -1), (d[..., :1], iK, Tb, Kb, H, W), (d, iK, Tb.expand(1, 2, 4, 4), Kb, H, W), (d, iK, Tb, Kb.expand(2, 4, 4), H, W)):
        with pytest.raises(IdhError):
            raster.warp_depth(*args)
