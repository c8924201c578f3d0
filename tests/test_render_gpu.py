"""Shaded mesh render on the GPU (csrc/raster_shade.hip, raster.render_shaded / AssetRenderer, StreamingSession.composite_asset) against
the depth-only path (bit for bit) and the fp64 brute force of tests/render_ref.py.  What counts as ambiguous is defined there;
test_render_cpu.py checks that the general scenes stay under the 1 % cap.

Error bars.  Depth: the project's 1e-4 relative.  Barycentrics and attributes: at most FACTOR x the largest error of the float32 numpy
restatement of the kernel's expressions (render_ref.restate_f32) on the same view, with a floor of 1e-6; the factor covers another
summation order and division rounding - a margin over the reference's own arithmetic, not a number taken from the kernel.  Colours:
within 1 of the fp64 rounding, equal where the fp64 value is more than 0.05 from a half-integer."""
import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import raster_ref as rr
import render_ref as R

pytestmark = pytest.mark.gpu
RTOL = 1e-4
FACTOR, FLOOR = 4.0, 1e-6
HALF_BAND = 0.05


def _render(verts, faces, cams, K, H, W, **kw):
    from implicit_depth_amd import raster

    return raster.render_shaded(verts.cuda(), faces.cuda(), cams.cuda(), K.cuda(), H, W, **kw)


def _all_outputs(verts, faces, cams, K, H, W, C=3, ambient=0.3, seed=11):
    attrs, colors = R.vertex_attrs(len(verts), C, seed), R.vertex_colors(len(verts), seed + 1)
    out = _render(verts, faces, cams, K, H, W, colors=torch.from_numpy(colors).cuda(), attrs=torch.from_numpy(attrs).cuda(), ambient=ambient,
                  return_faces=True, return_bary=True)
    torch.cuda.synchronize()
    assert out["depth"].shape == (len(cams), 1, H, W) and out["rgba"].shape == (len(cams), H, W, 4) and out["rgba"].dtype == torch.uint8
    assert out["attrs"].shape == (len(cams), H, W, C) and out["pix_to_face"].shape == (len(cams), H, W) and out["pix_to_face"].dtype == torch.int32
    assert out["bary"].shape == (len(cams), H, W, 3)
    return out, attrs, colors


def _check_view(what, out, b, ref, verts, faces, cam, K, H, W, attrs, colors, ambient):
    """One camera of a render with every output against its reference.  Returns the number of unambiguous covered pixels."""
    v, f, cam, K = verts.numpy(), faces.numpy(), cam.numpy(), K.numpy()
    depth = out["depth"][b, 0].cpu().numpy().astype(np.float64)
    face = out["pix_to_face"][b].cpu().numpy().astype(np.int64)
    bary = out["bary"][b].cpu().numpy().astype(np.float64)
    att = out["attrs"][b].cpu().numpy().astype(np.float64)
    rgba = out["rgba"][b].cpu().numpy().astype(np.int64)
    ok, cov = ~ref["ambiguous"], ref["covered"]
    # coverage, depth and the winning face
    wrong, err, empties = rr.compare_render(depth, ref["depth"], ref["ambiguous"])
    assert wrong == 0 and empties and err < RTOL, (what, b, wrong, err)
    assert ((face >= 0) == (depth > 0)).all() and (face < len(f)).all(), (what, b)
    assert (face[ok] == ref["face"][ok]).all(), (what, b, int((face[ok] != ref["face"][ok]).sum()))
    gcov = face >= 0
    own = R.face_depth(v, f, cam, K, H, W, face)
    with np.errstate(invalid="ignore", divide="ignore"):
        werr = np.abs(own[gcov] - ref["z"][gcov]) / ref["z"][gcov]
    worst = float(werr.max()) if werr.size else 0.0
    print(f"{what} view {b}: ambiguous {ref['ambiguous'].mean():.4%}, depth err {err:.2e}, reported faces' own depth vs the reference's {worst:.2e}")
    assert worst <= RTOL, (what, b, worst)  # every reported face is a legitimate winner (an uncovered reference pixel gives inf)
    # empties
    e = ~gcov
    assert (bary[e] == 0).all() and (att[e] == 0).all() and (rgba[e] == 0).all(), (what, b)
    assert ((rgba[..., 3] == 0) == e).all(), (what, b)  # alpha 0 exactly on the empty pixels (the test's colours have alpha >= 64)
    m = ok & cov
    n = int(m.sum())
    if n == 0:
        return 0
    ys, xs = np.nonzero(m)
    base = R.restate_f32(v, f, cam, K, ys, xs, ref["face"][m], attrs=attrs, colors=colors, ambient=ambient)
    for name, got, want, restated in (("bary", bary[m], ref["bary"][m], base["bary"]),
                                      ("attrs", att[m], R.interpolate(ref, f, attrs)[m], base["attrs"])):
        e_ref = max(float(np.abs(restated.astype(np.float64) - want).max()), FLOOR)
        e_got = float(np.abs(got - want).max())
        print(f"{what} view {b} {name}: kernel {e_got:.2e}, float32 restatement {e_ref:.2e}, ratio {e_got / e_ref:.2f} (bound {FACTOR})")
        assert e_got <= FACTOR * e_ref, (what, b, name, e_got, e_ref)
    col = R.colour(ref, f, colors, ambient)[m]
    want = R.round_u8(col)
    diff = np.abs(rgba[m] - want)
    clipped = np.clip(col, 0.0, 255.0)
    clear = np.abs(clipped - np.floor(clipped) - 0.5) > HALF_BAND
    print(f"{what} view {b} rgba: off by one at {int((diff == 1).sum())} of {diff.size} channel values, {int((~clear).sum())} within {HALF_BAND} of a half-integer")
    assert diff.max() <= 1 and (diff[clear] == 0).all(), (what, b, int(diff.max()), int((diff[clear] != 0).sum()))
    return n


def _check_scene(what, verts, faces, cams, K, H, W, refs=None, C=3, ambient=0.3, need_covered=True):
    from implicit_depth_amd import raster

    out, attrs, colors = _all_outputs(verts, faces, cams, K, H, W, C=C, ambient=ambient)
    plain = raster.render_depth(verts.cuda(), faces.cuda(), cams.cuda(), K.cuda(), H, W)
    assert torch.equal(out["depth"], plain), what
    total = 0
    for b in range(len(cams)):
        ref = refs[b] if refs is not None else R.render(verts.numpy(), faces.numpy(), cams[b].numpy(), K[b].numpy(), H, W)
        total += _check_view(what, out, b, ref, verts, faces, cams[b], K[b], H, W, attrs, colors, ambient)
    assert total > 0 or not need_covered, what
    return out


# ---- depth bits -----------------------------------------------------------------------------------------------------
def _depth_bits(what, verts, faces, cams, K, H, W):
    from implicit_depth_amd import raster

    v, f, T, Km = verts.cuda(), faces.cuda().to(torch.int32), cams.cuda(), K.cuda()
    plain = raster.render_depth(v, f, T, Km, H, W)
    col = torch.from_numpy(R.vertex_colors(len(verts), 3)).cuda()
    att = torch.from_numpy(R.vertex_attrs(len(verts), 2, 4)).cuda()
    for kw in (dict(), dict(colors=col), dict(attrs=att, return_faces=True), dict(colors=col, attrs=att, return_faces=True, return_bary=True, ambient=1.0)):
        out = raster.render_shaded(v, f, T, Km, H, W, **kw)
        assert torch.equal(out["depth"], plain), (what, sorted(kw))
        assert set(out) == {"depth"} | ({"rgba"} if "colors" in kw else set()) | ({"attrs"} if "attrs" in kw else set()) | \
            ({"pix_to_face"} if kw.get("return_faces") else set()) | ({"bary"} if kw.get("return_bary") else set())
    zero = raster.render_shaded(v, f, T, Km, H, W, empty_depth=0.0, return_faces=True)
    empty = plain == -1
    assert torch.equal(zero["depth"][~empty], plain[~empty]) and (zero["depth"][empty] == 0).all(), what
    assert torch.equal(zero["pix_to_face"][:, None] == -1, empty), what
    return plain, empty


@pytest.mark.parametrize("case", [0, 1])
def test_depth_equals_the_depth_only_path_on_the_general_scenes(case):
    name, H, W, verts, faces, cams, K = list(rr.general_cases())[case]
    plain, empty = _depth_bits(name, verts, faces, cams, K, H, W)  # B = 2 in one call
    assert 0 < int(empty.sum()) < empty.numel()


def test_depth_equals_the_depth_only_path_on_the_wall_and_the_query_plane():
    from implicit_depth_amd import raster

    verts, faces, cams, K = syn.static_vertex_scene(192, 256)
    plain, empty = _depth_bits("static", verts, faces, cams, K, 192, 256)
    assert not empty.any()
    H, W = 192, 256
    plane = raster.plane_vertices(syn.plane_pose(0).cuda(), torch.tensor(2.0)).contiguous().cpu()
    pf = raster.plane_faces()
    Km = syn.intrinsics(W, H).float()[None]
    for ry, holes in ((0.0, False), (1.2, True)):  # after the turn part of the plane is behind the camera: faces cross z = 0
        cam = torch.linalg.inv(syn._rot_y(ry)).float()[None]
        plain, empty = _depth_bits(f"plane turned {ry}", plane, pf, cam, Km, H, W)
        assert bool(empty.any()) == holes and not empty.all()


# ---- faces, barycentrics, attributes, colours against fp64 ------------------------------------------------------------
@pytest.mark.parametrize("case,C,ambient", [(0, 3, 0.3), (1, 16, 1.0), (1, 1, 0.3)])
def test_general_scenes_match_the_brute_force(case, C, ambient):
    name, H, W, verts, faces, cams, K, refs = R.general_case(case)
    for ref in refs:
        assert ref["ambiguous"].mean() <= rr.AMBIGUOUS_CAP
    _check_scene(f"{name} C={C} ambient={ambient}", verts, faces, cams, K, H, W, refs=refs, C=C, ambient=ambient)


def test_two_renders_are_identical_and_the_lowest_face_wins_a_tie():
    name, H, W, verts, faces, cams, K = list(rr.general_cases())[1]
    a, _, _ = _all_outputs(verts, faces, cams, K, H, W)
    b, _, _ = _all_outputs(verts, faces, cams, K, H, W)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    one, _, _ = _all_outputs(verts, faces, cams[1:], K[1:], H, W)
    for k in a:
        assert torch.equal(one[k][0], a[k][1]), f"{k}: a camera's render depends on its place in the batch"
    # every face twice: each hit now ties with its copy F faces later, and the first must win everywhere
    twice, _, _ = _all_outputs(verts, torch.cat([faces, faces]), cams, K, H, W)
    for k in a:
        assert torch.equal(twice[k], a[k]), k
    # the copies first in another order: the winner is the lowest index, so the reported face moves with the order and nothing else does
    flipped, _, _ = _all_outputs(verts, torch.cat([faces.flip(0), faces]), cams, K, H, W)
    # (where two DIFFERENT faces are within rounding of each other the other one may now be first: those pixels are ambiguous)
    clear = torch.from_numpy(np.stack([~r["ambiguous"] for r in R.general_case(1)[7]])).cuda() & (a["pix_to_face"] >= 0)
    assert torch.equal(flipped["pix_to_face"][clear].long(), len(faces) - 1 - a["pix_to_face"][clear].long())
    assert torch.equal(flipped["depth"], a["depth"])


# ---- the smallest shapes where it can go wrong ------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (9, 7), (17, 70)])
def test_small_and_odd_images(H, W):
    verts, faces, cams, K = syn.raster_scene(H, W, seed=3, cells=6)
    _check_scene(f"{H}x{W}", verts, faces, cams, K, H, W, need_covered=H * W > 1)


def _small_cam(W, H):
    return torch.eye(4)[None], syn.intrinsics(W, H).float()[None]


def test_single_faces_through_the_queue():
    H, W = 30, 41
    cam, K = _small_cam(W, H)
    # one triangle covering the whole image: a box of H x W pixel centres, resolved by a wave over 8 x 8 tiles
    verts = torch.tensor([[-9.0, -8.0, 2.0], [11.0, -7.0, 3.5], [0.5, 14.0, 2.5]])
    out = _check_scene("covering", verts, torch.tensor([[0, 1, 2]]), cam, K, H, W)
    assert (out["pix_to_face"] == 0).all()
    # one triangle across z = 0: its box is the whole image, only its front part is drawn
    verts = torch.tensor([[-1.0, -1.0, 1.5], [1.5, -0.5, 2.0], [0.2, 0.8, -0.5]])
    out = _check_scene("straddling", verts, torch.tensor([[0, 1, 2]]), cam, K, H, W)
    cov = out["pix_to_face"] >= 0
    assert cov.any() and not cov.all()


def test_mesh_of_small_faces_only():
    """Cells of about 2 x 2 pixels: every face's box holds far fewer than 64 pixel centres, so nothing is queued."""
    H, W, n = 40, 56, 24
    cam, K = _small_cam(W, H)
    Km = K[0].double()
    r = np.random.default_rng(0)
    gy, gx = np.meshgrid(np.linspace(0.08, 0.93, n + 1), np.linspace(0.05, 0.9, n + 1), indexing="ij")
    z = 2.0 + 0.2 * np.sin(3 * gx) * np.cos(2 * gy) + 0.01 * r.standard_normal(gx.shape)
    x, y = (gx * W - float(Km[0, 2])) / float(Km[0, 0]) * z, (gy * H - float(Km[1, 2])) / float(Km[1, 1]) * z
    verts = torch.from_numpy(np.stack([x, y, z], -1).reshape(-1, 3)).float()
    faces = torch.from_numpy(syn._grid_faces(n, n))
    out = _check_scene("small faces", verts, faces, cam, K, H, W)
    cov = out["pix_to_face"] >= 0
    assert 0.5 < cov.float().mean() < 1.0


def test_three_cameras_with_their_own_intrinsics():
    H, W = 33, 47
    verts, faces, cams, K = syn.raster_scene(H, W, seed=4, cells=8)
    third = torch.linalg.inv(syn._rot_y(-0.15)).float()
    third[0, 3], third[2, 3] = 0.2, 0.3
    cams3 = torch.cat([cams, third[None]])
    K3 = torch.stack([K[0], syn.pinhole(31.7, 44.3, 20.9, 15.2).float(), syn.pinhole(52.0, 47.0, 25.5, 13.0).float()])
    out = _check_scene("three cameras", verts, faces, cams3, K3, H, W)
    assert not torch.equal(out["depth"][0], out["depth"][1]) and not torch.equal(out["depth"][1], out["depth"][2])


def test_faces_that_draw_nothing_and_no_faces():
    H, W = 30, 40
    cam, K = _small_cam(W, H)
    verts = torch.tensor([[0.0, 0.0, 1.0], [float("nan"), 0.0, 1.0], [0.0, float("inf"), 1.0], [0.1, 0.0, 1.0], [0.0, 0.1, 1.0]])
    col = torch.full((5, 4), 200, dtype=torch.uint8).cuda()
    att = torch.ones(5, 2).cuda()
    for faces in (torch.zeros(0, 3, dtype=torch.int64), torch.tensor([[0, 1, 3], [0, 2, 4], [0, 0, 3], [0, 3, 77], [-1, 3, 4]])):
        out = _render(verts, faces, cam, K, H, W, colors=col, attrs=att, return_faces=True, return_bary=True, empty_depth=-3.0)
        assert (out["depth"] == -3.0).all() and (out["pix_to_face"] == -1).all()
        assert (out["rgba"] == 0).all() and (out["attrs"] == 0).all() and (out["bary"] == 0).all()
    faces = torch.tensor([[0, 1, 3], [0, 3, 77], [0, 3, 4], [0, 2, 4]])
    out = _check_scene("one drawable face of four", verts, faces, cam, K, H, W)
    drawn = out["pix_to_face"][out["pix_to_face"] >= 0]
    assert drawn.numel() > 0 and (drawn == 2).all()
    none = _render(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64), cam, K, H, W, return_faces=True)
    assert (none["depth"] == -1).all() and (none["pix_to_face"] == -1).all()


def test_python_checks_its_arguments():
    from implicit_depth_amd import raster
    from implicit_depth_amd._lib import IdhError

    verts, faces, cams, K = (t.cuda() for t in syn.static_vertex_scene(16, 24))
    V = len(verts)
    for kw in (dict(colors=torch.zeros(V, 3, dtype=torch.uint8).cuda()), dict(colors=torch.zeros(V, 4).cuda()), dict(colors=torch.zeros(V, 4, dtype=torch.uint8)),
               dict(attrs=torch.zeros(V, 17).cuda()), dict(attrs=torch.zeros(V + 1, 2).cuda()), dict(attrs=torch.zeros(V, 2)), dict(ambient=1.5),
               dict(ambient=float("nan"))):
        with pytest.raises(IdhError):
            raster.render_shaded(verts, faces, cams, K, 16, 24, **kw)


# ---- AssetRenderer ----------------------------------------------------------------------------------------------------
def _asset_mesh(seed=0, n=10, size=0.5):
    r = np.random.default_rng(seed)
    g = np.linspace(-size / 2, size / 2, n + 1)
    yy, xx = np.meshgrid(g, g, indexing="ij")
    zz = 0.08 * np.sin(7 * xx) * np.cos(5 * yy) + 0.004 * r.standard_normal(xx.shape)
    verts = torch.from_numpy(np.stack([xx, yy, zz], -1).reshape(-1, 3)).float()
    return verts, torch.from_numpy(syn._grid_faces(n, n)), torch.from_numpy(R.vertex_colors(len(verts), seed + 5))


def test_asset_renderer_renders_and_moves_the_asset():
    from implicit_depth_amd import AssetRenderer, raster

    H, W = 48, 64
    verts, faces, colors = _asset_mesh()
    K = syn.intrinsics(W, H).float()
    world_T_cam = syn.keyframe_trajectory("orbit")[0][5]
    asset = AssetRenderer(verts, faces, colors, ambient=0.45)
    placements = [np.eye(4), syn._rot_y(0.4).numpy()]
    placements[1][:3, 3] = (0.25, -0.1, 0.3)
    faces_seen = []
    for i, world_T_asset in enumerate(placements):
        if i:
            asset.place(world_T_asset)
        got = asset.render(world_T_cam, K, (H, W), return_faces=True, return_bary=True)
        cam_T_mesh = torch.from_numpy((np.linalg.inv(world_T_cam) @ world_T_asset).astype(np.float32))[None]
        want = raster.render_shaded(verts.cuda(), faces.cuda(), cam_T_mesh.cuda(), K[None].cuda(), H, W, colors=colors.cuda(), ambient=0.45,
                                    return_faces=True, return_bary=True)
        assert set(got) == set(want) == {"depth", "rgba", "pix_to_face", "bary"}
        for k in want:
            assert torch.equal(got[k], want[k]), (i, k)
        zero = asset.render(world_T_cam, K[None], (H, W), empty_depth=0.0)
        assert torch.equal(zero["depth"] == 0, got["depth"] == -1) and torch.equal(zero["rgba"], got["rgba"])
        ref = R.render(verts.numpy(), faces.numpy(), cam_T_mesh[0].numpy(), K.numpy(), H, W)
        face = got["pix_to_face"][0].cpu().numpy()
        ok = ~ref["ambiguous"]
        assert (face[ok] == ref["face"][ok]).all(), i
        assert 0.02 < ref["covered"].mean() < 0.9, (i, ref["covered"].mean())
        faces_seen.append(face)
    assert (faces_seen[0] != faces_seen[1]).mean() > 0.02  # the asset moved in the image


# ---- the live frame --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("query_keyframes", [1, 3])
def test_composite_asset_equals_the_public_calls_chained_by_hand(query_keyframes):
    from implicit_depth_amd import AssetRenderer, compositing, raster
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession
    from test_ray_query_gpu import BUFFER, IMG_H, IMG_W, _frame, _model

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    session = StreamingSession(_model("mlp", 3), buffer_size=BUFFER, query_keyframes=query_keyframes)
    verts, faces, colors = _asset_mesh(seed=1)
    asset = AssetRenderer(verts, faces, colors, world_T_asset=np.eye(4), ambient=0.3)  # the orbit's centre: 1.5 m in front of every camera
    K = syn.intrinsics(IMG_W, IMG_H).float().cuda()
    image = torch.randint(0, 256, (1, IMG_H, IMG_W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    with pytest.raises(IdhError, match="no prediction"):
        session.composite_asset(image, asset, poses[0], K)
    predictions, done = 0, False
    for t in range(9):
        out, code = session.step(_frame(t, poses), world_T_cam=poses[t], dist_to_last_valid=dists[t])
        predictions += out is not None
        if out is not None or predictions == 0:
            continue
        # a frame where step() returned None, after at least one prediction: the asset at the live pose, the features of the keyframe(s)
        assert predictions >= query_keyframes
        cam_T_mesh = torch.from_numpy(np.linalg.inv(poses[t]).astype(np.float32))[None].cuda()  # world_T_asset is the identity
        rgba = raster.render_shaded(asset.verts, asset.faces, cam_T_mesh, K[None], IMG_H, IMG_W, colors=asset.colors, ambient=0.3)["rgba"]
        shown = rgba[0, ..., 3] > 0
        assert 0.01 < shown.float().mean() < 0.9
        for size in (None, (45, 60)):
            kw = {} if size is None else {"query_size": size}
            h, w = compositing.MODEL_SIZE if size is None else size
            got = session.composite_asset(image, asset, poses[t], K, return_parts=True, **kw)
            Kq = K[None].clone()
            Kq[:, 0] *= w / IMG_W
            Kq[:, 1] *= h / IMG_H
            depth = raster.render_shaded(asset.verts, asset.faces, cam_T_mesh, Kq, h, w, colors=asset.colors, ambient=0.3)["depth"]
            v = session.occlusion_for_view(depth, poses[t], torch.linalg.inv(Kq), fill=-20.0)
            frame = compositing.composite_mask(image, v["view_pred"], virtual_rgba=rgba)
            assert torch.equal(got["frame"], frame) and torch.equal(got["asset_depth"], depth) and torch.equal(got["asset_rgba"], rgba)
            for k in v:
                assert (got[k] is None and v[k] is None) or torch.equal(got[k], v[k]), k
            assert frame.shape == image.shape and frame.dtype == torch.uint8
            assert tuple(depth.shape) == (1, 1, h, w) and 0 < int((depth > 0).sum()) < h * w
            assert int((frame[0][~shown].int() - image[0][~shown].int()).abs().max()) <= 1 and not torch.equal(frame[0][shown], image[0][shown])
            assert torch.equal(session.composite_asset(image, asset, poses[t], K, **kw), frame)
            faded = session.composite_asset(image, asset, poses[t], K, bgr=True, fade=[0.5], **kw)
            assert torch.equal(faded, compositing.composite_mask(image, v["view_pred"], virtual_rgba=rgba, fade=[0.5], bgr=True))
        done = True
        break
    assert done, "the sequence has no frame between keyframes after the first prediction"
