"""Host side of the shaded mesh render (include/idh_raster.h: idh_raster_shaded_fwd; raster.render_shaded, AssetRenderer, load_ply's
colours): argument validation of the C entry point and its workspace query, the Python entry points' refusal of CPU tensors, the PLY
reader's colours, and the fp64 reference of tests/render_ref.py - its ambiguity caps on the scenes test_render_gpu.py renders and its
agreement with tests/raster_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import raster_ref as rr
import render_ref as R

OK, EINVAL, EUNSUPPORTED, EWORKSPACE = 0, -1, -2, -4
P = 0x1000  # a non-null, 256-byte aligned pointer that validation never dereferences


def _call(L, **k):
    from implicit_depth_amd import _lib

    a = _lib.RasterShadedArgs()
    base = dict(verts_v3=P, faces_f3=P, cam_T_world_b44=P, K_b44=P, colors_v4=P, attrs_vc=P, depth_b1hw=P, pix_to_face_bhw=P, bary_bhw3=P,
                attr_out_bhwc=P, rgba_bhw4=P, workspace=P, workspace_bytes=1 << 24, ambient=0.3, empty_depth=-1.0, V=8, F=4, B=1, H=4, W=4, C=3)
    for name, val in {**base, **k}.items():
        setattr(a, name, val)
    return L.idh_raster_shaded_fwd(C.byref(a), None)


def test_shaded_entry_point_validates_on_the_host():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert L.idh_sizeof_raster_shaded_args() == C.sizeof(_lib.RasterShadedArgs) == _lib.RasterShadedArgs().struct_size
    # workspace: what the depth-only path needs plus 8 bytes per pixel and camera
    wb = L.idh_raster_shaded_workspace_bytes
    assert wb(2, 100, 50, 30, 40) % 256 == 0 and wb(2, 100, 50, 30, 40) >= L.idh_raster_workspace_bytes(2, 100, 50) - 256 + 2 * 30 * 40 * 8
    assert wb(1, 0, 0, 1, 1) >= 8
    for bad in ((-1, 1, 1, 4, 4), (1, -1, 1, 4, 4), (1, 1, -1, 4, 4), (1, 1, 1, 0, 4), (1, 1, 1, 4, 0), (1, 1, 1, -4, 4)):
        assert wb(*bad) == 0, bad
    r = lambda **k: _call(L, **k)
    assert L.idh_raster_shaded_fwd(None, None) == EINVAL
    assert r(struct_size=8) == EINVAL
    for bad in (dict(verts_v3=None), dict(faces_f3=None), dict(cam_T_world_b44=None), dict(K_b44=None), dict(H=0), dict(W=0), dict(H=-3),
                dict(V=-1), dict(F=-1), dict(B=-1), dict(H=1 << 16, W=1 << 16),
                dict(C=0), dict(C=17), dict(C=-1),                                        # attrs without C; C > 16
                dict(attrs_vc=None, C=3), dict(attrs_vc=None, C=0),                       # attr_out without attrs
                dict(colors_v4=None),                                                     # rgba without colours
                dict(ambient=-0.01), dict(ambient=1.01), dict(ambient=float("nan")), dict(ambient=float("inf")),
                dict(depth_b1hw=None, pix_to_face_bhw=None, bary_bhw3=None, attr_out_bhwc=None, rgba_bhw4=None)):  # no output at all
        assert r(**bad) == EINVAL, bad
    # every output is optional on its own, and so are the inputs only it reads
    for only in ("depth_b1hw", "pix_to_face_bhw", "bary_bhw3", "attr_out_bhwc", "rgba_bhw4"):
        outs = {n: None for n in ("depth_b1hw", "pix_to_face_bhw", "bary_bhw3", "attr_out_bhwc", "rgba_bhw4")}
        outs[only] = P
        assert r(**outs, workspace=None) == EWORKSPACE, only  # gets as far as the workspace check
    assert r(attr_out_bhwc=None, attrs_vc=None, C=0, rgba_bhw4=None, colors_v4=None, workspace=None) == EWORKSPACE
    assert r(ambient=0.0, workspace=None) == EWORKSPACE and r(ambient=1.0, workspace=None) == EWORKSPACE
    assert r(C=16, workspace=None) == EWORKSPACE and r(C=1, workspace=None) == EWORKSPACE
    assert r(B=0) == OK and r(B=0, depth_b1hw=None, cam_T_world_b44=None, workspace=None) == OK  # nothing to do
    assert r(B=0, ambient=2.0) == EINVAL and r(B=0, H=0) == EINVAL
    need = wb(1, 8, 4, 4, 4)
    assert r(workspace=None) == EWORKSPACE and r(workspace_bytes=need - 1) == EWORKSPACE and r(workspace_bytes=-1) == EWORKSPACE
    assert r(workspace=P + 8) == EWORKSPACE and r(workspace=P + 128) == EWORKSPACE
    assert r(workspace_bytes=L.idh_raster_workspace_bytes(1, 8, 4)) == EWORKSPACE  # the depth-only path's size is short: no key plane
    assert r(F=0, faces_f3=None, workspace=None) == EWORKSPACE  # no faces is a valid request (all empty)
    assert r(V=0, verts_v3=None, workspace=None) == EWORKSPACE
    assert r(B=70000, workspace_bytes=1 << 40) == EUNSUPPORTED
    assert r(B=40000, H=256, W=256, workspace_bytes=1 << 40) == EUNSUPPORTED  # B * H * W >= 2^31


def test_python_entry_points_refuse_cpu_tensors():
    import implicit_depth_amd
    from implicit_depth_amd import _lib, raster

    verts, faces, cams, K = syn.static_vertex_scene(16, 24)
    colors = torch.zeros(len(verts), 4, dtype=torch.uint8)
    with pytest.raises(_lib.IdhError):
        raster.render_shaded(verts, faces, cams, K, 16, 24)
    with pytest.raises(_lib.IdhError):
        raster.render_shaded(verts, faces, cams, K, 16, 24, colors=colors, return_faces=True, return_bary=True)
    assert implicit_depth_amd.AssetRenderer is raster.AssetRenderer
    asset = raster.AssetRenderer(verts, faces, colors, device="cpu")
    assert asset.faces.dtype == torch.int32 and np.array_equal(asset.world_T_asset, np.eye(4))
    with pytest.raises(_lib.IdhError):
        asset.render(np.eye(4), K, (16, 24))
    # the camera-from-asset transform is formed in float64 on the host and rounded once
    world_T_cam, world_T_asset = syn.keyframe_trajectory("orbit")[0][7], syn._rot_y(0.3).numpy()
    world_T_asset[:3, 3] = (0.2, -0.1, 1.4)
    asset.place(torch.from_numpy(world_T_asset))
    want = (np.linalg.inv(world_T_cam) @ world_T_asset).astype(np.float32)
    got = asset.cam_T_mesh(world_T_cam)
    assert tuple(got.shape) == (1, 4, 4) and got.dtype == torch.float32 and np.array_equal(got[0].numpy(), want)
    for bad in (np.eye(3), torch.eye(4)[None]):
        with pytest.raises(_lib.IdhError):
            asset.place(bad)
    with pytest.raises(_lib.IdhError):
        raster.AssetRenderer(verts, faces, colors[:, :3], device="cpu")


# ---- PLY colours ----------------------------------------------------------------------------------------------------
def _write_ply(path, verts, faces, binary, colours=None, alpha=True):
    names = [] if colours is None else ["red", "green", "blue"] + (["alpha"] if alpha else [])
    head = (["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", f"element vertex {len(verts)}", "property float x",
             "property float y", "property float z"] + [f"property uchar {n}" for n in names] +
            [f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"])
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if binary:
            vt = np.zeros(len(verts), dtype=[("p", "<f4", (3,))] + ([("c", "u1", (len(names),))] if names else []))
            vt["p"] = verts
            if names:
                vt["c"] = colours[:, :len(names)]
            f.write(vt.tobytes())
            ft = np.zeros(len(faces), dtype=[("n", "u1"), ("i", "<i4", (3,))])
            ft["n"], ft["i"] = 3, faces
            f.write(ft.tobytes())
        else:
            for i, p in enumerate(verts):
                c = "" if colours is None else " " + " ".join(str(int(x)) for x in colours[i, :len(names)])
                f.write((" ".join(repr(float(x)) for x in p) + c + "\n").encode())
            for row in faces:
                f.write(("3 " + " ".join(str(int(i)) for i in row) + "\n").encode())


@pytest.mark.parametrize("binary", [False, True])
def test_load_ply_returns_vertex_colours(tmp_path, binary):
    from implicit_depth_amd import load_ply

    r = np.random.default_rng(5)
    verts = r.standard_normal((41, 3)).astype(np.float32)
    colours = r.integers(0, 256, (41, 4)).astype(np.uint8)
    colours[0], colours[1] = 0, 255
    faces = r.integers(0, 41, (63, 3)).astype(np.int64)
    for alpha in (True, False):
        path = tmp_path / f"rgb{'a' if alpha else ''}.ply"
        _write_ply(path, verts, faces, binary, colours, alpha)
        v, f, c = load_ply(str(path), return_colors=True)
        np.testing.assert_array_equal(v.numpy(), verts)
        np.testing.assert_array_equal(f.numpy(), faces)
        assert c.dtype == torch.uint8 and tuple(c.shape) == (41, 4)
        want = colours.copy()
        if not alpha:
            want[:, 3] = 255
        np.testing.assert_array_equal(c.numpy(), want)
        pair = load_ply(str(path))  # the default call returns the pair it always did
        assert len(pair) == 2 and torch.equal(pair[0], v) and torch.equal(pair[1], f)
    path = tmp_path / "plain.ply"
    _write_ply(path, verts, faces, binary)
    v, f, c = load_ply(str(path), return_colors=True)
    assert c is None and tuple(v.shape) == (41, 3) and tuple(f.shape) == (63, 3)
    assert len(load_ply(str(path))) == 2


def test_load_ply_refuses_colours_that_are_not_uchar(tmp_path):
    from implicit_depth_amd import load_ply

    path = tmp_path / "floatcol.ply"
    path.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nproperty float red\n"
                     b"property float green\nproperty float blue\nend_header\n0 0 0 0.5 0.5 0.5\n")
    with pytest.raises(ValueError, match="uchar"):
        load_ply(str(path), return_colors=True)
    assert len(load_ply(str(path))) == 2  # not asked for: skipped as any other property


# ---- the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1])
def test_reference_agrees_with_raster_ref_and_stays_under_the_ambiguity_cap(case):
    name, H, W, verts, faces, cams, K, refs = R.general_case(case)
    for b, ref in enumerate(refs):
        frac, zf = ref["ambiguous"].mean(), (ref["zfight"] & ~ref["edge_ambiguous"]).mean()
        print(f"{name} view {b}: ambiguous {frac:.4%} (edge lines {ref['edge_ambiguous'].mean():.4%}, z-fight alone {zf:.4%}), covered {ref['covered'].mean():.3f}")
        assert frac <= rr.AMBIGUOUS_CAP, (name, b, frac)
        # the same depth as raster_ref.render, which test_raster_gpu.py holds the depth-only path to
        np.testing.assert_array_equal(np.where(ref["covered"], ref["z"], -1.0), ref["depth"])
        assert (ref["face"][ref["covered"]] >= 0).all() and (ref["face"][~ref["covered"]] == -1).all()
        w = ref["bary"][ref["covered"]]
        assert np.abs(w.sum(-1) - 1.0).max() < 1e-12 and w.min() > -1e-9
        # the winning face's own plane gives the winning depth, and the second hit is never nearer
        own = R.face_depth(verts.numpy(), faces.numpy(), cams[b].numpy(), K[b].numpy(), H, W, ref["face"])
        assert np.abs(own[ref["covered"]] / ref["z"][ref["covered"]] - 1.0).max() < 1e-9
        assert (ref["z2"] >= ref["z"]).all()
        assert 0.0 < ref["lam"][ref["covered"]].min() and ref["lam"].max() <= 1.0 + 1e-12


def test_float32_restatement_is_close_to_the_reference():
    """The error baseline of the GPU tests is the float32 restatement's own distance from fp64: it must be a rounding-sized number."""
    name, H, W, verts, faces, cams, K, refs = R.general_case(1)
    ref = refs[0]
    m = ref["covered"] & ~ref["ambiguous"]
    ys, xs = np.nonzero(m)
    attrs, colors = R.vertex_attrs(len(verts), 3, 1), R.vertex_colors(len(verts), 2)
    got = R.restate_f32(verts.numpy(), faces.numpy(), cams[0].numpy(), K[0].numpy(), ys, xs, ref["face"][m], attrs=attrs, colors=colors, ambient=0.3)
    eb = np.abs(got["bary"].astype(np.float64) - ref["bary"][m]).max()
    ez = np.abs(got["z"].astype(np.float64) / ref["z"][m] - 1.0).max()
    el = np.abs(got["lam"].astype(np.float64) - ref["lam"][m]).max()
    ea = np.abs(got["attrs"].astype(np.float64) - R.interpolate(ref, faces.numpy(), attrs)[m]).max()
    ec = np.abs(got["colour"].astype(np.float64) - R.colour(ref, faces.numpy(), colors, 0.3)[m]).max()
    print(f"{name} view 0 float32 restatement: bary {eb:.2e}, rel depth {ez:.2e}, lam {el:.2e}, attrs {ea:.2e}, colour {ec:.2e} (of 255)")
    assert eb < 1e-4 and ez < 1e-4 and el < 1e-4 and ea < 1e-3 and ec < 0.05
