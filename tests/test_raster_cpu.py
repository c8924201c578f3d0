"""Host side of the mesh depth rasteriser and the temporal evaluation (include/idh_raster.h, raster.py, evaluation.TemporalEvaluator):
argument validation of the C entry points, the PLY reader, the plane mesh and the two host methods of TemporalEvaluator against the
reference's outputs (golden G15, tests/golden/gen_golden_temporal.py), and the ambiguity caps of the scenes test_raster_gpu.py renders
(computed by tests/raster_ref.py alone)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import raster_ref as rr
from conftest import load_golden

OK, EINVAL, EUNSUPPORTED, EWORKSPACE = 0, -1, -2, -4
P = 0x1000  # a non-null pointer that validation never dereferences


def test_entry_points_validate_on_the_host():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert L.idh_raster_workspace_bytes(1, 100, 50) >= 100 * 24 + 50 * 4 and L.idh_raster_workspace_bytes(1, 100, 50) % 256 == 0
    assert L.idh_raster_workspace_bytes(-1, 1, 1) == 0 and L.idh_raster_workspace_bytes(1, -1, 1) == 0 and L.idh_raster_workspace_bytes(1, 1, -1) == 0
    r = lambda **k: L.idh_raster_depth_fwd(*[{**dict(v=P, V=8, f=P, F=4, T=P, K=P, B=1, H=4, W=4, out=P, ws=P, n=1 << 20, st=None), **k}[a]
                                             for a in ("v", "V", "f", "F", "T", "K", "B", "H", "W", "out", "ws", "n", "st")])
    for bad in (dict(v=None), dict(f=None), dict(T=None), dict(K=None), dict(out=None), dict(H=0), dict(W=0), dict(H=0, W=0), dict(H=-3),
                dict(V=-1), dict(F=-1), dict(B=-1), dict(H=1 << 16, W=1 << 16)):
        assert r(**bad) == EINVAL, bad
    assert r(B=0) == OK and r(B=0, out=None) == OK  # nothing to do
    assert r(ws=None) == EWORKSPACE and r(n=64) == EWORKSPACE and r(ws=P + 8) == EWORKSPACE
    assert r(F=0, f=None, ws=None) == EWORKSPACE  # no faces is a valid request (all -1): it gets as far as the workspace check
    assert r(F=0, f=None, out=None) == EINVAL
    assert r(B=70000, n=1 << 30) == EUNSUPPORTED
    assert r(B=40000, H=256, W=256, n=1 << 30) == EUNSUPPORTED  # B * H * W >= 2^31
    vp = lambda **k: L.idh_vertex_predictions_fwd(*[{**dict(v=P, V=8, T=P, K=P, p=P, d=P, H=4, W=4, tol=0.05, out=P, st=None), **k}[a]
                                                    for a in ("v", "V", "T", "K", "p", "d", "H", "W", "tol", "out", "st")])
    for bad in (dict(v=None), dict(T=None), dict(K=None), dict(p=None), dict(d=None), dict(out=None), dict(H=0), dict(W=0), dict(V=-1)):
        assert vp(**bad) == EINVAL, bad
    assert vp(V=0) == OK
    assert L.idh_vertex_occlusion_changes_fwd(P, 3, 4, None, None) == EINVAL
    assert L.idh_vertex_occlusion_changes_fwd(None, 3, 4, P, None) == EINVAL
    assert L.idh_vertex_occlusion_changes_fwd(P, -1, 4, P, None) == EINVAL and L.idh_vertex_occlusion_changes_fwd(P, 3, -4, P, None) == EINVAL


def test_python_entry_points_refuse_cpu_tensors():
    from implicit_depth_amd import _lib, raster

    verts, faces, cams, K = syn.static_vertex_scene(16, 24)
    with pytest.raises(_lib.IdhError):
        raster.render_depth(verts, faces, cams, K, 16, 24)
    r = raster.MeshDepthRasterizer(16, 24)
    r.mesh = (verts, faces)
    with pytest.raises(_lib.IdhError):
        r(cams, K)
    with pytest.raises(_lib.IdhError):
        raster.vertex_predictions(verts, cams, K, torch.zeros(1, 1, 16, 24), torch.zeros(1, 1, 16, 24))
    with pytest.raises(_lib.IdhError):
        raster.vertex_occlusion_changes(torch.zeros(3, 5))
    with pytest.raises(ValueError):
        raster.MeshDepthRasterizer(16, 24)(cams, K)


# ---- PLY ---------------------------------------------------------------------------------------------------------
def _write_ply(path, verts, colours, faces, binary, count_type="uchar", index_type="int", face_flags=False):
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", "comment written by the test", f"element vertex {len(verts)}",
            "property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue",
            "property uchar alpha", f"element face {len(faces)}", f"property list {count_type} {index_type} vertex_indices"] + (["property uchar flags"] if face_flags else []) + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if binary:
            vt = np.zeros(len(verts), dtype=[("p", "<f4", (3,)), ("c", "u1", (4,))])
            vt["p"], vt["c"] = verts, colours
            f.write(vt.tobytes())
            n = faces.shape[1] if len(faces) else 3
            ft = np.zeros(len(faces), dtype=[("n", "<" + {"uchar": "u1", "int": "i4"}[count_type]), ("i", "<" + {"int": "i4", "uint": "u4"}[index_type], (n,))]
                          + ([("flags", "u1")] if face_flags else []))
            ft["n"], ft["i"] = n, faces
            if face_flags:
                ft["flags"] = 7
            f.write(ft.tobytes())
        else:
            for p, c in zip(verts, colours):
                f.write((" ".join(repr(float(x)) for x in p) + " " + " ".join(str(int(x)) for x in c) + "\n").encode())
            for row in faces:
                f.write((f"{len(row)} " + " ".join(str(int(i)) for i in row) + (" 7" if face_flags else "") + "\n").encode())


@pytest.mark.parametrize("binary", [False, True])
def test_load_ply_round_trips_a_coloured_mesh(tmp_path, binary):
    from implicit_depth_amd import load_ply

    r = np.random.default_rng(3)
    verts = r.standard_normal((57, 3)).astype(np.float32)
    colours = r.integers(0, 256, (57, 4)).astype(np.uint8)
    faces = r.integers(0, 57, (91, 3)).astype(np.int64)
    for ct, it in (("uchar", "int"), ("int", "uint")) if binary else (("uchar", "int"),):
        path = tmp_path / f"mesh_{ct}_{it}.ply"
        _write_ply(path, verts, colours, faces, binary, ct, it)
        v, f = load_ply(str(path))
        assert v.dtype == torch.float32 and f.dtype == torch.int64 and tuple(v.shape) == (57, 3) and tuple(f.shape) == (91, 3)
        np.testing.assert_array_equal(v.numpy(), verts)
        np.testing.assert_array_equal(f.numpy(), faces)
    quads = r.integers(0, 57, (5, 4)).astype(np.int64)
    path = tmp_path / "quads.ply"
    _write_ply(path, verts, colours, quads, binary)
    with pytest.raises(ValueError, match="triangle"):
        load_ply(str(path))
    # a scalar property beside the face list, as some exporters write; an unknown property type is named in the error
    path = tmp_path / "flags.ply"
    _write_ply(path, verts, colours, faces, binary, face_flags=True)
    v, f = load_ply(str(path))
    np.testing.assert_array_equal(v.numpy(), verts)
    np.testing.assert_array_equal(f.numpy(), faces)
    path = tmp_path / "badtype.ply"
    path.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty half x\nend_header\n0\n")
    with pytest.raises(ValueError, match="half"):
        load_ply(str(path))
    path = tmp_path / "not.ply"
    path.write_bytes(b"solid nothing\n")
    with pytest.raises(ValueError):
        load_ply(str(path))


# ---- golden G15 ----------------------------------------------------------------------------------------------------
def test_plane_mesh_equals_the_reference():
    from implicit_depth_amd.raster import MeshDepthRasterizer

    g = load_golden("g15_temporal")
    rows, stride = g["face_rows_index"], int(g["vert_stride"])
    r = MeshDepthRasterizer(192, 256)
    faces_before = None
    for i, dist in ((0, 2.0), (1, 3.25)):
        r.create_plane_from_camera(syn.plane_pose(i), distance=torch.tensor(dist))
        v, f = r.mesh
        assert tuple(v.shape) == (1024 * 1024, 3) and v.dtype == torch.float32 and tuple(f.shape) == (2 * 1023 * 1023, 3) and f.dtype == torch.int64
        np.testing.assert_array_equal(f[rows].numpy(), g[f"plane{i}_face_rows"])
        np.testing.assert_array_equal(f.sum(0).numpy(), g[f"plane{i}_face_colsum"])
        # the same float32 grid through the same matmul: bit for bit
        np.testing.assert_array_equal(v[::stride].numpy(), g[f"plane{i}_verts"])
        np.testing.assert_allclose(v.double().sum(0).numpy(), g[f"plane{i}_vert_sum"], rtol=1e-12)
        assert faces_before is None or f is faces_before  # built once
        faces_before = f


def test_temporal_evaluator_host_methods_equal_the_reference():
    from implicit_depth_amd import TemporalEvaluator, temporal_final_metrics

    g = load_golden("g15_temporal")
    for h, w in ((24, 32), (9, 20), (8, 8)):
        p = syn.randn((1, 1, h, w), 80, "edge_pred").clone()
        assert TemporalEvaluator.mask_prediction_edges(p) is None
        np.testing.assert_array_equal(p.numpy(), g[f"edges_{h}x{w}"])
    for T, V, seed in ((6, 500, 1), (2, 64, 2), (30, 2000, 3)):
        hist = syn.vertex_histories(T, V, seed)
        assert (hist == -1).any() and (hist == 0.5).any() and (hist > 0.5).any() and ((hist < 0.5) & (hist > 0)).any()
        ev = TemporalEvaluator()
        ev.rasterizer = types.SimpleNamespace(gt_vertex_predictions=list(hist))
        ev.compute_vertex_occlusion_changes()
        ev.compute_vertex_occlusion_changes()
        ref = g[f"changes_{T}x{V}_s{seed}"]
        assert float(ev.total_diffs) == ref[0] and ev.total_verts == ref[1]
        assert 2 * rr.occlusion_changes(hist.numpy()) == ref[0]  # the brute force agrees with the reference too
    m = temporal_final_metrics(120.0, eval_length=30, warmup=5, eval_frame_multiplier=4, n_scans=3)
    assert m == {"total_diffs_d_-1.0": 120.0, "temporal_score_d_-1.0": 120.0 / ((30 - 5) * 4 * 3)}


# ---- the GPU tests' scenes stay under their ambiguity caps -------------------------------------------------------------
def test_general_scenes_stay_under_the_ambiguity_cap():
    for name, H, W, verts, faces, cams, K in rr.general_cases():
        assert len(faces) > 3000
        for b in range(2):
            depth, amb = rr.render(verts.numpy(), faces.numpy(), cams[b].numpy(), K[b].numpy(), H, W)
            frac = amb.mean()
            print(f"{name} view {b}: ambiguous {frac:.4%}, covered {np.mean(depth > 0):.3f}")
            assert frac <= rr.AMBIGUOUS_CAP, (name, b, frac)
            assert 0.5 < np.mean(depth > 0) < 1.0  # both covered and empty pixels are exercised


def test_vertex_scenes_stay_under_the_ambiguity_cap():
    verts, faces, cams, K, preds = rr.track_case()
    out, amb = rr.track_reference(verts, faces, cams, K, preds)
    print(f"track: ambiguous vertices per frame {amb.mean(1)}, sampled {np.mean(out > 0):.3f}, flips {rr.occlusion_changes(out)}")
    assert (amb.mean(1) <= rr.AMBIGUOUS_CAP).all(), amb.mean(1)
    assert (out > 0).sum() > 200 and rr.occlusion_changes(out) > 10  # enough visible samples and flips to mean something
    verts, faces, cams, K, preds = rr.static_case()
    out, amb = rr.track_reference(verts, faces, cams, K, preds)
    assert amb.sum() == 0, int(amb.sum())
    assert rr.occlusion_changes(out) > 10 and 0.2 < np.mean(out > 0) < 0.6
