"""Mesh extraction from the TSDF volume (include/idh_fusion.h), what holds without a GPU: the generated case table, the
numpy reference (tests/mesh_ref.py) judged by checks that do not use the table, the host-side validation of the two C entry points, and
the PLY writer."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import mesh_ref as M
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_mc_table as G  # noqa: E402


def test_committed_table_is_the_generators_output():
    with open(os.path.join(ROOT, "implicit-depth_amd", "csrc", "mc_table.h")) as f:
        assert f.read() == G.render()


def test_table_check_values():
    assert max(G.TRI_COUNT) == 5 and sum(G.TRI_COUNT) == 820
    assert {k: G.TRI_COUNT.count(k) for k in range(6)} == {0: 2, 1: 16, 2: 50, 3: 80, 4: 76, 5: 32}
    assert G.TRI_COUNT[0] == 0 and G.TRI_COUNT[255] == 0
    assert G.in_face_diagonals() == 36
    for case in range(256):
        crossed = G.crossed_edges(case)
        assert crossed == G.crossed_edges(255 - case)  # the complement crosses the same edges
        used = sorted({e for t in G.TABLE[case] for e in t})
        assert used == crossed, case                   # every crossed edge carries a vertex of the case, no other does
        assert all(len(set(t)) == 3 for t in G.TABLE[case])


def test_edge_numbering_is_the_headers():
    # e = 4 * axis + j, j = first + 2 * second of the lower corner's other two coordinates in x < y < z order
    assert G.edge_corners(0) == ((0, 0, 0), (1, 0, 0)) and G.edge_corners(3) == ((0, 1, 1), (1, 1, 1))
    assert G.edge_corners(5) == ((1, 0, 0), (1, 1, 0)) and G.edge_corners(6) == ((0, 0, 1), (0, 1, 1))
    assert G.edge_corners(9) == ((1, 0, 0), (1, 0, 1)) and G.edge_corners(10) == ((0, 1, 0), (0, 1, 1))
    for e in range(12):
        assert G.edge_id(*G.edge_corners(e)) == e
    assert G.TABLE[1] == [(0, 4, 8)]


def _noise_volume():
    """12^3: Gaussian noise inside, a positive shell, everything known."""
    vals = np.ones((12, 12, 12, 2), np.float32)
    vals[1:-1, 1:-1, 1:-1, 0] = np.random.default_rng(7).standard_normal((10, 10, 10)).astype(np.float32)
    return vals


@pytest.mark.parametrize("name", ["all_cases", "noise"])
def test_every_directed_edge_is_used_as_often_as_its_reverse(name):
    vals = M.case_volume() if name == "all_cases" else _noise_volume()
    r = M.extract(vals, (0, 0, 0), 1.0)
    V = len(r["verts"])
    keys, counts, rcounts = M.directed_edges(r["faces"], V)
    print(f"{name}: V = {V}, F = {len(r['faces'])}, directed edges by multiplicity {np.bincount(counts).tolist()}")
    assert len(r["faces"]) > 500
    assert (counts == rcounts).all()  # zero boundary
    assert counts.max() <= 2
    assert M.vertices_on_crossed_edges(r["verts"], vals, (0, 0, 0), 1.0).all()
    vols = M.signed_volumes(r["verts"], r["faces"])
    if name == "all_cases":  # one closed surface (or several) per brick round its inside corners
        assert (counts == 1).all() and min(vols.values()) > 0
        assert len(r["faces"]) == sum(G.TRI_COUNT[k] + sum(G.TRI_COUNT[c] for c in _neighbour_cases(k)) for k in range(256))
    else:
        assert sum(vols.values()) > 0


def _neighbour_cases(k):
    """The cases of the 26 cells round the inner cell of brick k that see some of its corners (the rest of their corners are outside)."""
    out = []
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                if (ox, oy, oz) == (0, 0, 0):
                    continue
                case = 0
                for c in range(8):
                    x, y, z = ox + (c & 1), oy + ((c >> 1) & 1), oz + (c >> 2)
                    if 0 <= x <= 1 and 0 <= y <= 1 and 0 <= z <= 1 and (k >> (x + 2 * y + 4 * z)) & 1:
                        case |= 1 << c
                out.append(case)
    return out


def test_sphere_is_a_closed_manifold_with_positive_volume():
    vals = M.sphere_volume((20, 20, 20), (9.3, 10.1, 8.7), 6.3)
    origin, v = (-0.4, 0.2, 1.0), 0.05
    r = M.extract(vals, origin, v)
    V, F = len(r["verts"]), len(r["faces"])
    keys, counts, rcounts = M.directed_edges(r["faces"], V)
    vols = M.signed_volumes(r["verts"], r["faces"])
    ball = 4 / 3 * np.pi * (6.3 * v) ** 3
    print(f"sphere: V = {V}, F = {F}, volume {sum(vols.values()):.6g} against the ball's {ball:.6g}")
    assert (counts == 1).all() and (rcounts == 1).all()
    assert M.euler_characteristic(r["faces"], V) == 2 and len(vols) == 1
    assert 0.97 * ball < sum(vols.values()) < ball  # the chords of a convex surface lie inside it
    assert M.vertices_on_crossed_edges(r["verts"], vals, origin, v).all()
    # weights interpolate like positions; min_weight removes cells
    assert (r["weights"] == 1).all()
    vals[:8, :8, :8, 1] = 0
    cut = M.extract(vals, origin, v)
    assert 0 < len(cut["faces"]) < F and not cut["known"][:8, :8, :8].any()
    assert len(M.extract(vals, origin, v, min_weight=1.0)["faces"]) == 0


def _workspace_bytes(n):
    n4 = (n + 3) // 4 * 4
    total, p = 8 * n4, n4
    while True:
        p = -(-p // 1024)
        total += 8 * p
        if p <= 1024:
            return total


def _good_args():
    from implicit_depth_amd import _lib

    a, v = _lib.TsdfMeshArgs(), _lib.TsdfVolume()
    v.values, v.block_flags, v.block_flag_bytes = 0x10000, 0x20000, 3 * 4 * 5
    v.voxel_size, v.trunc_voxels, v.Nz, v.Ny, v.Nx = 0.05, 3.0, 20, 28, 36
    a.volume = v
    a.workspace, a.workspace_bytes = 0x30000, _workspace_bytes(20 * 28 * 36)
    a.totals, a.verts_v3, a.faces_f3 = 0x40000, 0x50000, 0x60000
    a.vert_capacity, a.face_capacity, a.min_weight = 10, 10, 0.0
    return a


def test_abi_sizes_workspace_formula_and_error_codes():
    """Validation happens on the host before any launch, so every refusal is returned without a GPU."""
    from implicit_depth_amd import _lib

    L = _lib.lib()
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
    assert L.idh_sizeof_tsdf_mesh_args() == C.sizeof(_lib.TsdfMeshArgs) == _lib.TsdfMeshArgs().struct_size
    for dims in ((2, 2, 2), (20, 28, 36), (23, 37, 131), (4, 4, 1024), (104, 104, 104), (96, 256, 256), (1024, 512, 512)):
        assert L.idh_tsdf_mesh_workspace_bytes(*dims) == _workspace_bytes(dims[0] * dims[1] * dims[2]), dims
    assert L.idh_tsdf_mesh_workspace_bytes(104, 104, 104) > 8 * 104 ** 3 + 8 * 1099  # a second level of partial sums
    assert L.idh_tsdf_mesh_workspace_bytes(1, 28, 36) == 0 and L.idh_tsdf_mesh_workspace_bytes(1024, 512, 513) == 0

    def run(fn, **edits):
        a = _good_args()
        for k, x in edits.items():
            obj = a.volume if k in ("values", "block_flags", "block_flag_bytes", "voxel_size", "Nz", "Ny", "Nx") else a
            setattr(obj, k, x)
        return fn(C.byref(a), None)

    for fn in (L.idh_tsdf_mesh_count_fwd, L.idh_tsdf_mesh_emit_fwd):
        assert fn(None, None) == EINVAL
        assert run(fn, struct_size=8) == EINVAL
        assert run(fn, min_weight=-0.5) == EINVAL and run(fn, min_weight=float("nan")) == EINVAL
        assert run(fn, values=None) == EINVAL and run(fn, Nx=1) == EINVAL and run(fn, voxel_size=0.0) == EINVAL  # the volume's conditions
        assert run(fn, block_flags=None) == EWORKSPACE and run(fn, block_flag_bytes=59) == EWORKSPACE
        assert run(fn, Nz=1024, Ny=512, Nx=513, block_flag_bytes=1 << 30, workspace_bytes=1 << 40) == EUNSUPPORTED  # one voxel row past 2^28
        assert run(fn, workspace=None) == EWORKSPACE
        assert run(fn, workspace_bytes=_workspace_bytes(20 * 28 * 36) - 1) == EWORKSPACE and run(fn, workspace_bytes=-1) == EWORKSPACE
        assert run(fn, workspace=0x30008) == EINVAL  # not 16-byte aligned
        # the order: an argument of the call before the volume, the volume before the workspace
        assert run(fn, min_weight=-1.0, Nx=1, workspace=None) == EINVAL
        assert run(fn, block_flags=None, workspace=None, Nz=1024, Ny=512, Nx=513) == EWORKSPACE  # the flags are the volume's
    assert run(L.idh_tsdf_mesh_count_fwd, totals=None) == EINVAL
    assert run(L.idh_tsdf_mesh_emit_fwd, verts_v3=None) == EINVAL and run(L.idh_tsdf_mesh_emit_fwd, faces_f3=None) == EINVAL
    assert run(L.idh_tsdf_mesh_emit_fwd, vert_capacity=-1) == EINVAL and run(L.idh_tsdf_mesh_emit_fwd, face_capacity=-1) == EINVAL
    assert run(L.idh_tsdf_mesh_emit_fwd, vert_capacity=0, face_capacity=0) == 0  # nothing to write: nothing is launched
    assert run(L.idh_tsdf_mesh_emit_fwd, totals=None, vert_capacity=0, face_capacity=0) == 0  # emit does not read the totals


@pytest.mark.parametrize("colors", [None, 3, 4])
def test_save_ply_round_trip_is_exact(tmp_path, colors):
    from implicit_depth_amd import raster

    r = M.extract(M.sphere_volume((9, 10, 11), (5.2, 4.6, 4.1), 2.7), (0.3, -1.2, 2.0), 0.04)
    verts, faces = torch.from_numpy(r["verts"].astype(np.float32)), torch.from_numpy(r["faces"].astype(np.int32))
    col = None if colors is None else torch.from_numpy(np.random.default_rng(1).integers(0, 256, (len(verts), colors), dtype=np.uint8))
    path = str(tmp_path / "mesh.ply")
    raster.save_ply(path, verts, faces, col)
    v2, f2, c2 = raster.load_ply(path, return_colors=True)
    assert v2.dtype == torch.float32 and torch.equal(v2, verts)
    assert f2.dtype == torch.int64 and torch.equal(f2, faces.long())
    if colors is None:
        assert c2 is None
    else:
        assert torch.equal(c2[:, :colors], col) and (colors == 4 or (c2[:, 3] == 255).all())
    # an empty mesh
    raster.save_ply(path, torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32))
    v0, f0 = raster.load_ply(path)
    assert tuple(v0.shape) == (0, 3) and tuple(f0.shape) == (0, 3)
    with pytest.raises(ValueError):
        raster.save_ply(path, verts, faces + len(verts))
