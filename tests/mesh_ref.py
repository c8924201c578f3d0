"""Vectorised numpy statement of the TSDF mesh extraction (include/idh_fusion.h: idh_tsdf_mesh_count_fwd / _emit_fwd),
written from the header and independent of the kernels.  The input is the float32 pair tensor the kernels are given; topology comes from
comparisons of the stored values, so faces and vertex counts are exact; positions and weights are evaluated in float64.  No Python loop
runs over cells.  The case table is imported from the generator (tools/gen_mc_table.py).

The second half holds checks that do not depend on the table being right: directed-edge counting, signed volume per connected
component, the Euler characteristic, and "every vertex lies on a grid edge whose endpoints differ in sign"."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_mc_table as G  # noqa: E402

TRI_COUNT = np.array(G.TRI_COUNT, np.int64)
TRI_EDGES = np.zeros((256, G.MAX_TRIS, 3), np.int64)
for _case, _tris in enumerate(G.TABLE):
    for _t, _tri in enumerate(_tris):
        TRI_EDGES[_case, _t] = _tri
# per cube edge: its axis and the (dz, dy, dx) of its lower corner
EDGE_AXIS = np.arange(12) // 4
EDGE_LOW = np.array([G.edge_corners(e)[0][::-1] for e in range(12)], np.int64)


def position_bound(origin, voxel_size, dims):
    """include/idh_fusion.h's vertex arithmetic against fp64: each component takes at most four fp32 roundings at the magnitude of the
    largest coordinate in the scene, plus voxel_size * 2^-22 for the rounding of r."""
    o, v = np.asarray(origin, np.float64), float(voxel_size)
    far = np.abs(np.stack([o, o + v * (np.array(dims[::-1]) - 1)])).max()
    return 4 * 2.0 ** -23 * far + v * 2.0 ** -22


def case_volume(inner=0.5):
    """The all-cases volume: dims (4, 4, 1024); brick k (x in [4k, 4k + 4)) holds case k in its inner 2 x 2 x 2 as -+inner, everything
    else is {1, 1}."""
    vals = np.ones((4, 4, 1024, 2), np.float32)
    for k in range(256):
        for c in range(8):
            dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
            vals[1 + dz, 1 + dy, 4 * k + 1 + dx, 0] = -inner if (k >> c) & 1 else inner
    return vals


def sphere_volume(dims, centre, radius, trunc=3.0, weight=1.0):
    """T = clip((|p - centre| - radius) / trunc, -1, 1) in voxel units (centre as (x, y, z)), W = weight."""
    zz, yy, xx = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in dims), indexing="ij")
    d = np.sqrt((xx - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (zz - centre[2]) ** 2) - radius
    vals = np.empty((*dims, 2), np.float32)
    vals[..., 0], vals[..., 1] = np.clip(d / trunc, -1, 1), weight
    return vals


def extract(values, origin, voxel_size, min_weight=0.0):
    """dict: ``verts`` (V,3) float64, ``faces`` (F,3) int64, ``weights`` (V,) float64, ``owner`` (V,) linear voxel index and ``axis`` (V,)
    of every vertex, ``cell`` (F,) the linear index of every face's cell, ``known`` (Nz-1,Ny-1,Nx-1) bool, ``emitted`` likewise."""
    values = np.asarray(values)
    assert values.dtype == np.float32 and values.ndim == 4 and values.shape[3] == 2
    Nz, Ny, Nx = values.shape[:3]
    n = Nz * Ny * Nx
    T, W = values[..., 0], values[..., 1]
    inside, kv = T <= 0, W > np.float32(min_weight)
    known = np.ones((Nz - 1, Ny - 1, Nx - 1), bool)
    case = np.zeros((Nz - 1, Ny - 1, Nx - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        sl = (slice(dz, Nz - 1 + dz), slice(dy, Ny - 1 + dy), slice(dx, Nx - 1 + dx))
        known &= kv[sl]
        case |= inside[sl].astype(np.int64) << c
    emitted = known & (case != 0) & (case != 255)
    # Ep[z + 1, y + 1, x + 1] = emitted[z, y, x]; False where there is no cell
    Ep = np.zeros((Nz + 1, Ny + 1, Nx + 1), bool)
    Ep[1:Nz, 1:Ny, 1:Nx] = emitted
    used = np.zeros((Nz, Ny, Nx, 3), bool)
    for axis in range(3):
        lo = [slice(None)] * 3  # (z, y, x) slices of the owners that have a neighbour along the axis
        hi = [slice(None)] * 3
        lo[2 - axis], hi[2 - axis] = slice(0, -1), slice(1, None)
        crossed = inside[tuple(lo)] != inside[tuple(hi)]
        any_cell = np.zeros_like(crossed)
        others = [a for a in range(3) if a != axis]
        for d0 in (0, 1):
            for d1 in (0, 1):
                sl = [None] * 3
                sl[2 - axis] = slice(1, (Nx, Ny, Nz)[axis])
                for a, d in zip(others, (d0, d1)):
                    sl[2 - a] = slice(1 - d, (Nx, Ny, Nz)[a] + 1 - d)
                any_cell |= Ep[tuple(sl)]
        used[tuple(lo) + (axis,)] = crossed & any_cell
    flat = used.reshape(n, 3)
    vidx = (np.cumsum(flat.reshape(-1)) - 1).reshape(n, 3)
    owner, axis = np.nonzero(flat)
    V = len(owner)
    stride = np.array([1, Nx, Nx * Ny])
    Tf, Wf = T.reshape(-1).astype(np.float64), W.reshape(-1).astype(np.float64)
    Ta, Tb, Wa, Wb = Tf[owner], Tf[owner + stride[axis]], Wf[owner], Wf[owner + stride[axis]]
    r = Ta / (Ta - Tb)
    idx = np.stack([owner % Nx, (owner // Nx) % Ny, owner // (Nx * Ny)], 1).astype(np.float64)
    idx[np.arange(V), axis] += r
    o, v = np.asarray(origin, np.float32).astype(np.float64), float(np.float32(voxel_size))
    verts = o[None] + v * idx
    weights = Wa + r * (Wb - Wa)
    cz, cy, cx = np.nonzero(emitted)
    cell = (cz * Ny + cy) * Nx + cx
    cc = case[cz, cy, cx]
    edges = TRI_EDGES[cc]  # (cells, 5, 3)
    low = EDGE_LOW[edges]  # (cells, 5, 3, 3)
    own = cell[:, None, None] + low[..., 2] + low[..., 1] * Nx + low[..., 0] * Nx * Ny
    live = np.arange(G.MAX_TRIS)[None] < TRI_COUNT[cc][:, None]
    own, eax = own[live], EDGE_AXIS[edges][live]
    assert flat[own, eax].all()  # every face vertex exists
    faces = vidx[own, eax]
    if len(faces):
        assert len(np.unique(faces)) == V  # no orphan vertices
    return dict(verts=verts, faces=faces.reshape(-1, 3), weights=weights, owner=owner, axis=axis, cell=np.repeat(cell, TRI_COUNT[cc]),
                known=known, emitted=emitted)


# ---- checks that do not use the table ---------------------------------------------------------------------------------------
def directed_edges(faces, V):
    """Unique directed edges a -> b as keys a * V + b, their counts, and the counts of their reverses."""
    f = np.asarray(faces, np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    keys, counts = np.unique(a * V + b, return_counts=True)
    rev = (keys % V) * V + keys // V
    pos = np.searchsorted(keys, rev)
    pos_c = np.minimum(pos, len(keys) - 1)
    rcounts = np.where(keys[pos_c] == rev, counts[pos_c], 0) if len(keys) else counts
    return keys, counts, rcounts


def euler_characteristic(faces, V):
    f = np.asarray(faces, np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    E = len(np.unique(np.minimum(a, b) * V + np.maximum(a, b)))
    return V - E + len(f)


def components(faces, V):
    """(V,) label per vertex: the smallest vertex index of its connected component."""
    f = np.asarray(faces, np.int64)
    lab = np.arange(V)
    while True:
        m = lab[f].min(1)
        new = lab.copy()
        for k in range(3):
            np.minimum.at(new, f[:, k], m)
        new = new[new]
        if (new == lab).all():
            return lab
        lab = new


def signed_volumes(verts, faces):
    """{component label: signed volume}: the sum of v0 . (v1 x v2) / 6 over the component's faces, taken about the mesh's centroid."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    lab = components(f, len(v))
    p = v - v.mean(0)
    vol = np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])) / 6
    return {int(L): float(vol[lab[f[:, 0]] == L].sum()) for L in np.unique(lab[f[:, 0]])}


def vertices_on_crossed_edges(verts, values, origin, voxel_size, tol=1e-4):
    """(V,) bool: the vertex lies (within tol voxels) on a grid edge whose two endpoints differ in T <= 0."""
    values = np.asarray(values)
    dims = np.array(values.shape[:3])[::-1]  # (Nx, Ny, Nz)
    inside = values[..., 0] <= 0
    g = (np.asarray(verts, np.float64) - np.asarray(origin, np.float32).astype(np.float64)) / float(np.float32(voxel_size))
    ok = np.zeros(len(g), bool)
    for axis in range(3):
        others = [a for a in range(3) if a != axis]
        near = np.rint(g)
        on_line = (np.abs(g[:, others] - near[:, others]) < tol).all(1)
        for shift in (0, -1):
            lo = np.floor(g[:, axis]) + shift
            a = near.copy()
            a[:, axis] = lo
            b = a.copy()
            b[:, axis] += 1
            inb = (a >= 0).all(1) & (b < dims).all(1) & on_line & (g[:, axis] >= lo - tol) & (g[:, axis] <= lo + 1 + tol)
            ai, bi = a[inb].astype(np.int64), b[inb].astype(np.int64)
            hit = inside[ai[:, 2], ai[:, 1], ai[:, 0]] != inside[bi[:, 2], bi[:, 1], bi[:, 0]]
            ok[np.nonzero(inb)[0][hit]] = True
    return ok
