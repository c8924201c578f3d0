"""fp64 numpy statement of the TSDF fusion's semantics (include/idh_fusion.h: idh_tsdf_integrate_fwd, idh_tsdf_raycast_fwd; DESIGN.md
§4.21), written from the header and independent of the kernels.  The inputs are the float32 arrays the kernels are given; everything
is evaluated in float64 from those values, except what the kernel's fp32 arithmetic restates exactly: the weights (small integers) and
the ``min(W + 1, max_weight)`` cap, kept in ``np.float32``.

Both functions also say what is *ambiguous*: what another fp32 implementation may decide the other way.  With u = 2^-24 (the relative
rounding of one fp32 operation) and MARGIN = 4 between a worst-case rounding bound and the mask built from it:

Voxel (``integrate``).  p = origin + v (x, y, z) and c = R p + t take 8 roundings on partial results no larger than
S = |R| |p| + |t| (per row), so each component of c is within dc = 8 u S of its fp64 value.  The voxel is ambiguous when in any map
  * |c.z| < EPS_Z = MARGIN dc.z                                                         (the c.z > 0 test), or
  * px (or py) is within EPS_PX of an integer, EPS_PX = MARGIN (fx (dc.x + |c.x / c.z| dc.z) / c.z + 3 u (|fx c.x / c.z| + |px|)):
    the quotient's error from its operands, and three more roundings (divide, multiply, add) on the magnitudes they produce
                                                                                        (the pixel borders of the nearest tap), or
  * |sdf + trunc| < EPS_SDF = MARGIN (dc.z + 2 u (|d| + |c.z|) + 2 u trunc): c.z's error, the subtraction's rounding, and the rounding of
    trunc = trunc_voxels * v itself                                                     (the truncation test).
Typical values at the committed scenes: EPS_Z 1e-5 m, EPS_PX 1e-4 px, EPS_SDF 1e-5 m.

Pixel (``raycast``).  g = og + t dg in voxel units: og = (o - origin) / v (2 roundings at magnitude G = the largest |g| along the ray),
t = near + k step (2 roundings), dg = R (q / |q|) / v (about 10 roundings, relative), t dg and the sum (2 more): within
dg_err = 16 u G of the fp64 value, G <= 64 at the committed scenes: 6.1e-5 voxels.
  * EPS_VOX = MARGIN 16 u 64 = 2.5e-4 voxels: a sample this close to a cell face across which knownness differs is ambiguous;
  * inside a cell the interpolant's slope along an axis is at most the largest difference D_axis between corners that are neighbours
    along it, so f moves by at most dg_err (D_x + D_y + D_z), and the seven lerps add 14 u:
    EPS_F = MARGIN (dg_err (D_x + D_y + D_z) + 14 u), per sample, about 1.5e-4 on a surface of slope 1 / trunc_voxels: a known sample
    with |f| < EPS_F is ambiguous (the sign tests of the hit rule).
For the normals, which the header defines by the cell that holds the hit point, ``normal_ambiguous`` further marks hits within EPS_VOX of
any cell face (the gradient is discontinuous there) or whose gradient is shorter than 0.05 (the rounding of the differences, 1e-6,
relative to the length, then exceeds the 1e-3 bound's MARGIN)."""
import functools

import numpy as np

U = 2.0 ** -24
MARGIN = 4.0
EPS_VOX = MARGIN * 16 * U * 64
MIN_GRADIENT = 0.05
CAP = 0.01  # the share of touched voxels / of pixels a GPU test may leave out

HIT, NONE_KNOWN, SOME_KNOWN, NO_NORMAL = 1, 2, 4, 8


def empty_volume(dims):
    v = np.zeros((*dims, 2), np.float32)
    v[..., 0] = 1
    return v


def trunc_of(trunc_voxels, voxel_size):
    return float(np.float32(trunc_voxels) * np.float32(voxel_size))


def integrate(values, depths, Ks, cam_T_worlds, origin, voxel_size, trunc_voxels=3.0, max_weight=64.0):
    """``values`` (Nz,Ny,Nx,2) float32 before; M maps.  Returns dict: ``T`` (Nz,Ny,Nx) fp64, ``W`` float32, ``touched`` bool (some map
    updated the voxel), ``ambiguous`` bool, and per-map counts ``behind`` (skipped by the truncation), ``outside`` (c.z <= 0 or off the
    image), ``invalid`` (tap not finite and positive)."""
    values = np.asarray(values)
    assert values.dtype == np.float32
    Nz, Ny, Nx = values.shape[:3]
    T = values[..., 0].astype(np.float64)
    W = values[..., 1].copy()
    v = float(np.float32(voxel_size))
    o = np.asarray(origin, np.float32).astype(np.float64)
    trunc = trunc_of(trunc_voxels, voxel_size)
    zz, yy, xx = np.meshgrid(np.arange(Nz), np.arange(Ny), np.arange(Nx), indexing="ij")
    p = np.stack([o[0] + v * xx, o[1] + v * yy, o[2] + v * zz], -1)
    touched = np.zeros((Nz, Ny, Nx), bool)
    amb = np.zeros((Nz, Ny, Nx), bool)
    stats = dict(behind=0, outside=0, invalid=0)
    for depth, K, E in zip(depths, Ks, cam_T_worlds):
        d32 = np.asarray(depth, np.float32).reshape(depth.shape[-2:])
        h, w = d32.shape
        K, E = np.asarray(K, np.float32).astype(np.float64), np.asarray(E, np.float32).astype(np.float64)
        c = p @ E[:3, :3].T + E[:3, 3]
        dc = 8 * U * (np.abs(p) @ np.abs(E[:3, :3]).T + np.abs(E[:3, 3]))
        amb |= np.abs(c[..., 2]) < MARGIN * dc[..., 2]
        front = c[..., 2] > 0
        cz = np.where(front, c[..., 2], 1.0)
        rx, ry = c[..., 0] / cz, c[..., 1] / cz
        px, py = K[0, 0] * rx + K[0, 2], K[1, 1] * ry + K[1, 2]
        ex = MARGIN * (K[0, 0] * (dc[..., 0] + np.abs(rx) * dc[..., 2]) / cz + 3 * U * (np.abs(K[0, 0] * rx) + np.abs(px)))
        ey = MARGIN * (K[1, 1] * (dc[..., 1] + np.abs(ry) * dc[..., 2]) / cz + 3 * U * (np.abs(K[1, 1] * ry) + np.abs(py)))
        near_image = front & (px > -1) & (px < w + 1) & (py > -1) & (py < h + 1)
        amb |= near_image & ((np.abs(px - np.rint(px)) < ex) | (np.abs(py - np.rint(py)) < ey))
        inside = front & (px >= 0) & (px < w) & (py >= 0) & (py < h)
        j = np.where(inside, np.floor(px), 0).astype(np.int64)
        i = np.where(inside, np.floor(py), 0).astype(np.int64)
        d = d32[i, j]
        ok = inside & np.isfinite(d) & (d > 0)
        dd = np.where(ok, d, 1.0).astype(np.float64)
        sdf = dd - c[..., 2]
        amb |= ok & (np.abs(sdf + trunc) < MARGIN * (dc[..., 2] + 2 * U * (dd + np.abs(c[..., 2])) + 2 * U * trunc))
        upd = ok & ~(sdf < -trunc)
        s = np.minimum(1.0, sdf / trunc)
        W64 = W.astype(np.float64)
        T = np.where(upd, (W64 * T + s) / (W64 + 1), T)
        W = np.where(upd, np.minimum(W + np.float32(1), np.float32(max_weight)), W)
        assert W.dtype == np.float32
        touched |= upd
        stats["behind"] += int((ok & ~upd).sum())
        stats["outside"] += int((~inside).sum())
        stats["invalid"] += int((inside & ~ok).sum())
    return dict(T=T, W=W, touched=touched, ambiguous=amb, **stats)


def known_cells(values):
    """(Nz-1,Ny-1,Nx-1) bool: all eight corners of the cell have W > 0."""
    s = np.asarray(values)[..., 1] > 0
    k = s[:-1] & s[1:]
    k = k[:, :-1] & k[:, 1:]
    return k[:, :, :-1] & k[:, :, 1:]


def block_flags(values):
    """The header's block flags, (NBz,NBy,NBx) uint8 over 8-cell blocks: 1 iff some voxel a cell of the block reads has W > 0; and the
    same for "W > 0 and T < 1", the set the flags must at least hold."""
    values = np.asarray(values)
    dims = values.shape[:3]
    nb = [(n + 6) // 8 for n in dims]
    seen, surf = values[..., 1] > 0, (values[..., 1] > 0) & (values[..., 0] < 1)
    out = [np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)]
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                box = tuple(slice(8 * b, 8 * b + 9) for b in (bz, by, bx))
                out[0][bz, by, bx], out[1][bz, by, bx] = seen[box].any(), surf[box].any()
    return out[0], out[1]


class _Grid:
    def __init__(self, values):
        self.T = np.asarray(values)[..., 0].astype(np.float64)
        self.known = known_cells(values)
        self.n = np.array(self.known.shape)  # cells per axis (z, y, x)

    def is_known(self, cz, cy, cx):
        ok = (cz >= 0) & (cz < self.n[0]) & (cy >= 0) & (cy < self.n[1]) & (cx >= 0) & (cx < self.n[2])
        out = np.zeros(ok.shape, bool)
        out[ok] = self.known[cz[ok], cy[ok], cx[ok]]
        return out

    def corners(self, cz, cy, cx):
        """T at the eight corners, indexed [dz][dy][dx] (cells must be in range)."""
        return [[[self.T[cz + a, cy + b, cx + c] for c in (0, 1)] for b in (0, 1)] for a in (0, 1)]


def _lerp(a, b, r):
    return a + r * (b - a)


def raycast(values, origin, voxel_size, world_T_cam, invK, H, W, near=0.25, step_voxels=1.0, max_steps=64, empty_depth=-1.0,
            world_normals=True):
    """The plain march over every sample for one camera.  Returns dict: ``depth`` (H,W) fp64, ``flags`` (H,W) uint8 (bit 8 as if normals
    were asked), ``normals`` (3,H,W), ``ambiguous`` (H,W) bool, ``normal_ambiguous`` (H,W) bool, ``hit_cell`` (H,W,3) int (z, y, x; -1),
    ``missed`` (H,W) bool: no sample of the ray lies inside the volume's cells."""
    values = np.asarray(values)
    assert values.dtype == np.float32
    G = _Grid(values)
    v = float(np.float32(voxel_size))
    o = np.asarray(origin, np.float32).astype(np.float64)
    E, iK = np.asarray(world_T_cam, np.float32).astype(np.float64), np.asarray(invK, np.float32).astype(np.float64)
    step = float(np.float32(step_voxels) * np.float32(voxel_size))
    near = float(np.float32(near))
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    q = np.stack([jj + 0.5, ii + 0.5, np.ones((H, W))], -1).reshape(-1, 3) @ iK[:3, :3].T
    dc = q / np.linalg.norm(q, axis=1, keepdims=True)
    dirw = dc @ E[:3, :3].T
    og, dg = (E[:3, 3] - o) / v, dirw / v
    P = H * W
    active = np.ones(P, bool)
    hit = np.zeros(P, bool)
    t_star = np.zeros(P)
    n_known = np.zeros(P, np.int64)
    n_total = np.full(P, max_steps, np.int64)
    prev_known = np.zeros(P, bool)
    f_prev = np.zeros(P)
    amb = np.zeros(P, bool)
    entered = np.zeros(P, bool)

    def sample(g):
        cell = np.floor(g).astype(np.int64)
        cx, cy, cz = cell[:, 0], cell[:, 1], cell[:, 2]
        kn = G.is_known(cz, cy, cx)
        r = g - cell
        f, eps_f = np.zeros(len(g)), np.zeros(len(g))
        if kn.any():
            c = G.corners(cz[kn], cy[kn], cx[kn])
            rx, ry, rz = r[kn, 0], r[kn, 1], r[kn, 2]
            a = [[_lerp(c[z][y][0], c[z][y][1], rx) for y in (0, 1)] for z in (0, 1)]
            f[kn] = _lerp(_lerp(a[0][0], a[0][1], ry), _lerp(a[1][0], a[1][1], ry), rz)
            c = np.array(c)  # [z][y][x][sample]
            spread = sum(np.abs(np.diff(c, axis=ax)).max(axis=(0, 1, 2)) for ax in (0, 1, 2))
            eps_f[kn] = MARGIN * (16 * U * 64 * spread + 14 * U)
        return cell, r, kn, f, eps_f

    for k in range(max_steps):
        if not active.any():
            break
        t = near + k * step
        g = og + t * dg
        cell, r, kn, f, eps_f = sample(g)
        cx, cy, cz = cell[:, 0], cell[:, 1], cell[:, 2]
        entered |= active & (cz >= 0) & (cz < G.n[0]) & (cy >= 0) & (cy < G.n[1]) & (cx >= 0) & (cx < G.n[2])
        a_k = kn & (np.abs(f) < eps_f)
        for ax, (dz, dy, dx) in enumerate(((0, 0, 1), (0, 1, 0), (1, 0, 0))):
            lo, hi = r[:, ax] < EPS_VOX, r[:, ax] > 1 - EPS_VOX
            a_k |= lo & (G.is_known(cz - dz, cy - dy, cx - dx) != kn)
            a_k |= hi & (G.is_known(cz + dz, cy + dy, cx + dx) != kn)
        amb |= active & a_k
        n_known += active & kn
        new = active & kn & prev_known & (f_prev > 0) & (f <= 0)
        if new.any():
            t_star[new] = (t - step) + step * (f_prev[new] / (f_prev[new] - f[new]))
            n_total[new] = k + 1
            hit |= new
            active &= ~new
        prev_known, f_prev = kn, f
    flags = hit.astype(np.uint8) * HIT
    flags |= np.where(n_known == 0, NONE_KNOWN, np.where(n_known < n_total, SOME_KNOWN, 0)).astype(np.uint8)
    depth = np.where(hit, t_star * dc[:, 2], empty_depth)
    # normals at the hit point
    normals = np.zeros((P, 3))
    namb = np.zeros(P, bool)
    hit_cell = np.full((P, 3), -1, np.int64)
    if hit.any():
        g = og[None] + t_star[hit, None] * dg[hit]
        cell, r, kn, _, _ = sample(g)
        idx = np.nonzero(hit)[0]
        hit_cell[idx] = cell[:, ::-1]
        namb[idx] = ((r < EPS_VOX) | (r > 1 - EPS_VOX)).any(1)
        n = np.zeros((len(idx), 3))
        if kn.any():
            c = G.corners(cell[kn, 2], cell[kn, 1], cell[kn, 0])
            rx, ry, rz = r[kn, 0], r[kn, 1], r[kn, 2]
            Gx = _lerp(_lerp(c[0][0][1] - c[0][0][0], c[0][1][1] - c[0][1][0], ry), _lerp(c[1][0][1] - c[1][0][0], c[1][1][1] - c[1][1][0], ry), rz)
            Gy = _lerp(_lerp(c[0][1][0] - c[0][0][0], c[0][1][1] - c[0][0][1], rx), _lerp(c[1][1][0] - c[1][0][0], c[1][1][1] - c[1][0][1], rx), rz)
            Gz = _lerp(_lerp(c[1][0][0] - c[0][0][0], c[1][0][1] - c[0][0][1], rx), _lerp(c[1][1][0] - c[0][1][0], c[1][1][1] - c[0][1][1], rx), ry)
            Gv = np.stack([Gx, Gy, Gz], -1)
            L = np.linalg.norm(Gv, axis=1)
            good = L > 0
            nk = np.zeros_like(Gv)
            nk[good] = Gv[good] / L[good, None]
            nk = np.where((nk * dirw[idx[kn]]).sum(1, keepdims=True) > 0, -nk, nk)
            if not world_normals:
                nk = nk @ E[:3, :3]  # R^T N
            n[kn] = nk
            sub = idx[kn]
            namb[sub] |= L < MIN_GRADIENT
            flags[sub[~good]] |= NO_NORMAL
        flags[idx[~kn]] |= NO_NORMAL
        normals[idx] = n
    shp = (H, W)
    return dict(depth=depth.reshape(shp), flags=flags.reshape(shp), normals=normals.T.reshape(3, H, W), ambiguous=amb.reshape(shp),
                normal_ambiguous=(namb | amb).reshape(shp), hit_cell=hit_cell.reshape(H, W, 3), missed=~entered.reshape(shp))


# ---- the committed scenes --------------------------------------------------------------------------------------------
def _pinhole(fx, fy, cx, cy):
    K = np.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return K


def _pose(ry, rx, rz, t):
    cy_, sy, cx_, sx, cz_, sz = np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx), np.cos(rz), np.sin(rz)
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Rz = np.array([[cz_, -sz, 0], [sz, cz_, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, t
    return T


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _depth_map(h, w, K, seed, box=True, holes=True):
    """A smooth surface about 1.75 m away with a box about 1.45 m away in front of it, and a few taps that are zero, NaN, negative or
    infinite; smooth in the camera's rays, not in pixels, so maps of different sizes see similar rooms."""
    r = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x, y = (jj + 0.5 - K[0, 2]) / K[0, 0], (ii + 0.5 - K[1, 2]) / K[1, 1]
    d = 1.75 + 0.12 * np.sin(3.1 * x + 0.4 * seed) * np.cos(2.7 * y) + 0.003 * r.standard_normal((h, w))
    if box:
        inb = (np.abs(x + 0.05) < 0.16) & (np.abs(y - 0.03) < 0.13)
        d = np.where(inb, 1.45 + 0.1 * x + 0.05 * y, d)
    d = d.astype(np.float32)
    if holes:
        d[3, 5], d[3, 6], d[h - 5, w - 5], d[h // 2, w // 2 + 6], d[h - 4, 4], d[5, w - 7] = 0.0, np.nan, np.nan, 0.0, -1.5, np.inf
    return d


# world_T_cam of the keyframes and of the live cameras: generic (no identity, no axis-aligned view), about 0.1 rad and 0.1 m apart
KEY_POSES = (_pose(0.05, -0.03, 0.04, (0.03, -0.02, 0.01)), _pose(-0.09, 0.04, -0.05, (0.13, 0.03, -0.04)), _pose(0.11, 0.06, 0.02, (-0.12, -0.04, 0.05)))
LIVE_POSES = {
    "near": _pose(0.02, 0.05, -0.07, (0.06, 0.04, 0.02)),
    "side": _pose(-0.42, 0.08, 0.1, (0.75, -0.1, 0.25)),   # looks across the volume: rays that miss it, rays through unobserved space
}

# name -> (dims (Nz,Ny,Nx), voxel size, origin, map size, K of the maps, number of maps)
SCENES = {
    "room24x32": ((20, 28, 36), 0.05, (-0.887, -0.679, 1.207), (24, 32), _pinhole(28.9, 28.4, 15.6, 12.3), 3),
    "room30x44": ((22, 19, 27), 0.06, (-0.813, -0.551, 1.153), (30, 44), _pinhole(38.3, 36.1, 23.4, 13.2), 2),
}
# name -> (H, W, K)
LIVE_CAMERAS = {"24x32": (24, 32, _pinhole(28.9, 28.4, 17.2, 11.1)), "30x44": (30, 44, _pinhole(38.3, 36.1, 20.9, 16.4))}
RAYCAST_CASES = (("room24x32", "near", "30x44"), ("room24x32", "side", "24x32"), ("room30x44", "near", "24x32"), ("room30x44", "side", "30x44"))
NEAR, FAR = 0.3, 2.7


def scene_inputs(name, M=None):
    """(dims, voxel_size, origin (3,) float32, depth (M,1,h,w) float32, K (M,4,4) float32, cam_T_world (M,4,4) float32)."""
    dims, v, origin, (h, w), K, n = SCENES[name]
    M = n if M is None else M
    depth = np.stack([_depth_map(h, w, K, seed=m)[None] for m in range(M)])
    return dims, v, _f32(origin), depth, _f32(np.stack([K] * M)), _f32(np.stack([np.linalg.inv(KEY_POSES[m]) for m in range(M)]))


@functools.lru_cache(maxsize=None)
def scene_integrated(name, M=None, max_weight=64.0):
    dims, v, origin, depth, K, E = scene_inputs(name, M)
    return integrate(empty_volume(dims), depth, K, E, origin, v, 3.0, max_weight)


def reference_values(name):
    """The reference's own fused volume as the float32 pair tensor a kernel would hold (for the CPU tests of the march)."""
    r = scene_integrated(name)
    return np.stack([r["T"].astype(np.float32), r["W"]], -1)


def live_camera(pose, cam):
    """(world_T_cam (4,4) float32, invK (4,4) float32, H, W)."""
    H, W, K = LIVE_CAMERAS[cam]
    return _f32(LIVE_POSES[pose]), _f32(np.linalg.inv(K)), H, W


def max_steps_for(voxel_size, step_voxels=1.0, near=NEAR, far=FAR):
    return int(np.ceil((far - near) / float(np.float32(step_voxels) * np.float32(voxel_size))))
