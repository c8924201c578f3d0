"""fp64 numpy statement of the TSDF colour semantics (include/idh_fusion.h: idh_tsdf_integrate_color_fwd, idh_tsdf_raycast_color_fwd,
idh_tsdf_mesh_colors_fwd), written from the header and independent of the kernels.  It reuses the scenes, poses and
the rounding model (U, MARGIN, CAP) of tests/tsdf_ref.py and adds the camera frames.

Voxel (``integrate``).  The {T, W} update and its ambiguity terms are tsdf_ref.integrate's, restated here because the colour needs the
per-map state.  Two more decisions can fall the other way in fp32, under the same MARGIN:
  * |sdf - trunc| < EPS_SDF at updated voxels (the ``sdf <= trunc`` test; EPS_SDF as for the truncation test), and
  * qx (or qy) within EPS_PX of an integer at band voxels, EPS_PX formed as for px with the colour camera's focal lengths (the tap's
    pixel borders, and with them the frame's own borders 0 and wc / hc).
The colour itself: per channel one update is a multiply, an add, an add and a divide on magnitudes up to Wc * 255 + 255 <= 765 for three
maps - with the conversion 9 roundings over the maps the scenes have at magnitude <= 765: 9 * 2^-24 * 765 = 4e-4 < the tests' 1e-3.

Pixel (``raycast_colors``).  The march is tsdf_ref.raycast's and tested there; the colour takes the kernel's own hit depth as input and
restates the interpolation alone.  g* = og + t* dg carries the position error of tsdf_ref (dg_err = 16 u 64 voxels; t* = depth / dc.z adds
two relative roundings, far inside it).  With S the coloured corners, v = sum_S w C / sum_S w:
  * all eight coloured (den = 1): v is the trilinear interpolant, its slope along an axis at most the largest difference D_axis between
    corners that are neighbours along it: |dv| <= dg_err (D_x + D_y + D_z);
  * otherwise dv/dg = sum_S (dw/dg) (C - v) / den with sum |dw/dg_axis| <= 2 per axis and |C - v| <= the spread of C over S:
    |dv| <= 6 dg_err spread_S / den;
  * the arithmetic: a weight is two subtractions and two products (4 roundings, relative), w C one more, the eight-term sums 8 each at
    magnitude <= 255, the same relative error in den, and the divide: 24 u 255 = 3.7e-4.
  BOUND = MARGIN (the position term + 24 u 255) per pixel and channel: a byte is certain when v is further than BOUND from k + 0.5.
  A pixel is ambiguous when den < 1e-3 or when, within EPS_VOX of a cell face, the neighbouring cell's pattern of coloured corners differs.

Vertex (``mesh_colors``).  r = T_a / (T_a - T_b) (two roundings), C_a + r (C_b - C_a) three more at magnitude <= 255: 5 u 255 = 8e-5,
so a byte is certain when v is more than 1e-3 from k + 0.5."""
import functools

import numpy as np

import tsdf_ref as R

U, MARGIN, CAP, EPS_VOX = R.U, R.MARGIN, R.CAP, R.EPS_VOX
MIN_DEN = 1e-3
COLOR_CAMERAS = ("same", "double", "odd")
ROUNDINGS = 24 * U * 255


def color_camera(scene, cam):
    """(hc, wc, K (4,4) float64) of a colour camera of the scene: the map's own, twice its size, or an unrelated one whose frame does not
    cover all of the map's view."""
    (h, w), K = R.SCENES[scene][3], R.SCENES[scene][4]
    if cam == "same":
        return h, w, K.copy()
    if cam == "double":
        K2 = K.copy()
        K2[0] *= 2
        K2[1] *= 2
        return 2 * h, 2 * w, K2
    assert cam == "odd"
    return int(1.3 * h), int(1.25 * w), R._pinhole(K[0, 0] * 1.37, K[1, 1] * 1.41, 1.3 * K[0, 2] + 0.7, 1.35 * K[1, 2] - 0.4)


def _frame(hc, wc, K, seed):
    """A uint8 (hc,wc,3) frame: smooth in the camera's rays (frames of different sizes see similar rooms), a differently coloured box
    where _depth_map has its box, and a few units of noise."""
    r = np.random.default_rng(1000 + seed)
    ii, jj = np.meshgrid(np.arange(hc), np.arange(wc), indexing="ij")
    x, y = (jj + 0.5 - K[0, 2]) / K[0, 0], (ii + 0.5 - K[1, 2]) / K[1, 1]
    c = np.stack([128 + 90 * np.sin(2.3 * x + 0.5 * seed) * np.cos(1.9 * y), 120 + 80 * np.cos(2.9 * x - 1.1 * y + 0.3 * seed),
                  100 + 70 * np.sin(1.7 * y + 2.1 * x)], -1)
    inb = (np.abs(x + 0.05) < 0.16) & (np.abs(y - 0.03) < 0.13)
    box = np.stack([235 - 60 * x, 40 + 150 * np.abs(y), np.full_like(x, 30.0)], -1)
    c = np.where(inb[..., None], box, c) + r.integers(-3, 4, size=(hc, wc, 3))
    return np.clip(np.rint(c), 0, 255).astype(np.uint8)


def scene_frames(scene, cam, M=None):
    """(frames (M,hc,wc,3) uint8, K (M,4,4) float32): one frame per map of the scene in the colour camera ``cam``."""
    n = R.SCENES[scene][5]
    M = n if M is None else M
    hc, wc, K = color_camera(scene, cam)
    return np.stack([_frame(hc, wc, K, m) for m in range(M)]), R._f32(np.stack([K] * M))


def integrate(values, colors, depths, Ks, cam_T_worlds, frames, color_Ks, origin, voxel_size, trunc_voxels=3.0, max_weight=64.0):
    """``values`` (Nz,Ny,Nx,2) and ``colors`` (Nz,Ny,Nx,4) float32 before; M maps with their frames; ``frames`` None: depth only.
    Returns dict: ``T`` fp64, ``W`` float32, ``touched``, ``C`` (Nz,Ny,Nx,3) fp64, ``Wc`` float32, ``coloured`` bool (some map coloured
    the voxel), ``band`` bool (some map updated it with sdf <= trunc), ``free_only`` bool (touched, never in a band), ``band_outside``
    (band voxel-updates whose tap falls off the frame), ``ambiguous`` bool."""
    values, colors = np.asarray(values), np.asarray(colors)
    assert values.dtype == np.float32 and colors.dtype == np.float32
    Nz, Ny, Nx = values.shape[:3]
    T, W = values[..., 0].astype(np.float64), values[..., 1].copy()
    Cc, Wc = colors[..., :3].astype(np.float64), colors[..., 3].copy()
    v = float(np.float32(voxel_size))
    o = np.asarray(origin, np.float32).astype(np.float64)
    trunc = R.trunc_of(trunc_voxels, voxel_size)
    zz, yy, xx = np.meshgrid(np.arange(Nz), np.arange(Ny), np.arange(Nx), indexing="ij")
    p = np.stack([o[0] + v * xx, o[1] + v * yy, o[2] + v * zz], -1)
    shape = (Nz, Ny, Nx)
    touched, amb, coloured, band_any = (np.zeros(shape, bool) for _ in range(4))
    band_outside = 0
    for m, (depth, K, E) in enumerate(zip(depths, Ks, cam_T_worlds)):
        d32 = np.asarray(depth, np.float32).reshape(depth.shape[-2:])
        h, w = d32.shape
        K, E = np.asarray(K, np.float32).astype(np.float64), np.asarray(E, np.float32).astype(np.float64)
        c = p @ E[:3, :3].T + E[:3, 3]
        dc = 8 * U * (np.abs(p) @ np.abs(E[:3, :3]).T + np.abs(E[:3, 3]))
        amb |= np.abs(c[..., 2]) < MARGIN * dc[..., 2]
        front = c[..., 2] > 0
        cz = np.where(front, c[..., 2], 1.0)
        rx, ry = c[..., 0] / cz, c[..., 1] / cz

        def project(Km):
            qx, qy = Km[0, 0] * rx + Km[0, 2], Km[1, 1] * ry + Km[1, 2]
            ex = MARGIN * (Km[0, 0] * (dc[..., 0] + np.abs(rx) * dc[..., 2]) / cz + 3 * U * (np.abs(Km[0, 0] * rx) + np.abs(qx)))
            ey = MARGIN * (Km[1, 1] * (dc[..., 1] + np.abs(ry) * dc[..., 2]) / cz + 3 * U * (np.abs(Km[1, 1] * ry) + np.abs(qy)))
            return qx, qy, (np.abs(qx - np.rint(qx)) < ex) | (np.abs(qy - np.rint(qy)) < ey)

        px, py, near_int = project(K)
        near_image = front & (px > -1) & (px < w + 1) & (py > -1) & (py < h + 1)
        amb |= near_image & near_int
        inside = front & (px >= 0) & (px < w) & (py >= 0) & (py < h)
        j = np.where(inside, np.floor(px), 0).astype(np.int64)
        i = np.where(inside, np.floor(py), 0).astype(np.int64)
        d = d32[i, j]
        ok = inside & np.isfinite(d) & (d > 0)
        dd = np.where(ok, d, 1.0).astype(np.float64)
        sdf = dd - c[..., 2]
        eps_sdf = MARGIN * (dc[..., 2] + 2 * U * (dd + np.abs(c[..., 2])) + 2 * U * trunc)
        amb |= ok & (np.abs(sdf + trunc) < eps_sdf)
        upd = ok & ~(sdf < -trunc)
        s = np.minimum(1.0, sdf / trunc)
        W64 = W.astype(np.float64)
        T = np.where(upd, (W64 * T + s) / (W64 + 1), T)
        W = np.where(upd, np.minimum(W + np.float32(1), np.float32(max_weight)), W)
        touched |= upd
        if frames is None:
            continue
        # the colour, immediately after the voxel's {T, W} update for this map
        f8 = np.asarray(frames[m])
        assert f8.dtype == np.uint8 and f8.ndim == 3 and f8.shape[2] == 3
        hc, wc = f8.shape[:2]
        amb |= upd & (np.abs(sdf - trunc) < eps_sdf)
        band = upd & (sdf <= trunc)
        qx, qy, q_near_int = project(np.asarray(color_Ks[m], np.float32).astype(np.float64))
        amb |= band & q_near_int
        cin = band & (qx >= 0) & (qx < wc) & (qy >= 0) & (qy < hc)
        band_outside += int((band & ~cin).sum())
        jc = np.where(cin, np.floor(qx), 0).astype(np.int64)
        ic = np.where(cin, np.floor(qy), 0).astype(np.int64)
        tap = f8[ic, jc].astype(np.float64)
        Wc64 = Wc.astype(np.float64)[..., None]
        Cc = np.where(cin[..., None], (Wc64 * Cc + tap) / (Wc64 + 1), Cc)
        Wc = np.where(cin, np.minimum(Wc + np.float32(1), np.float32(max_weight)), Wc)
        assert Wc.dtype == np.float32
        coloured |= cin
        band_any |= band
    return dict(T=T, W=W, touched=touched, C=Cc, Wc=Wc, coloured=coloured, band=band_any, free_only=touched & ~band_any,
                band_outside=band_outside, ambiguous=amb)


@functools.lru_cache(maxsize=None)
def scene_integrated(scene, cam, M=None, max_weight=64.0):
    """The scene's maps and their frames in colour camera ``cam`` into an empty volume."""
    dims, v, origin, depth, K, E = R.scene_inputs(scene, M)
    frames, Kc = scene_frames(scene, cam, M)
    return integrate(R.empty_volume(dims), np.zeros((*dims, 4), np.float32), depth, K, E, frames, Kc, origin, v, 3.0, max_weight)


def byte_of(v):
    """The header's rounding of a channel, in fp64."""
    return np.floor(np.clip(v, 0, 255) + 0.5).astype(np.int64)


def boundary_distance(v):
    """How far a channel value is from the nearest k + 0.5 at which its byte changes (clipped values: from 0.5 or 254.5)."""
    c = np.clip(v, 0, 255)
    return np.abs(c - (np.floor(c) + 0.5))


def raycast_colors(colors, depth, hit, origin, voxel_size, world_T_cam, invK):
    """``colors`` (Nz,Ny,Nx,4) float32; ``depth`` (H,W) and ``hit`` (H,W) bool as the kernel returned them.  Returns dict: ``value``
    (H,W,3) fp64 (the channel before rounding; 0 without alpha), ``rgba`` (H,W,4) int64, ``alpha`` (H,W) bool (den > 0 at a hit whose
    cell is in range), ``bound`` (H,W) fp64, ``ambiguous`` (H,W) bool."""
    colors = np.asarray(colors)
    assert colors.dtype == np.float32
    Nz, Ny, Nx = colors.shape[:3]
    H, W = depth.shape
    v = float(np.float32(voxel_size))
    o = np.asarray(origin, np.float32).astype(np.float64)
    E, iK = np.asarray(world_T_cam, np.float32).astype(np.float64), np.asarray(invK, np.float32).astype(np.float64)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    q = np.stack([jj + 0.5, ii + 0.5, np.ones((H, W))], -1).reshape(-1, 3) @ iK[:3, :3].T
    dc = q / np.linalg.norm(q, axis=1, keepdims=True)
    og, dg = (E[:3, 3] - o) / v, (dc @ E[:3, :3].T) / v
    hit = np.asarray(hit).reshape(-1)
    t = np.where(hit, np.asarray(depth, np.float64).reshape(-1) / dc[:, 2], 0.0)
    g = og[None] + t[:, None] * dg
    cell = np.floor(g).astype(np.int64)
    r = g - cell
    n_cells = np.array([Nx - 1, Ny - 1, Nz - 1])
    P = H * W
    Cf, has = colors[..., :3].astype(np.float64), colors[..., 3] > 0

    def pattern(cl):
        """(P,8) bool: the coloured corners of the cells ``cl`` (x, y, z), and (P,) whether the cell is in range."""
        inr = ((cl >= 0) & (cl < n_cells)).all(1)
        c0 = np.where(inr[:, None], cl, 0)
        out = np.zeros((len(cl), 8), bool)
        for c in range(8):
            dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
            out[:, c] = has[c0[:, 2] + dz, c0[:, 1] + dy, c0[:, 0] + dx] & inr
        return out, inr

    pat, inr = pattern(cell)
    live = hit & inr
    c0 = np.where(live[:, None], cell, 0)
    num, den = np.zeros((P, 3)), np.zeros(P)
    corner = np.zeros((P, 8, 3))
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        w = (r[:, 0] if dx else 1 - r[:, 0]) * (r[:, 1] if dy else 1 - r[:, 1]) * (r[:, 2] if dz else 1 - r[:, 2])
        w = np.where(pat[:, c] & live, w, 0.0)
        corner[:, c] = Cf[c0[:, 2] + dz, c0[:, 1] + dy, c0[:, 0] + dx]
        num += w[:, None] * corner[:, c]
        den += w
    alpha = live & (den > 0)
    value = np.where(alpha[:, None], num / np.where(den > 0, den, 1.0)[:, None], 0.0)
    # the bound
    full = pat.all(1)
    cube = corner.reshape(P, 2, 2, 2, 3)  # [dz][dy][dx]
    slope = sum(np.abs(np.diff(cube, axis=ax)).max(axis=(1, 2, 3, 4)) for ax in (1, 2, 3))
    big = np.where(pat[:, :, None], corner, -np.inf).max(axis=(1, 2))
    small = np.where(pat[:, :, None], corner, np.inf).min(axis=(1, 2))
    spread = np.where(pat.any(1), big - small, 0.0)
    dg_err = 16 * U * 64
    position = np.where(full, dg_err * slope, 6 * dg_err * spread / np.maximum(den, MIN_DEN))
    bound = MARGIN * (position + ROUNDINGS)
    amb = live & (den < MIN_DEN)
    for ax in range(3):
        for side, shift in ((r[:, ax] < EPS_VOX, -1), (r[:, ax] > 1 - EPS_VOX, 1)):
            nb = cell.copy()
            nb[:, ax] += shift
            npat, _ = pattern(nb)
            amb |= hit & side & (npat != pat).any(1)
    rgba = np.concatenate([np.where(alpha[:, None], byte_of(value), 0), np.where(alpha, 255, 0)[:, None]], 1)
    return dict(value=value.reshape(H, W, 3), rgba=rgba.reshape(H, W, 4), alpha=alpha.reshape(H, W), bound=bound.reshape(H, W),
                ambiguous=amb.reshape(H, W))


def mesh_colors(values, colors, owner, axis):
    """The colours of the vertices mesh_ref.extract lists by ``owner`` and ``axis``.  Returns dict: ``value`` (V,3) fp64, ``rgba`` (V,4)
    int64, ``alpha`` (V,) bool."""
    values, colors = np.asarray(values), np.asarray(colors)
    Nz, Ny, Nx = values.shape[:3]
    stride = np.array([1, Nx, Nx * Ny])
    Tf = values[..., 0].reshape(-1).astype(np.float64)
    Cf, Wf = colors[..., :3].reshape(-1, 3).astype(np.float64), colors[..., 3].reshape(-1)
    a, b = owner, owner + stride[axis]
    r = Tf[a] / (Tf[a] - Tf[b])
    ha, hb = Wf[a] > 0, Wf[b] > 0
    value = np.where((ha & hb)[:, None], Cf[a] + r[:, None] * (Cf[b] - Cf[a]), np.where(ha[:, None], Cf[a], np.where(hb[:, None], Cf[b], 0.0)))
    alpha = ha | hb
    rgba = np.concatenate([np.where(alpha[:, None], byte_of(value), 0), np.where(alpha, 255, 0)[:, None]], 1)
    return dict(value=value, rgba=rgba, alpha=alpha)
