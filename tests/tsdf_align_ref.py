"""fp64 numpy statement of the TSDF pose alignment (include/idh_fusion.h: idh_tsdf_align_fwd), written from the header
and independent of the kernel, in the manner of tests/tsdf_ref.py, whose scenes, ``integrate``, ``U``, ``MARGIN``, ``EPS_VOX`` and ``CAP``
it reuses.  The inputs are the float32 arrays the kernel is given - the pose rounded to float32, as every iteration's per-pixel pass
reads it - and everything is evaluated in float64 from those values; ``trunc`` is the fp32 product the header defines.

``rows`` returns per pixel J (6), r, wgt and ``valid``, the bounds ``eps_J``, ``eps_r``, ``eps_w`` within which an fp32 evaluation in the
header's order must lie, and ``ambiguous``: where another fp32 implementation may decide differently.  With u = 2^-24 and MARGIN = 4:

Point.  q = invK (j + .5, i + .5, 1) takes 4 roundings, pc = q d one, R pc five and + t one: 11 roundings on partial results no larger
than S = |R| (|invK| (u, v, 1)) d + |t| (per row), so each component of pw is within dpw = 12 u S of its fp64 value.  g = (pw - o) / v
adds the subtraction's and the division's rounding: dg = (dpw + 2 u (|pw| + |o|)) / v voxels, 4.5e-5 at the committed scenes, below
tsdf_ref's 16 u 64 = 6.1e-5 from which EPS_VOX = 2.5e-4 comes.
  * a point within max(EPS_VOX, MARGIN dg) of a cell face is ambiguous: another implementation may take the neighbouring cell, and
    knownness and G are discontinuous there (f is not, but the test compares one cell's row).
Residual.  Inside a cell f moves by at most dg (D_x + D_y + D_z), D_axis the largest difference between corners that are neighbours
along the axis; a lerp a + r (b - a) of values in [-1, 1] adds at most 5 u (2 u the difference, 2 u the product, u the sum), three
levels 15 u; r = f trunc one more, relative:      eps_r = MARGIN (trunc (dg (D_x + D_y + D_z) + 16 u) + u |r|).
Gradient.  G.x is the bilinear interpolant in (r.y, r.z) of the four x-differences (each rounded once: 2 u).  It moves with r.y by at
most H_xy, the largest mixed second difference over the two z, and with r.z by at most H_xz; two levels of lerps of values in [-2, 2]
add 20 u.  n = G trunc_voxels one more:           eps_n.x = MARGIN (trunc_voxels (dg (H_xy + H_xz) + 24 u) + u |n.x|), y and z likewise.
Lever.  a = pw - t: dpw and the subtraction's rounding, da = dpw + u |a|.  A component of a x n, a.y n.z - a.z n.y, has two products
and a difference (3 roundings on magnitudes at most |a.y n.z| + |a.z n.y|):
    eps_J3 = MARGIN (|a.y| dn.z + |n.z| da.y + |a.z| dn.y + |n.y| da.z + 3 u (|a.y n.z| + |a.z n.y|))   with dn = eps_n / MARGIN.
Weight.  Without huber wgt = wm exactly.  With it, beyond the threshold, wgt = wm huber / |r|: eps_w = wgt (eps_r / |r| + 3 u MARGIN);
  * a pixel with | |r| - huber | < eps_r is ambiguous (the branch).
  * |G|^2 == 0: exact when the eight corners are equal (every difference is exactly 0 in fp32 too); otherwise a pixel whose |G| is below
    the norm of the eps_n / trunc_voxels is ambiguous.
  * The depth and weight tests (finite, > 0) are decided on the stored float32 by the same comparisons: never ambiguous.
Typical values at the committed scenes: eps_r 3e-7 m, eps_n 2e-5, eps_J3 5e-5.

``system`` sums the rows, ``solve`` is the header's damped Cholesky step with its pivot rule, ``align`` the whole loop with the pose in
fp64."""
import functools

import numpy as np

import tsdf_ref as R
from tsdf_ref import CAP, EPS_VOX, MARGIN, U  # noqa: F401  (the GPU tests read them from here)

PERTURBATION_A = ((0.02, -0.015, 0.01), (0.01, -0.008, 0.012))  # (dt metres, dr radians): 2.7 cm, 1.0 degree
PERTURBATION_B = ((0.04, 0.03, -0.03), (0.02, 0.02, -0.02))     # 5.8 cm, 2.0 degrees


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_so3(w):
    """Rodrigues in fp64; the first-order form below |w| = 1e-12 (the header's rule)."""
    w = np.asarray(w, np.float64)
    th = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    K = hat(w)
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def perturb(world_T_cam, dt, dr):
    """R0 = exp(dr^) R, t0 = t + dt, as float32 (4,4)."""
    T = np.asarray(world_T_cam, np.float64).copy()
    T[:3, :3] = exp_so3(dr) @ T[:3, :3]
    T[:3, 3] += np.asarray(dt, np.float64)
    return R._f32(T)


def pose_error(T, T_true):
    """(metres, radians) between two world_T_cam."""
    T, T_true = np.asarray(T, np.float64), np.asarray(T_true, np.float64)
    M = T[:3, :3] @ T_true[:3, :3].T
    # the angle from the antisymmetric part as well: arccos of the trace alone resolves no angle below 1e-4 once an entry is rounded to fp32
    s = 0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])), float(np.arctan2(s, (np.trace(M) - 1.0) / 2.0))


def rows(values, origin, voxel_size, trunc_voxels, depth, invK, world_T_cam, weight=None, stride=1, huber=0.0, exact_pose=False):
    """One per-pixel pass at the float32 pose ``world_T_cam``.  (h,w,...) arrays: ``J`` (6), ``r``, ``wgt``, ``valid``, ``selected``,
    ``ambiguous``, ``eps_J`` (6), ``eps_r``, ``eps_w``, ``face`` (distance to the nearest cell face in voxels; inf where the pixel has
    no point).  Rows of pixels that are not valid are zero.  ``exact_pose`` takes the pose as float64 (for finite differences)."""
    values = np.asarray(values)
    assert values.dtype == np.float32
    G = R._Grid(values)
    d32 = np.asarray(depth, np.float32).reshape(np.asarray(depth).shape[-2:])
    h, w = d32.shape
    v, tv = float(np.float32(voxel_size)), float(np.float32(trunc_voxels))
    trunc = R.trunc_of(trunc_voxels, voxel_size)
    hub = float(np.float32(huber))
    o = np.asarray(origin, np.float32).astype(np.float64)
    E, iK = np.asarray(world_T_cam, np.float32).astype(np.float64), np.asarray(invK, np.float32).astype(np.float64)
    if exact_pose:
        E = np.asarray(world_T_cam, np.float64)
    Rm, t = E[:3, :3], E[:3, 3]
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    selected = (ii % stride == 0) & (jj % stride == 0)
    ok = selected & np.isfinite(d32) & (d32 > 0)
    wm = np.ones((h, w))
    if weight is not None:
        w32 = np.asarray(weight, np.float32).reshape(h, w)
        ok &= np.isfinite(w32) & (w32 > 0)
        wm = np.where(ok, w32, 1.0).astype(np.float64)
    d = np.where(ok, d32, 1.0).astype(np.float64)
    uv1 = np.stack([jj + 0.5, ii + 0.5, np.ones((h, w))], -1)
    q = uv1 @ iK[:3, :3].T
    pc = q * d[..., None]
    pw = pc @ Rm.T + t
    S = ((uv1 @ np.abs(iK[:3, :3]).T) * d[..., None]) @ np.abs(Rm).T + np.abs(t)
    dpw = 12 * U * S
    g = (pw - o) / v
    dg = ((dpw + 2 * U * (np.abs(pw) + np.abs(o))) / v).max(-1)
    cell = np.floor(g).astype(np.int64)
    rr = g - cell
    face = np.minimum(rr, 1.0 - rr).min(-1)
    cx, cy, cz = cell[..., 0], cell[..., 1], cell[..., 2]
    known = np.zeros((h, w), bool)
    known[ok] = G.is_known(cz[ok], cy[ok], cx[ok])
    amb = ok & (face < np.maximum(EPS_VOX, MARGIN * dg))
    out = dict(J=np.zeros((h, w, 6)), r=np.zeros((h, w)), wgt=np.zeros((h, w)), eps_J=np.zeros((h, w, 6)), eps_r=np.zeros((h, w)),
               eps_w=np.zeros((h, w)), selected=selected, face=np.where(ok, face, np.inf))
    valid = np.zeros((h, w), bool)
    if known.any():
        k = known
        c = np.array(G.corners(cz[k], cy[k], cx[k]))  # [z][y][x][pixel]
        rx, ry, rz = rr[k, 0], rr[k, 1], rr[k, 2]
        L = R._lerp
        a = [[L(c[z][y][0], c[z][y][1], rx) for y in (0, 1)] for z in (0, 1)]
        f = L(L(a[0][0], a[0][1], ry), L(a[1][0], a[1][1], ry), rz)
        Gx = L(L(c[0][0][1] - c[0][0][0], c[0][1][1] - c[0][1][0], ry), L(c[1][0][1] - c[1][0][0], c[1][1][1] - c[1][1][0], ry), rz)
        Gy = L(L(c[0][1][0] - c[0][0][0], c[0][1][1] - c[0][0][1], rx), L(c[1][1][0] - c[1][0][0], c[1][1][1] - c[1][0][1], rx), rz)
        Gz = L(L(c[1][0][0] - c[0][0][0], c[1][0][1] - c[0][0][1], rx), L(c[1][1][0] - c[0][1][0], c[1][1][1] - c[0][1][1], rx), ry)
        Gv = np.stack([Gx, Gy, Gz], -1)
        D = sum(np.abs(np.diff(c, axis=ax)).max(axis=(0, 1, 2)) for ax in (0, 1, 2))
        m = c[1] - c[0]  # [y][x]
        Hyz, Hxz = np.abs(m[1] - m[0]).max(0), np.abs(m[:, 1] - m[:, 0]).max(0)
        Hxy = np.abs((c[:, 1, 1] - c[:, 1, 0]) - (c[:, 0, 1] - c[:, 0, 0])).max(0)
        dgk = dg[k]
        res = f * trunc
        eps_r = MARGIN * (trunc * (dgk * D + 16 * U) + U * np.abs(res))
        n = Gv * tv
        dG = np.stack([dgk * (Hxy + Hxz), dgk * (Hxy + Hyz), dgk * (Hxz + Hyz)], -1) + 24 * U
        dn = tv * dG + U * np.abs(n)
        al = pw[k] - t
        da = dpw[k] + U * np.abs(al)
        J = np.concatenate([n, np.cross(al, n)], -1)
        eps_J = np.zeros_like(J)
        eps_J[:, :3] = MARGIN * dn
        for comp, (p, s) in enumerate(((1, 2), (2, 0), (0, 1))):  # (a x n)[comp] = a[p] n[s] - a[s] n[p]
            eps_J[:, 3 + comp] = MARGIN * (np.abs(al[:, p]) * dn[:, s] + np.abs(n[:, s]) * da[:, p] + np.abs(al[:, s]) * dn[:, p] + np.abs(n[:, p]) * da[:, s]
                                           + 3 * U * (np.abs(al[:, p] * n[:, s]) + np.abs(al[:, s] * n[:, p])))
        G2 = (Gx * Gx + Gy * Gy) + Gz * Gz
        flat = c.reshape(8, -1).max(0) == c.reshape(8, -1).min(0)
        nonzero = G2 != 0
        amb_k = ~flat & (np.sqrt(G2) < MARGIN * np.linalg.norm(dG, axis=1))
        ar = np.abs(res)
        wgt = wm[k].copy()
        eps_w = np.zeros_like(wgt)
        if hub > 0:
            far = ar > hub
            wgt = np.where(far, wgt * hub / np.where(far, ar, 1.0), wgt)
            eps_w = np.where(far, wgt * (eps_r / np.where(far, ar, 1.0) + 3 * U * MARGIN), 0.0)
            amb_k |= np.abs(ar - hub) < eps_r
        idx = np.nonzero(k)
        sub = tuple(i[nonzero] for i in idx)
        valid[sub] = True
        out["J"][sub], out["r"][sub], out["wgt"][sub] = J[nonzero], res[nonzero], wgt[nonzero]
        out["eps_J"][sub], out["eps_r"][sub], out["eps_w"][sub] = eps_J[nonzero], eps_r[nonzero], eps_w[nonzero]
        amb[idx] |= amb_k
    out["valid"], out["ambiguous"] = valid, amb
    return out


TRIU = tuple((p, q) for p in range(6) for q in range(p, 6))


def system(J, r, wgt, valid=None):
    """(A (6,6), b (6), cost, count) of rows given as (...,6), (...), (...); ``valid`` defaults to wgt != 0 or J != 0."""
    J, r, wgt = np.asarray(J, np.float64).reshape(-1, 6), np.asarray(r, np.float64).ravel(), np.asarray(wgt, np.float64).ravel()
    A = (J * wgt[:, None]).T @ J
    b = (J * wgt[:, None]).T @ r
    count = int(np.asarray(valid).sum()) if valid is not None else int(((wgt != 0) | (J != 0).any(1)).sum())
    return A, b, float((wgt * r * r).sum()), count


def record_system(rec):
    """(A (6,6) symmetric, b) of one 40-double record."""
    A = np.zeros((6, 6))
    for n, (p, q) in enumerate(TRIU):
        A[p, q] = A[q, p] = rec[n]
    return A, np.asarray(rec[21:27], np.float64)


def solve(A, b, count, damping=0.0, min_count=64, min_pivot_ratio=1e-6):
    """(status, xi, pivots / diagonal).  Status 1: count < min_count; 2: a Cholesky pivot p_k <= min_pivot_ratio A'_kk; else 0 and
    xi = -(A')^-1 b with A' = A + damping diag(A)."""
    if count < min_count:
        return 1, np.zeros(6), None
    Ad = np.array(A, np.float64)
    Ad[np.diag_indices(6)] += damping * np.diag(A)
    Lm = np.zeros((6, 6))
    ratios = np.zeros(6)
    for k in range(6):
        p = Ad[k, k] - (Lm[k, :k] ** 2).sum()
        ratios[k] = p / Ad[k, k] if Ad[k, k] != 0 else 0.0
        if not p > min_pivot_ratio * Ad[k, k]:
            return 2, np.zeros(6), ratios
        Lm[k, k] = np.sqrt(p)
        for i in range(k + 1, 6):
            Lm[i, k] = (Ad[i, k] - (Lm[i, :k] * Lm[k, :k]).sum()) / Lm[k, k]
    y = np.linalg.solve(Lm, -np.asarray(b, np.float64))
    return 0, np.linalg.solve(Lm.T, y), ratios


def update(Rm, t, xi):
    return exp_so3(xi[3:]) @ Rm, t + xi[:3]


def align(values, origin, voxel_size, trunc_voxels, depth, invK, world_T_cam, weight=None, iters=8, stride=1, huber=0.0, damping=0.0,
          min_step=0.0, min_count=64, min_pivot_ratio=1e-6):
    """The whole loop.  Returns dict: ``world_T_cam`` (4,4) fp64 (the fp64 pose, not rounded), ``statuses``, ``steps`` (per executed
    status-0 iteration (|v|, |w|)), ``costs``, ``counts``, ``ratios`` (of iteration 0)."""
    E = np.asarray(world_T_cam, np.float32).astype(np.float64)
    Rm, t = E[:3, :3].copy(), E[:3, 3].copy()
    out = dict(statuses=[], steps=[], costs=[], counts=[], ratios=None)
    stopped = False
    for it in range(iters):
        if stopped:
            out["statuses"].append(3)
            continue
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = Rm, t
        rw = rows(values, origin, voxel_size, trunc_voxels, depth, invK, R._f32(P), weight, stride, huber)
        A, b, cost, count = system(rw["J"], rw["r"], rw["wgt"], rw["valid"])
        status, xi, ratios = solve(A, b, count, damping, min_count, min_pivot_ratio)
        if it == 0:
            out["ratios"] = ratios
        out["statuses"].append(status), out["costs"].append(cost), out["counts"].append(count)
        if status == 0:
            Rm, t = update(Rm, t, xi)
            nv, nw = float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]))
            out["steps"].append((nv, nw))
            stopped = nv < min_step and nw < min_step
        else:
            stopped = True
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = Rm, t
    out["world_T_cam"] = P
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name, box):
    """A committed scene as the alignment sees it: dict ``values`` (Nz,Ny,Nx,2) float32 - with ``box`` the reference's fused volume of
    all the scene's maps (``tsdf_ref.reference_values``), without it the volume of map 0 alone rendered without the box -, ``origin``,
    ``voxel_size``, ``trunc_voxels``, ``depth`` (h,w) float32: map 0 (with or without the box, holes kept), ``invK`` float32 (4,4) and
    ``pose``: map 0's own world_T_cam as float32, the truth."""
    dims, v, origin, (h, w), K, _ = R.SCENES[name]
    origin = R._f32(origin)
    if box:
        values = R.reference_values(name)
        depth = R.scene_inputs(name)[3][0, 0]
    else:
        depth = R._depth_map(h, w, K, seed=0, box=False)
        r = R.integrate(R.empty_volume(dims), depth[None, None], R._f32(K[None]), R._f32(np.linalg.inv(R.KEY_POSES[0])[None]), origin, v, 3.0, 64.0)
        values = np.stack([r["T"].astype(np.float32), r["W"]], -1)
    return dict(values=values, origin=origin, voxel_size=v, trunc_voxels=3.0, depth=depth, invK=R._f32(np.linalg.inv(K)), pose=R._f32(R.KEY_POSES[0]))


def plane_case():
    """A volume fused from a fronto-parallel constant-depth map seen by an axis-aligned camera: T depends on z alone, so G.x == 0 exactly
    at every pixel and the normal matrix's first pivot is 0."""
    dims, v, origin = (12, 14, 16), 0.05, R._f32((-0.4, -0.35, 0.7))
    h, w, K = 12, 16, R._pinhole(14.0, 14.0, 8.0, 6.0)
    depth = np.full((h, w), 1.0, np.float32)
    r = R.integrate(R.empty_volume(dims), depth[None, None], R._f32(K[None]), R._f32(np.eye(4)[None]), origin, v, 3.0, 64.0)
    values = np.stack([r["T"].astype(np.float32), r["W"]], -1)
    return dict(values=values, origin=origin, voxel_size=v, trunc_voxels=3.0, depth=depth, invK=R._f32(np.linalg.inv(K)), pose=R._f32(np.eye(4)))


def weight_map(h, w, seed=3):
    """Weights in (0.25, 2) with zeros, a NaN and a negative one among them."""
    wm = np.random.default_rng(seed).uniform(0.25, 2.0, (h, w)).astype(np.float32)
    wm[1, 2], wm[h // 2, w // 3], wm[h - 2, 3] = 0.0, 0.0, 0.0
    wm[2, w - 3], wm[h // 3, w // 2] = np.nan, -0.5
    return wm


# (scene, box, stride, weighted, huber) of the per-pixel GPU tests, and the 5 x 7 crops (fewer selected pixels than a wave)
ROW_CASES = tuple((name, box, s, wt, hub) for name in ("room24x32", "room30x44") for box in (False, True)
                  for s, wt, hub in ((1, False, 0.0), (1, True, 0.01), (2, True, 0.0), (3, False, 0.01)))
CROP = (8, 10, 5, 7)  # (i0, j0, h, w)


def row_inputs(name, box, weighted, crop=False):
    """The case's arrays with the input pose of the per-pixel tests - the truth moved by PERTURBATION_A - and the weight map or None;
    ``crop`` cuts the map to CROP (the principal point moves with it)."""
    c = dict(case(name, box))
    c["start"] = perturb(c["pose"], *PERTURBATION_A)
    if crop:
        i0, j0, h, w = CROP
        K = np.array(R.SCENES[name][4])
        K[0, 2], K[1, 2] = K[0, 2] - j0, K[1, 2] - i0
        c["depth"], c["invK"] = np.ascontiguousarray(c["depth"][i0:i0 + h, j0:j0 + w]), R._f32(np.linalg.inv(K))
    c["weight"] = weight_map(*c["depth"].shape) if weighted else None
    return c


@functools.lru_cache(maxsize=None)
def row_reference(name, box, stride, weighted, huber, crop=False):
    c = row_inputs(name, box, weighted, crop)
    return rows(c["values"], c["origin"], c["voxel_size"], c["trunc_voxels"], c["depth"], c["invK"], c["start"], c["weight"], stride, huber)


def analytic_depth(name, k, holes=True):
    """Map k of a sequence rendered consistently from ONE surface: ``tsdf_ref._depth_map``'s smooth wall (seed 0, no box, no noise),
    z = 1.75 + 0.12 sin(3.1 x / z) cos(2.7 y / z) in camera 0's frame, evaluated ANALYTICALLY along the rays of camera k (KEY_POSES[k],
    the scene's K): per pixel the root of z(p) - D(p) along the ray by bisection in fp64.  (h,w) float32, with a few holes."""
    _, _, _, (h, w), K, _ = R.SCENES[name]
    rel = np.linalg.inv(R.KEY_POSES[0]) @ R.KEY_POSES[k]  # camera k -> camera 0
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ray = np.stack([(jj + 0.5 - K[0, 2]) / K[0, 0], (ii + 0.5 - K[1, 2]) / K[1, 1], np.ones((h, w))], -1)  # z = 1: the parameter is the depth
    dirs, o = ray @ rel[:3, :3].T, rel[:3, 3]

    def gap(s):
        p = o + s[..., None] * dirs
        return p[..., 2] - (1.75 + 0.12 * np.sin(3.1 * p[..., 0] / p[..., 2]) * np.cos(2.7 * p[..., 1] / p[..., 2]))

    lo, hi = np.full((h, w), 1.0), np.full((h, w), 3.0)
    assert (gap(lo) < 0).all() and (gap(hi) > 0).all()
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        below = gap(mid) < 0
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    d = (0.5 * (lo + hi)).astype(np.float32)
    if holes:
        d[3, 5], d[3, 6], d[h - 5, w - 5], d[h // 2, w // 2 + 6] = 0.0, np.nan, np.inf, -1.5
    return d
