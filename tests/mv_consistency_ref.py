"""fp64 numpy statement of the multi-view depth consistency check (include/idh_geometry.h: idh_mv_consistency_fwd) and
of the weighted TSDF integrate (include/idh_fusion.h: idh_tsdf_integrate_weighted_fwd), written from the headers and independent of the
kernels.  The inputs are the float32 arrays the kernels are given; everything is evaluated in float64 from those values.

``check`` also says which (map, source, pixel) entries are *ambiguous* - what another fp32 implementation may decide the other way:
  * the fp64 projection px (or py) lies within EPS_PX = 1e-3 px of an integer - a border between two nearest taps, or an image edge -
    and within one pixel of the image (further out both neighbours are padding, so the outcome cannot differ), or
  * the gate comparison z_gate < ratio * s, or one of the tolerance comparisons err <= log_tol and l > log_tol, lies within
    EPS_REL = 1e-5 relative of its threshold.
A pixel is ambiguous when an entry of one of its K sources is.  At most CAP = 1 % of a case's pixels may be: the fixtures of
``fixture`` are nudged until that holds (``settle``), and tests/test_mv_consistency_cpu.py asserts it on this file alone.

The fixtures are synthetic: a planar wall seen by cameras with rotation and translation, patches in front of and behind the wall,
noise, and a few taps that are zero, negative, NaN or infinite.  tests/golden/gen_mv_depth_loss.py runs the reference's MVDepthLoss on
them and stores inputs and results in tests/golden/mv_depth_loss.npz."""
import numpy as np

import tsdf_ref

EPS_PX = 1e-3
EPS_REL = 1e-5
CAP = 0.01
RATIO, LOG_TOL = 1.05, 0.05
EPS_Z = float(np.float32(1e-5))  # Project3D's eps is a float32 buffer; the kernel's is 1e-5f

# name -> (h, w, B, K, seed): sizes that are no multiple of a tile or a workgroup, one and several maps, one, a few and the most sources
CASES = {"a": (13, 19, 1, 1, 11), "b": (13, 19, 3, 3, 12), "c": (24, 32, 1, 16, 13), "d": (24, 32, 3, 3, 14), "e": (24, 32, 1, 1, 15)}


def _valid(d):
    return np.isfinite(d) & (d > 0)


def _chain(depth, invK, E, P):
    """(B,h,w) depth -> projected (px, py, z) per source, each (B,K,h,w): the header's chain in fp64."""
    B, h, w = depth.shape
    v, u = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    pix = np.stack([u, v, np.ones_like(u)], 0).reshape(3, -1)
    with np.errstate(all="ignore"):
        q = invK[:, :3, :3] @ pix                                        # (B,3,N)
        cam = depth.reshape(B, 1, -1) * q
        X = E @ np.concatenate([cam, np.ones((B, 1, h * w))], 1)         # (B,4,N)
        c = P[:, :, :3] @ X[:, None]                                     # (B,K,3,N)
        z = np.maximum(c[:, :, 2], EPS_Z)                                # (a NaN stays a NaN, as in torch.maximum)
        px, py = c[:, :, 0] / z, c[:, :, 1] / z
    K = P.shape[1]
    return px.reshape(B, K, h, w), py.reshape(B, K, h, w), z.reshape(B, K, h, w)


def check(depth_b1hw, invK_b44, world_T_cam_b44, src_depth_bk1hw, src_K_bk44, src_cam_T_world_bk44, gate_depth=None, ratio=RATIO,
          log_tol=LOG_TOL, min_consistent=1, max_conflict=0):
    """All outputs of idh_mv_consistency_fwd in fp64, and ``ambiguous`` (B,K,h,w), ``ambiguous_pixel`` (B,h,w)."""
    f = lambda t: np.asarray(t, np.float32).astype(np.float64)
    d = f(depth_b1hw)[:, 0]
    B, h, w = d.shape
    src = f(src_depth_bk1hw)[:, :, 0]
    K = src.shape[1]
    invK, E = f(invK_b44), f(world_T_cam_b44)
    P = f(src_K_bk44) @ f(src_cam_T_world_bk44)
    ratio, log_tol = float(np.float32(ratio)), float(np.float32(log_tol))
    px, py, z_gate = _chain(d if gate_depth is None else f(gate_depth)[:, 0], invK, E, P)
    z_test = z_gate if gate_depth is None else _chain(d, invK, E, P)[2]
    with np.errstate(all="ignore"):
        xr, yr = np.rint(px - 0.5), np.rint(py - 0.5)                    # round-half-even
        inside = (xr >= 0) & (xr <= w - 1) & (yr >= 0) & (yr <= h - 1)
        xi, yi = np.where(inside, xr, 0).astype(np.int64), np.where(inside, yr, 0).astype(np.int64)
        bb, kk = np.meshgrid(np.arange(B), np.arange(K), indexing="ij")
        s = np.where(inside, src[bb[..., None, None], kk[..., None, None], yi, xi], 0.0)
        visible = (z_gate < ratio * s) & (z_gate > 0) & (s > 0)
        l = np.log(s) - np.log(z_test)
        err = np.abs(l)
        counted = visible & _valid(d)[:, None] & _valid(s) & inside
        consistent, conflict = counted & (err <= log_tol), counted & (l > log_tol)
        near = (px > -1) & (px < w + 1) & (py > -1) & (py < h + 1)
        amb = near & ((np.abs(px - np.rint(px)) < EPS_PX) | (np.abs(py - np.rint(py)) < EPS_PX))
        amb |= np.isfinite(s) & (s > 0) & (np.abs(z_gate - ratio * s) <= EPS_REL * ratio * s)
        amb |= counted & ((np.abs(err - log_tol) <= EPS_REL * log_tol) | (np.abs(l - log_tol) <= EPS_REL * log_tol))
    n_con, n_conf = consistent.sum(1), conflict.sum(1)
    kept = _valid(d) & (n_con >= min_consistent) & (n_conf <= max_conflict)
    take = visible & ~np.isnan(err)
    with np.errstate(all="ignore"):
        loss_sum = np.array([err[:, k][take[:, k]].sum() for k in range(K)], np.float64)
        loss_count = take.sum((0, 2, 3)).astype(np.int64)
        loss = float(np.mean(loss_sum / loss_count))
    return dict(visible=visible, err=np.where(visible, err, np.nan), sampled=s, inside=inside,
                counts=np.stack([visible.sum(1), n_con, n_conf], 1).astype(np.uint8), weight=np.where(kept, 1.0 + n_con, 0.0)[:, None],
                filtered_depth=np.where(kept, d, 0.0)[:, None], loss=loss, loss_sum=loss_sum, loss_count=loss_count, ambiguous=amb,
                ambiguous_pixel=amb.any(1))


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------

WALL_Z = 2.0  # the wall is the world plane z = 2


def _wall_depth(h, w, K, world_T_cam):
    """The camera's z of the wall at every pixel centre, (h,w) fp64."""
    v, u = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    q = np.linalg.inv(K)[:3, :3] @ np.stack([u, v, np.ones_like(u)], 0).reshape(3, -1)  # the point at depth d is d q in the camera
    R, t = world_T_cam[:3, :3], world_T_cam[:3, 3]
    return ((WALL_Z - t[2]) / (R[2] @ q)).reshape(h, w)


def _camera(r, h, w, spread):
    K = tsdf_ref._pinhole(0.9 * w + r.uniform(-1, 1), 0.9 * w + r.uniform(-1, 1), w / 2 + r.uniform(-1, 1), h / 2 + r.uniform(-1, 1))
    a = r.uniform(-1, 1, 3) * np.array([0.18, 0.14, 0.25]) * spread
    world_T_cam = tsdf_ref._pose(a[0], a[1], a[2], r.uniform(-1, 1, 3) * np.array([0.45, 0.3, 0.2]) * spread)
    return K, world_T_cam


def _patches(r, depth, n, factors):
    h, w = depth.shape
    for _ in range(n):
        i, j, f = r.integers(0, h - 3), r.integers(0, w - 4), r.choice(factors)
        depth[i:i + r.integers(2, 5), j:j + r.integers(2, 6)] *= f
    return depth


def _holes(r, depth, n, inf):
    flat = depth.reshape(-1)
    idx = r.choice(flat.size, size=4 * n, replace=False)
    for q, val in enumerate((0.0, -1.0, np.nan, np.inf if inf else 0.0)):
        flat[idx[q * n:(q + 1) * n]] = val
    return depth


def fixture(name):
    """Inputs of case ``name`` as float32 arrays: ``pred`` (B,1,h,w) the map under test, ``cur`` (B,1,h,w) the gate map (the wall with
    patches, without the noise), ``invK`` / ``world_T_cam`` (B,4,4), ``src_depth`` (B,K,1,h,w), ``src_K`` / ``src_cam_T_world`` (B,K,4,4)."""
    h, w, B, K, seed = CASES[name]
    r = np.random.default_rng(seed)
    inf = name == "b"  # an infinite tap passes the reference's gate and makes err and loss infinite: one case has them, the others a finite loss
    out = {k: [] for k in ("pred", "cur", "invK", "world_T_cam", "src_depth", "src_K", "src_cam_T_world")}
    for b in range(B):
        Kc, T = _camera(r, h, w, 0.4)
        cur = _patches(r, _wall_depth(h, w, Kc, T), 3, (0.7, 0.85, 1.2, 1.4))
        pred = cur * (1 + 0.02 * r.standard_normal((h, w)))
        cur, pred = _holes(r, cur, 1, inf), _holes(r, pred, 2, inf)
        sd, sK, sE = [], [], []
        for k in range(K):
            Ks, Ts = _camera(r, h, w, 2.0 if k % 4 == 3 else 1.0)  # every fourth source looks well away: projections off the image
            if k == 2 and inf:  # (case b) one source behind the tested camera's wall points: the 1e-5 clamp
                Ts = tsdf_ref._pose(np.pi, 0.0, 0.0, np.array([0.0, 0.0, 0.5 * WALL_Z])) @ Ts
            dep = _wall_depth(h, w, Ks, Ts) * (1 + 0.01 * r.standard_normal((h, w)))
            sd.append(_holes(r, _patches(r, dep, 2, (0.75, 1.3)), 2, inf))
            sK.append(Ks), sE.append(np.linalg.inv(Ts))
        for k_, v_ in zip(out, (pred[None], cur[None], np.linalg.inv(Kc), T, np.stack(sd)[:, None], np.stack(sK), np.stack(sE))):
            out[k_].append(v_)
    out = {k_: np.stack(v_).astype(np.float32) for k_, v_ in out.items()}
    return settle(out)


def _args(fx, gate):
    return (fx["pred"], fx["invK"], fx["world_T_cam"], fx["src_depth"], fx["src_K"], fx["src_cam_T_world"], fx["cur"] if gate else None)


def ambiguous_share(fx):
    """The larger share of ambiguous pixels of the two uses of a fixture: gated by ``cur``, and the tested map gating itself."""
    return max(float(check(*_args(fx, g))["ambiguous_pixel"].mean()) for g in (True, False))


def settle(fx, rounds=8):
    """Nudge the depth of ambiguous pixels (both maps, by a few tenths of a percent: less than the noise) until hardly any is left."""
    r = np.random.default_rng(99)
    for _ in range(rounds):
        amb = check(*_args(fx, True))["ambiguous_pixel"] | check(*_args(fx, False))["ambiguous_pixel"]
        if amb.mean() <= CAP / 4:
            break
        f = (1 + r.uniform(0.001, 0.004, amb.shape) * r.choice([-1, 1], amb.shape)).astype(np.float32)
        for k in ("pred", "cur"):
            fx[k][:, 0] = np.where(amb, fx[k][:, 0] * f, fx[k][:, 0])
    return fx


# ---- weighted integrate --------------------------------------------------------------------------------------------------------------

def integrate_weighted(values, depths, weights, Ks, cam_T_worlds, origin, voxel_size, trunc_voxels=3.0, max_weight=64.0):
    """``tsdf_ref.integrate`` with a weight map (1,h,w) per depth map: the same projection and the same ambiguity, T in fp64, W restated
    in float32 (W + g and the cap are single fp32 operations of the kernel).  Returns its dict (without the per-map counts)."""
    values = np.asarray(values)
    T, W = values[..., 0].astype(np.float64), values[..., 1].copy()
    touched, amb = np.zeros(W.shape, bool), np.zeros(W.shape, bool)
    trunc = tsdf_ref.trunc_of(trunc_voxels, voxel_size)
    for depth, g, K, E in zip(depths, weights, Ks, cam_T_worlds):
        g32 = np.asarray(g, np.float32).reshape(g.shape[-2:])
        d32 = np.asarray(depth, np.float32).reshape(depth.shape[-2:])
        good = np.isfinite(g32) & (g32 > 0)
        # the voxels map m updates and their s: from tsdf_ref on an empty volume, where T after one update IS s and W is 1
        one = tsdf_ref.integrate(tsdf_ref.empty_volume(W.shape), [np.where(good, d32, 0)], [K], [E], origin, voxel_size, trunc_voxels, max_weight)
        upd, s = one["touched"], one["T"]
        gw = _tap_weights(g32, K, E, origin, voxel_size, W.shape)  # the weight at the tap each voxel read
        assert (gw[upd] > 0).all()
        W64 = W.astype(np.float64)
        with np.errstate(all="ignore"):
            T = np.where(upd, (W64 * T + gw * s) / (W64 + gw), T)
        W = np.where(upd, np.minimum(W + gw.astype(np.float32), np.float32(max_weight)), W)
        touched |= upd
        amb |= one["ambiguous"]
    return dict(T=T, W=W, touched=touched, ambiguous=amb)


def _tap_weights(g32, K, E, origin, voxel_size, dims):
    """The weight each voxel taps: the projection of tsdf_ref.integrate (same expressions), (Nz,Ny,Nx) fp64; 0 where there is no tap."""
    Nz, Ny, Nx = dims
    h, w = g32.shape
    v, o = float(np.float32(voxel_size)), np.asarray(origin, np.float32).astype(np.float64)
    K, E = np.asarray(K, np.float32).astype(np.float64), np.asarray(E, np.float32).astype(np.float64)
    zz, yy, xx = np.meshgrid(np.arange(Nz), np.arange(Ny), np.arange(Nx), indexing="ij")
    p = np.stack([o[0] + v * xx, o[1] + v * yy, o[2] + v * zz], -1)
    c = p @ E[:3, :3].T + E[:3, 3]
    front = c[..., 2] > 0
    cz = np.where(front, c[..., 2], 1.0)
    px, py = K[0, 0] * (c[..., 0] / cz) + K[0, 2], K[1, 1] * (c[..., 1] / cz) + K[1, 2]
    inside = front & (px >= 0) & (px < w) & (py >= 0) & (py < h)
    j, i = np.where(inside, np.floor(px), 0).astype(np.int64), np.where(inside, np.floor(py), 0).astype(np.int64)
    g = np.where(inside, g32[i, j], 0.0).astype(np.float64)
    return np.where(np.isfinite(g) & (g > 0), g, 0.0)
