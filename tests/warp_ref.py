"""fp64 numpy statement of the depth warp's semantics (include/idh_raster.h: idh_depth_warp_fwd), written independently
of the kernels.  ``build`` turns one source depth map into the explicit vertex and face lists the kernels never form - the tear rule is
evaluated in ``np.float32``, which restates the kernel's one multiply and one compare exactly - and ``render`` is the brute force over
the drawn faces of all sources: nearest hit per pixel, the id of the winner, and what another floating-point implementation may decide
the other way.

A pixel is *ambiguous* when its centre is within ``raster_ref.EDGE_PX`` of a projected edge SEGMENT of a drawn face whose grown box holds
it.  (``raster_ref`` measures the distance to the edge's whole line, which is meant for triangles of 3 px and marks too much for triangles
of 1 px.)  For a face that crosses z = 0 the projection of an edge is not the segment between its projected ends: ``raster_ref``'s
whole-image line rule is kept there."""
import functools

import numpy as np

import raster_ref as rr

SMALL_BOX = 64  # pixel centres one lane resolves in place (csrc/raster_common.h: kSmallBox); above it a face goes through the queue


def build(depth, invK, cam_T_src, tear_ratio=1.1):
    """One source in the target camera: (verts (h*w,3) fp64, faces (2(h-1)(w-1),3) int64, draws (faces,) bool, valid (h,w) bool)."""
    d32 = np.asarray(depth, np.float32)
    h, w = d32.shape
    iK, T = np.asarray(invK, np.float64), np.asarray(cam_T_src, np.float64)
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rays = np.stack([jj + 0.5, ii + 0.5, np.ones((h, w))], -1) @ iK[:3, :3].T
    valid = np.isfinite(d32) & (d32 > 0)
    src = np.where(valid, d32, 0).astype(np.float64)[..., None] * rays  # invalid vertices are never referenced by a drawn face
    verts = (src @ T[:3, :3].T + T[:3, 3]).reshape(-1, 3)
    qi, qj = np.meshgrid(np.arange(h - 1), np.arange(w - 1), indexing="ij")
    v00 = (qi * w + qj).reshape(-1)
    v01, v10, v11 = v00 + 1, v00 + w, v00 + w + 1
    faces = np.stack([np.stack([v00, v10, v01], -1), np.stack([v01, v10, v11], -1)], 1).reshape(-1, 3)  # face 2q, face 2q + 1
    fvalid = valid.reshape(-1)[faces].all(1)
    fd = np.where(fvalid[:, None], d32.reshape(-1)[faces], np.float32(1))
    with np.errstate(over="ignore"):
        keep = fd.max(1) <= fd.min(1) * np.float32(tear_ratio)  # float32 * float32, one compare
    assert fd.dtype == np.float32
    return verts, faces, fvalid & keep, valid


def _segment_distance(px, py, a, b):
    ab = b - a
    L2 = float(ab @ ab)
    t = np.zeros_like(px) if L2 == 0 else np.clip(((px - a[0]) * ab[0] + (py - a[1]) * ab[1]) / L2, 0.0, 1.0)
    return np.hypot(px - (a[0] + t * ab[0]), py - (a[1] + t * ab[1]))


def render(depths, invKs, cam_T_srcs, K, H, W, tear_ratio=1.1):
    """Brute force of M sources in one target camera.  Returns a dict: ``depth`` (H,W) fp64, -1 where empty; ``source`` (H,W) int64 id
    of the winner (the lowest among equal depths), -1 where empty; ``ambiguous`` (H,W) bool; ``drawn`` faces drawn in all; ``large``
    front faces whose box holds more than SMALL_BOX pixel centres; ``crossing`` drawn faces with corners on both sides of z = 0."""
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    PX, PY = jj + 0.5, ii + 0.5
    DX, DY = (PX - cx) / fx, (PY - cy) / fy
    best = np.full((H, W), np.inf)
    win = np.full((H, W), -1, np.int64)
    amb = np.zeros((H, W), bool)
    drawn = large = crossing = 0
    for m, (depth, invK, T) in enumerate(zip(depths, invKs, cam_T_srcs)):
        verts, faces, draws, _ = build(depth, invK, T, tear_ratio)
        for f in np.nonzero(draws)[0]:
            A, B, C = verts[faces[f]]
            if not np.isfinite(np.stack([A, B, C])).all():
                continue
            zs = np.array([A[2], B[2], C[2]])
            if (zs <= 0).all():
                continue
            drawn += 1
            front = bool((zs > 0).all())
            if front:
                u = fx * np.array([A[0], B[0], C[0]]) / zs + cx
                v = fy * np.array([A[1], B[1], C[1]]) / zs + cy
                nx = min(np.floor(u.max() - 0.5), W - 1) - max(np.ceil(u.min() - 0.5), 0) + 1
                ny = min(np.floor(v.max() - 0.5), H - 1) - max(np.ceil(v.min() - 0.5), 0) + 1
                large += bool(nx > 0 and ny > 0 and nx * ny > SMALL_BOX)
                x0, x1 = int(max(np.floor(u.min() - 1.5), 0)), int(min(np.ceil(u.max() + 0.5), W - 1))
                y0, y1 = int(max(np.floor(v.min() - 1.5), 0)), int(min(np.ceil(v.max() + 0.5), H - 1))
                if x1 < x0 or y1 < y0:
                    continue
            else:
                crossing += 1
                x0, x1, y0, y1 = 0, W - 1, 0, H - 1
            box = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            dx, dy = DX[box], DY[box]
            n = [np.cross(B, C), np.cross(C, A), np.cross(A, B)]
            e = [dx * q[0] + dy * q[1] + q[2] for q in n]
            if front:
                px, py = PX[box], PY[box]
                corners = np.stack([u, v], -1)
                for a, b in ((1, 2), (2, 0), (0, 1)):
                    amb[box] |= _segment_distance(px, py, corners[a], corners[b]) < rr.EDGE_PX
            else:
                for q, ei in zip(n, e):
                    g = np.hypot(q[0] / fx, q[1] / fy)
                    amb[box] |= (np.abs(ei) < rr.EDGE_PX * g) if g > 0 else (ei == 0)
            k = float(np.dot(A, n[0]))
            if k == 0:
                continue
            s = 1.0 if k > 0 else -1.0
            inside = (s * e[0] >= 0) & (s * e[1] >= 0) & (s * e[2] >= 0)
            den = s * (e[0] + e[1] + e[2])
            with np.errstate(divide="ignore", invalid="ignore"):
                z = np.where(inside & (den > 0), s * k / den, np.inf)
            z = np.where(z > 0, z, np.inf)
            closer = z < best[box]  # strict: among equal depths the first (lowest id) stays
            win[box] = np.where(closer, m * len(faces) + f, win[box])
            best[box] = np.where(closer, z, best[box])
    return dict(depth=np.where(np.isfinite(best), best, -1.0), source=win, ambiguous=amb, drawn=drawn, large=large, crossing=crossing)


def face_depth(depths, invKs, cam_T_srcs, K, H, W, source):
    """fp64 depth, at every pixel, of the plane of the face ``source`` (H,W) names there (nan where it names none): the face's corners
    rebuilt from the id alone, as a caller of ``decode_source`` would."""
    K = np.asarray(K, np.float64)
    source = np.asarray(source, np.int64)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    d = np.stack([(jj + 0.5 - K[0, 2]) / K[0, 0], (ii + 0.5 - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)
    out = np.full((H, W), np.nan)
    for m, (depth, invK, T) in enumerate(zip(depths, invKs, cam_T_srcs)):
        verts, faces, _, _ = build(depth, invK, T, np.inf)
        sel = (source >= 0) & (source // len(faces) == m)
        if sel.any():
            A, B, C = (verts[faces[source[sel] % len(faces)][:, i]] for i in range(3))
            N = np.cross(B - A, C - A)
            out[sel] = (N * A).sum(-1) / (N * d[sel]).sum(-1)
    return out


def source_id(m, i, j, upper, h, w):
    """The id of face (source m, quad with top-left vertex (i, j), upper 0 / 1): m * 2 (h-1) (w-1) + 2 q + upper, q = i (w-1) + j."""
    return m * (2 * (h - 1) * (w - 1)) + 2 * (i * (w - 1) + j) + upper


def compare(got, ref, empty_depth=-1.0, rtol=1e-4):
    """(coverage mismatches outside ambiguous pixels, largest relative depth error over unambiguous pixels covered in both, whether
    every unambiguous pixel the reference leaves empty holds exactly ``empty_depth``)."""
    got = np.asarray(got, np.float64)
    ok = ~ref["ambiguous"]
    cov_r = ref["depth"] > 0
    cov_g = got != empty_depth
    both = ok & cov_r & cov_g
    err = float((np.abs(got[both] - ref["depth"][both]) / ref["depth"][both]).max()) if both.any() else 0.0
    return int((ok & (cov_g != cov_r)).sum()), err, bool((got[ok & ~cov_r] == empty_depth).all())


# ---- the committed scenes --------------------------------------------------------------------------------------------
SRC_H, SRC_W = 24, 32
BOX = (slice(8, 16), slice(10, 20))  # the foreground box, about 1.2 m in front of a surface at about 2 m


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


def source_K():
    return _pinhole(28.9, 28.4, 15.6, 12.3)


def source_depth(seed=0, box=True, holes=True):
    """(24,32) float32: a smooth surface about 2 m away, a tilted box 1.15 - 1.3 m away in front of it, and a few taps that are zero,
    NaN, negative or infinite."""
    r = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(SRC_H), np.arange(SRC_W), indexing="ij")
    d = 2.0 + 0.25 * np.sin(0.21 * jj + 0.4 * seed) * np.cos(0.17 * ii) + 0.004 * r.standard_normal((SRC_H, SRC_W))
    if box:
        d[BOX] = (1.15 + 0.015 * (jj - 10) + 0.004 * (ii - 8))[BOX]
    d = d.astype(np.float32)
    if holes:
        d[3, 5], d[3, 6], d[19, 27], d[12, 14], d[20, 4], d[5, 25] = 0.0, np.nan, np.nan, 0.0, -1.5, np.inf
    return d


GENERIC_POSE = _pose(0.07, -0.04, 0.06, (0.12, -0.05, 0.075))  # about 0.1 rad (with some roll: mesh edges cross the pixel grid) and 0.15 m
CLOSE_POSE = _pose(0.3, 0.02, 0.03, (-0.12, 0.02, -1.18))      # the target camera stands inside the box's depth range: faces of it cross z = 0

# name -> (H, W, K, cam_T_src)
TARGETS = {
    "24x32": (24, 32, _pinhole(28.9, 28.4, 17.2, 11.1), GENERIC_POSE),
    "48x64": (48, 64, _pinhole(57.8, 56.8, 29.7, 26.4), GENERIC_POSE),
    "30x44": (30, 44, _pinhole(38.3, 36.1, 23.4, 13.2), GENERIC_POSE),
    "closeup": (40, 56, _pinhole(120.0, 118.0, 27.3, 19.1), CLOSE_POSE),
}
PLAIN = ("24x32", "48x64", "30x44")


def scene_inputs(name):
    """(depth (1,24,32) float32, invK (1,4,4), cam_T_src (1,4,4), K (4,4), H, W): float32 arrays, what the kernels are given; the
    reference reads the same float32 values."""
    H, W, K, T = TARGETS[name]
    f = lambda x: np.asarray(x, np.float64).astype(np.float32)
    return source_depth()[None], f(np.linalg.inv(source_K()))[None], f(T)[None], f(K), H, W


@functools.lru_cache(maxsize=None)
def scene_reference(name, tear_ratio=1.1):
    depth, invK, T, K, H, W = scene_inputs(name)
    return render(depth, invK, T, K, H, W, tear_ratio)


def plane_case():
    """A source looking at the plane n.X = c, a generic second camera, and the closed form in it.  Returns (depth (1,24,32) float32,
    invK, cam_T_src, K, H, W, want (H,W) fp64 depth of the plane in the target, inside (H,W) bool: the hit point projects at least
    1 px inside the hull of the source's vertices)."""
    n, c = np.array([0.25, -0.15, 1.0]), 2.1
    iK = np.linalg.inv(source_K()).astype(np.float32).astype(np.float64)
    ii, jj = np.meshgrid(np.arange(SRC_H), np.arange(SRC_W), indexing="ij")
    rays = np.stack([jj + 0.5, ii + 0.5, np.ones((SRC_H, SRC_W))], -1) @ iK[:3, :3].T
    depth = (c / (rays @ n)).astype(np.float32)  # rays have z = 1 up to rounding: the depth is the z of the hit
    H, W, K, T = TARGETS["30x44"]
    T = T.astype(np.float32).astype(np.float64)
    K = K.astype(np.float32).astype(np.float64)
    nt = T[:3, :3] @ n
    ct = c + nt @ T[:3, 3]
    tj, ti = np.meshgrid(np.arange(W), np.arange(H))
    d = np.stack([(tj + 0.5 - K[0, 2]) / K[0, 0], (ti + 0.5 - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)
    want = ct / (d @ nt)
    hit_src = ((want[..., None] * d) - T[:3, 3]) @ T[:3, :3]  # R^T (X - t)
    Ks = np.linalg.inv(iK)
    us = Ks[0, 0] * hit_src[..., 0] / hit_src[..., 2] + Ks[0, 2]
    vs = Ks[1, 1] * hit_src[..., 1] / hit_src[..., 2] + Ks[1, 2]
    inside = (want > 0) & (hit_src[..., 2] > 0) & (us >= 1.5) & (us <= SRC_W - 1.5) & (vs >= 1.5) & (vs <= SRC_H - 1.5)
    f = lambda x: np.asarray(x).astype(np.float32)
    return depth[None], f(iK)[None], f(T)[None], f(K), H, W, want, inside
