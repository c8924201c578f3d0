"""fp64 numpy statement of the shaded render's semantics (include/idh_raster.h), written independently of the kernels,
on top of tests/raster_ref.py: per pixel the nearest hit, the second-nearest hit of ANOTHER face, the winning face, its barycentrics, and
from those interpolated attributes and the colour before rounding.  ``restate_f32`` restates the kernel's expressions in float32 numpy for
given (pixel, face) pairs: its distance from the fp64 values is the error any fp32 implementation of those expressions has, the
baseline the GPU tests measure the kernel against.

A pixel is *ambiguous* when ``raster_ref`` marks it (within ``EDGE_PX`` of a candidate edge line) or two different faces are within
``ZFIGHT * z`` of each other there: another fp32 implementation may pick the other face."""
import functools

import numpy as np

import raster_ref as rr

ZFIGHT = 1e-3


def _setup(verts, faces, cam_T_world, K, H, W):
    K = np.asarray(K, np.float64)
    P = rr._camera(verts, cam_T_world)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    DX, DY = (jj + 0.5 - K[0, 2]) / K[0, 0], (ii + 0.5 - K[1, 2]) / K[1, 1]
    return K, P, DX, DY


def _face_terms(P, tri, dx, dy):
    """For faces ``tri`` (n,3) and rays (dx, dy, 1) (n,): edge functions e (n,3) and k = N.A, all signed so that k > 0, and N."""
    A, B, C = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
    d = np.stack([dx, dy, np.ones_like(dx)], -1)
    n = [np.cross(B, C), np.cross(C, A), np.cross(A, B)]
    N = np.cross(B - A, C - A)
    k = (N * A).sum(-1)
    s = np.where(k > 0, 1.0, -1.0)
    e = np.stack([(d * m).sum(-1) for m in n], -1) * s[:, None]
    return e, k * s, N * s[:, None], d


def render(verts, faces, cam_T_world, K, H, W):
    """One camera.  Returns a dict of (H,W) arrays: ``z`` nearest depth (inf where empty), ``z2`` nearest depth of another face (inf
    where none), ``face`` (int64, -1 where empty; the lowest index among exactly equal depths), ``bary`` (H,W,3), ``lam`` (the headlight
    factor d.N / (|d| |N|) of the winning face), ``covered``, ``ambiguous``, and ``depth`` / ``edge_ambiguous`` as raster_ref.render
    returns them."""
    verts, faces = np.asarray(verts), np.asarray(faces)
    Km, P, DX, DY = _setup(verts, faces, cam_T_world, K, H, W)
    fx, fy, cx, cy = Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2]
    z1, z2 = np.full((H, W), np.inf), np.full((H, W), np.inf)
    face = np.full((H, W), -1, np.int64)
    nV = len(P)
    for fi, f in enumerate(faces):
        if (f < 0).any() or (f >= nV).any():
            continue
        A, B, C = P[f[0]], P[f[1]], P[f[2]]
        if not np.isfinite(np.stack([A, B, C])).all():
            continue
        zs = np.array([A[2], B[2], C[2]])
        if (zs <= 0).all():
            continue
        if (zs > 0).all():
            u = fx * np.array([A[0], B[0], C[0]]) / zs + cx
            v = fy * np.array([A[1], B[1], C[1]]) / zs + cy
            x0, x1 = int(max(np.floor(u.min() - 1.5), 0)), int(min(np.ceil(u.max() + 0.5), W - 1))
            y0, y1 = int(max(np.floor(v.min() - 1.5), 0)), int(min(np.ceil(v.max() + 0.5), H - 1))
            if x1 < x0 or y1 < y0:
                continue
        else:
            x0, x1, y0, y1 = 0, W - 1, 0, H - 1
        dx, dy = DX[y0:y1 + 1, x0:x1 + 1], DY[y0:y1 + 1, x0:x1 + 1]
        n = [np.cross(B, C), np.cross(C, A), np.cross(A, B)]
        e = [dx * m[0] + dy * m[1] + m[2] for m in n]
        k = float(np.dot(A, n[0]))
        if k == 0:
            continue
        s = 1.0 if k > 0 else -1.0
        inside = (s * e[0] >= 0) & (s * e[1] >= 0) & (s * e[2] >= 0)
        den = s * (e[0] + e[1] + e[2])
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(inside & (den > 0), s * k / den, np.inf)
        z = np.where(z > 0, z, np.inf)
        a1, a2, af = z1[y0:y1 + 1, x0:x1 + 1], z2[y0:y1 + 1, x0:x1 + 1], face[y0:y1 + 1, x0:x1 + 1]
        closer = z < a1  # strict: among equal depths the first (lowest) face stays
        a2[...] = np.where(closer, a1, np.minimum(a2, z))
        af[...] = np.where(closer, fi, af)
        a1[...] = np.where(closer, z, a1)
    covered = np.isfinite(z1)
    bary, lam = np.zeros((H, W, 3)), np.zeros((H, W))
    if covered.any():
        e, k, N, d = _face_terms(P, faces[face[covered]], DX[covered], DY[covered])
        bary[covered] = e / e.sum(-1, keepdims=True)
        lam[covered] = (d * N).sum(-1) / np.sqrt((N * N).sum(-1) * (d * d).sum(-1))
    depth, edge_amb = rr.render(verts, faces, cam_T_world, K, H, W)
    with np.errstate(invalid="ignore"):
        zfight = covered & (z2 - z1 <= ZFIGHT * z1)
    return dict(z=z1, z2=z2, face=face, bary=bary, lam=lam, covered=covered, zfight=zfight, edge_ambiguous=edge_amb,
                ambiguous=edge_amb | zfight, depth=depth)


def face_depth(verts, faces, cam_T_world, K, H, W, pix_to_face):
    """fp64 depth, at every pixel, of the plane of the face ``pix_to_face`` (H,W) names there (nan where it names none)."""
    _, P, DX, DY = _setup(verts, faces, cam_T_world, K, H, W)
    out = np.full((H, W), np.nan)
    m = np.asarray(pix_to_face) >= 0
    if m.any():
        e, k, N, d = _face_terms(P, np.asarray(faces)[np.asarray(pix_to_face)[m]], DX[m], DY[m])
        out[m] = k / (d * N).sum(-1)
    return out


def interpolate(ref, faces, values):
    """(H,W,C) fp64: per-vertex ``values`` (V,C) interpolated with the reference's barycentrics over its winning face, 0 where empty."""
    values, faces = np.asarray(values, np.float64), np.asarray(faces)
    out = np.zeros(ref["face"].shape + (values.shape[1],))
    m = ref["covered"]
    tri = faces[ref["face"][m]]
    out[m] = sum(ref["bary"][m][:, i:i + 1] * values[tri[:, i]] for i in range(3))
    return out


def colour(ref, faces, colors, ambient):
    """(H,W,4) fp64 colour before rounding: interpolated uint8 channels, RGB times ambient + (1 - ambient) * lam, alpha unlit."""
    c = interpolate(ref, faces, np.asarray(colors, np.float64))
    c[..., :3] *= (ambient + (1.0 - ambient) * ref["lam"])[..., None]
    return c


def round_u8(c):
    return np.floor(np.clip(c, 0.0, 255.0) + 0.5).astype(np.int64)


def restate_f32(verts, faces, cam_T_world, K, ys, xs, fidx, attrs=None, colors=None, ambient=0.3):
    """The kernel's expressions (csrc/raster_common.h: to_camera, edge_normal, tri_setup, shade; csrc/raster_shade.hip: the shade pass) in
    float32 numpy, operation by operation and in the kernel's order, for pixels (ys, xs) and faces fidx.  Returns a dict: ``z``,
    ``bary`` (n,3), ``lam``, and with ``attrs`` / ``colors`` the interpolated attributes and the colour before rounding."""
    f32 = np.float32
    T, Km, v = np.asarray(cam_T_world, f32), np.asarray(K, f32), np.asarray(verts, f32)
    tri = np.asarray(faces)[fidx]

    def cam(idx):
        X, Y, Z = v[idx, 0], v[idx, 1], v[idx, 2]
        return [T[r, 0] * X + T[r, 1] * Y + T[r, 2] * Z + T[r, 3] for r in range(3)]

    sub = lambda a, b: [a[0] - b[0], a[1] - b[1], a[2] - b[2]]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    def edge_normal(Pv, ip, Qv, iq):
        swap = ip > iq
        L = [np.where(swap, q, p) for p, q in zip(Pv, Qv)]
        Hi = [np.where(swap, p, q) for p, q in zip(Pv, Qv)]
        n = cross(L, sub(Hi, L))
        return [np.where(swap, -c, c) for c in n]

    ia, ib, ic = tri[:, 0], tri[:, 1], tri[:, 2]
    A, B, C = cam(ia), cam(ib), cam(ic)
    N = cross(sub(B, A), sub(C, A))
    k = dot(N, A)
    s = np.where(k > 0, f32(1), f32(-1))
    N = [c * s for c in N]
    k = k * s
    n0 = [c * s for c in edge_normal(B, ib, C, ic)]
    n1 = [c * s for c in edge_normal(C, ic, A, ia)]
    n2 = [c * s for c in edge_normal(A, ia, B, ib)]
    d = [(np.asarray(xs).astype(f32) + f32(0.5) - Km[0, 2]) / Km[0, 0], (np.asarray(ys).astype(f32) + f32(0.5) - Km[1, 2]) / Km[1, 1],
         np.ones(len(tri), f32)]
    e0, e1, e2 = dot(d, n0), dot(d, n1), dot(d, n2)
    ssum = e0 + e1 + e2
    w = [e0 / ssum, e1 / ssum, e2 / ssum]
    den = dot(d, N)
    out = {"z": k / den, "bary": np.stack(w, -1), "lam": den / np.sqrt(dot(N, N) * dot(d, d))}
    assert all(x.dtype == f32 for x in (out["z"], out["bary"], out["lam"]))
    if attrs is not None:
        a = np.asarray(attrs, f32)
        out["attrs"] = w[0][:, None] * a[ia] + w[1][:, None] * a[ib] + w[2][:, None] * a[ic]
    if colors is not None:
        c = np.asarray(colors).astype(f32)
        col = w[0][:, None] * c[ia] + w[1][:, None] * c[ib] + w[2][:, None] * c[ic]
        light = f32(ambient) + (f32(1) - f32(ambient)) * out["lam"]
        col[:, :3] = col[:, :3] * light[:, None]
        out["colour"] = col
    return out


# ---- the committed scenes, rendered once per process ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general_case(case):
    """(name, H, W, verts, faces, cams, K, [reference of camera 0, of camera 1]) of raster_ref.general_cases()[case]."""
    name, H, W, verts, faces, cams, K = list(rr.general_cases())[case]
    refs = [render(verts.numpy(), faces.numpy(), cams[b].numpy(), K[b].numpy(), H, W) for b in range(2)]
    return name, H, W, verts, faces, cams, K, refs


def vertex_attrs(V, C, seed):
    return np.random.default_rng(seed).standard_normal((V, C)).astype(np.float32)


def vertex_colors(V, seed):
    """Random RGBA with alpha >= 64: a covered pixel's alpha then never rounds to 0, which means "no asset"."""
    c = np.random.default_rng(seed).integers(0, 256, (V, 4))
    c[:, 3] = 64 + c[:, 3] * 3 // 4
    return c.astype(np.uint8)
