"""Reference for the surface-normal kernels (include/idh_geometry.h, csrc/normals.hip): an fp64 numpy restatement of the contract, written
with explicit index maps and slices, and the torch fp32 composition that the reference's NormalGenerator executes through kornia 0.6.7
(utils/geometry_utils.py:121-138): F.pad(reflect) + conv2d twice, BackprojectDepth, F.pad(replicate) + conv2d, torch.cross, F.normalize.
The composition is the yardstick for accuracy: a kernel may differ from fp64 by a small factor of what the composition differs by.

The contract was restated from the library's documented definition (gaussian_blur2d: separable, reflect border; spatial_gradient: Sobel,
order 1, normalised, replicate border); kornia is not installed, so neither form here is machine-checked against it."""
import numpy as np
import torch
import torch.nn.functional as F

KS = (1, 3, 5, 7)
SOBEL_X = np.array([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]]) / 8.0
SOBEL_Y = SOBEL_X.T.copy()
EPS = 1e-12
FACTOR = 4.0                                  # the kernel's error may be this many times the composition's (other summation order)
FLOOR = 4.0 * float(np.finfo(np.float32).eps)  # ... or a few fp32 ulps of 1.0 where the composition happens to be exact


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
SCALES = (1.0, 0.7, 1.3)  # the second batch element is scaled by 0.7 (a third one by 1.3)


def field(B, H, W):
    """(B,1,H,W) fp32: a smooth depth with a step of 1.0 in one quadrant."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, v = x / W, y / H
    d = 2.5 + 1.2 * np.sin(5 * u + 1) + 0.8 * np.cos(4 * v) + 0.3 * np.sin(9 * u * v)
    d = d + 1.0 * ((v > 0.6) & (u > 0.5))
    return torch.from_numpy(np.stack([d * SCALES[b % 3] for b in range(B)])[:, None].astype(np.float32))


def inv_intrinsics(B, H, W):
    """(B,4,4) fp32: non-square, off-centre, another focal length and centre per batch element."""
    out = np.zeros((B, 4, 4))
    for b in range(B):
        K = np.eye(4)
        K[0, 0], K[1, 1] = 0.9 * W * (1 + 0.1 * b), 1.2 * W * (1 + 0.1 * b)
        K[0, 2], K[1, 2] = W / 2 + 1.3 + 0.5 * b, H / 2 - 0.7
        out[b] = np.linalg.inv(K)
    return torch.from_numpy(out.astype(np.float32))


def rotations(B, seed=3):
    """(B,3,3) fp32 proper rotations."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((B, 3, 3)))
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return torch.from_numpy(q.astype(np.float32))


# ---- the contract in fp64 --------------------------------------------------------------------------------------------------------------
def gauss_weights(k, s):
    """fp32 weights exp(-(i - k//2)^2 / (2 s^2)) / sum."""
    x = np.arange(k, dtype=np.float32) - np.float32(k // 2)
    g = np.exp(-(x * x) / np.float32(2.0 * s * s)).astype(np.float32)
    return (g / g.sum(dtype=np.float32)).astype(np.float32)


def reflect(i, n):
    """`reflect` padding's source index: -1 -> 1, n -> n - 2."""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _maps(H, W, k):
    """For the two blur passes the source rows / columns of tap j: reflect(arange + j - k//2)."""
    r = k // 2
    return [reflect(np.arange(H) + j - r, H) for j in range(k)], [reflect(np.arange(W) + j - r, W) for j in range(k)]


def blur64(d, k, s):
    """(B,H,W) fp64 -> the separable blur: horizontal pass first, then vertical, each with reflect padding."""
    if k == 1:
        return d.copy()
    g = gauss_weights(k, s).astype(np.float64)
    rows, cols = _maps(d.shape[1], d.shape[2], k)
    hb = sum(g[j] * d[:, :, cols[j]] for j in range(k))
    return sum(g[j] * hb[:, rows[j], :] for j in range(k))


def backproject64(d, invK):
    """(B,H,W), (B,4,4) -> (B,3,H,W): d * (invK[:3,:3] @ (x + 0.5, y + 0.5, 1))."""
    B, H, W = d.shape
    y, x = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    K = invK.astype(np.float64)
    ray = np.stack([K[:, c, 0, None, None] * x + K[:, c, 1, None, None] * y + K[:, c, 2, None, None] for c in range(3)], 1)
    return d[:, None] * ray


def _taps(H, W):
    """Replicate padding of 1: the source rows / columns of the three taps."""
    return [np.clip(np.arange(H) + t - 1, 0, H - 1) for t in range(3)], [np.clip(np.arange(W) + t - 1, 0, W - 1) for t in range(3)]


def normal_of_gradients(gx, gy, axis):
    n = np.cross(gx, gy, axis=axis)
    with np.errstate(invalid="ignore", divide="ignore"):
        return n / np.maximum(np.sqrt((n * n).sum(axis, keepdims=True)), EPS)  # np.maximum keeps NaN, as clamp_min


def dense(depth, invK, k=5, s=2.0, world_R_cam=None, orient=False, flags=None, need=3):
    """The contract for (B,1,H,W) depth: (normals (B,3,H,W) fp64, valid (B,1,H,W) uint8 | None, n . p of the unflipped camera-space normal)."""
    d = np.asarray(depth, dtype=np.float64)[:, 0]
    B, H, W = d.shape
    with np.errstate(invalid="ignore", over="ignore"):
        pts = backproject64(blur64(d, k, s), np.asarray(invK))
        rows, cols = _taps(H, W)
        gx, gy = np.zeros_like(pts), np.zeros_like(pts)
        for i in range(3):
            for j in range(3):  # every tap, the zero ones too: 0 * NaN = NaN, as in the convolution
                nb = pts[:, :, rows[i]][:, :, :, cols[j]]
                gx, gy = gx + SOBEL_X[i, j] * nb, gy + SOBEL_Y[i, j] * nb
        n = normal_of_gradients(gx, gy, 1)
        dot = (n * pts).sum(1)
        if orient:
            n = np.where((dot > 0)[:, None], -n, n)
        if world_R_cam is not None:
            n = np.einsum("bij,bjhw->bihw", np.asarray(world_R_cam, dtype=np.float64), n)
    valid = None
    if flags is not None:
        ok = np.asarray(flags)[:, 0] == need
        if k > 1:
            brow, bcol = _maps(H, W, k)
            ok = np.logical_and.reduce([ok[:, :, c] for c in bcol])
            ok = np.logical_and.reduce([ok[:, r, :] for r in brow])
        ok = np.logical_and.reduce([ok[:, rows[i]][:, :, cols[j]] for i in range(3) for j in range(3)])
        n = np.where(ok[:, None], n, 0.0)
        valid = ok[:, None].astype(np.uint8)
    return n, valid, dot


def patch(points, cam_centre=None, orient=False, flags=None, need=3):
    """The contract for (B,N,9,3) patches: (normals (B,N,3) fp64, valid (B,N) uint8 | None, n . view of the unflipped normal)."""
    p = np.asarray(points, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        gx = sum(SOBEL_X.reshape(-1)[t] * p[:, :, t] for t in range(9))
        gy = sum(SOBEL_Y.reshape(-1)[t] * p[:, :, t] for t in range(9))
        n = normal_of_gradients(gx, gy, -1)
        dot = None
        if orient:
            dot = (n * (p[:, :, 4] - np.asarray(cam_centre, dtype=np.float64)[:, None])).sum(-1)
            n = np.where((dot > 0)[..., None], -n, n)
    valid = None
    if flags is not None:
        ok = (np.asarray(flags) == need).all(-1)
        n = np.where(ok[..., None], n, 0.0)
        valid = ok.astype(np.uint8)
    return n, valid, dot


# ---- what kornia executes, in torch fp32 -----------------------------------------------------------------------------------------------
def composition(depth, invK, k=5, s=2.0):
    """(B,3,H,W) fp32 on the inputs' device: the launches behind NormalGenerator.forward."""
    d = depth
    B, _, H, W = d.shape
    if k > 1:  # gaussian_blur2d, separable: filter2d along x, then along y, each after F.pad(reflect)
        r = k // 2
        x = torch.arange(k, dtype=torch.float32, device=d.device) - r
        g = torch.exp(-x.pow(2.0) / (2 * s ** 2))
        g = g / g.sum()
        d = F.conv2d(F.pad(d, (r, r, 0, 0), mode="reflect"), g.view(1, 1, 1, k))
        d = F.conv2d(F.pad(d, (0, 0, r, r), mode="reflect"), g.view(1, 1, k, 1))
    ys, xs = torch.meshgrid(torch.arange(H, device=d.device), torch.arange(W, device=d.device), indexing="ij")
    pix = torch.stack([xs + 0.5, ys + 0.5, torch.ones_like(xs, dtype=torch.float32)], 0).reshape(1, 3, -1).float()
    pts = (d.flatten(2) * torch.matmul(invK[:, :3, :3], pix)).view(B, 3, H, W)  # BackprojectDepth
    sobel = torch.tensor(np.stack([SOBEL_X, SOBEL_Y]), dtype=torch.float32, device=d.device)[:, None]  # spatial_gradient: (2,1,3,3)
    grad = F.conv2d(F.pad(pts.reshape(B * 3, 1, H, W), (1, 1, 1, 1), mode="replicate"), sobel).view(B, 3, 2, H, W)
    return F.normalize(torch.cross(grad[:, :, 0], grad[:, :, 1], dim=1), dim=1)


def points32(depth, invK):
    """(B,3,H,W) fp32: step 2 on an UNSMOOTHED depth in torch with the kernel's expression order, every product and sum rounded on its own:
    d * ((k0 * (x + 0.5) + k1 * (y + 0.5)) + k2)."""
    B, _, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=depth.device).float() + 0.5, torch.arange(W, device=depth.device).float() + 0.5, indexing="ij")
    K = invK[:, :3, :3]
    rows = []
    for c in range(3):
        a, b = K[:, c, 0].view(B, 1, 1) * xs, K[:, c, 1].view(B, 1, 1) * ys
        rows.append(depth[:, 0] * ((a + b) + K[:, c, 2].view(B, 1, 1)))
    return torch.stack(rows, 1)


def patches_of(pts_b3hw):
    """(B,(H-2)(W-2),9,3): the 3x3 patches of the interior pixels, row-major."""
    B, _, H, W = pts_b3hw.shape
    p = pts_b3hw.permute(0, 2, 3, 1)
    nb = [p[:, i:H - 2 + i, j:W - 2 + j] for i in range(3) for j in range(3)]
    return torch.stack(nb, 3).reshape(B, (H - 2) * (W - 2), 9, 3).contiguous()


def max_err(got, ref64):
    """The metric: the largest absolute component difference (not the angle: acos near 1 turns 6e-8 into 3e-4 rad)."""
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref64).max())


def conditioning(depth, invK, k, s):
    """min |cross| / median |cross| of the field in fp64: no pixel of a test field may be ill-conditioned."""
    d = np.asarray(depth, dtype=np.float64)[:, 0]
    pts = backproject64(blur64(d, k, s), np.asarray(invK))
    rows, cols = _taps(d.shape[1], d.shape[2])
    gx = sum(SOBEL_X[i, j] * pts[:, :, rows[i]][:, :, :, cols[j]] for i in range(3) for j in range(3))
    gy = sum(SOBEL_Y[i, j] * pts[:, :, rows[i]][:, :, :, cols[j]] for i in range(3) for j in range(3))
    c = np.sqrt((np.cross(gx, gy, axis=1) ** 2).sum(1))
    return float(c.min() / np.median(c))
