"""Reference for the edge-mask and validation-loss kernels (include/idh_geometry.h, csrc/edge_mask.hip): the torch fp32
composition that the reference's get_edge_mask executes through kornia 0.6.7 (utils/generic_utils.py:286-292: kornia.filters.sobel,
torch.nanquantile, F.max_pool2d), an fp64 numpy restatement of the same contract, and both forms of the `phase != "train"` branch of
BDModel.compute_binary_losses (experiment_modules/bd_model.py:451-495).  Everything works for any B, H, W.

kornia.filters.sobel(x, normalized=True, eps=1e-6) was restated from the library's documented definition (spatial_gradient: Sobel, order 1,
normalised by 8, replicate border; magnitude sqrt(gx^2 + gy^2 + eps)); kornia is not installed, so it is not machine-checked against it.
The quantile and dilation semantics ARE pinned to the reference's own code: tests/golden/gen_golden_edge.py runs get_edge_mask and
compute_binary_losses themselves, with `sobel32` below standing in for kornia's function."""
import numpy as np
import torch
import torch.nn.functional as F

from normals_ref import SOBEL_X, SOBEL_Y, field

EPS = 1e-6
BAND = 1e-5        # |S64 - thr64| <= BAND * thr64: pixels another fp32 implementation may decide either way
BAND_CAP = 0.005   # at most this fraction of an image may lie in the band, or the input is no test of the mask


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def with_zero_patch(depth, y0=None, x0=None, size=6):
    """A copy with a size x size patch of zero depth (clipped to the image) in every image."""
    d = depth.clone()
    H, W = d.shape[-2:]
    y0 = H // 3 if y0 is None else y0
    x0 = W // 4 if x0 is None else x0
    d[..., y0:y0 + size, x0:x0 + size] = 0.0
    return d


def with_scattered_zeros(depth, fraction=0.10):
    """A copy with `fraction` of the pixels of every image at zero depth, at positions fixed by a multiplicative hash of the index."""
    d = depth.clone()
    H, W = d.shape[-2:]
    idx = np.arange(H * W, dtype=np.uint64)
    h = (idx * np.uint64(2654435761)) % np.uint64(1000)
    zero = torch.from_numpy((h < np.uint64(int(1000 * fraction))).reshape(H, W))
    d[..., zero] = 0.0
    return d


def loss_inputs(B=2, D=3, h=24, w=32):
    """pred (B,D,h,w) logits in about [-6, 6], rendered (B,D,h,w) planes around 2, 3, 4 .. with a strip of non-positive values, depth
    (B,1,h,w) = the field with a zero patch: closed forms of the index, so that a golden need not store them."""
    i = np.arange(B * D * h * w, dtype=np.float64).reshape(B, D, h, w)
    pred = 6.0 * np.sin(0.37 * i + 0.001 * (i % 97) ** 2)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    rendered = np.stack([np.stack([2.0 + p + 0.4 * np.sin(0.3 * x + b) + 0.3 * np.cos(0.2 * y * (p + 1)) for p in range(D)]) for b in range(B)])
    rendered[:, :, :, :2] = 0.0
    rendered[:, 0, 1, :] = -1.0
    depth = with_zero_patch(field(B, h, w))
    return torch.from_numpy(pred.astype(np.float32)), torch.from_numpy(rendered.astype(np.float32)), depth


# ---- what the reference executes, in torch fp32 ----------------------------------------------------------------------------------------
def sobel32(x):
    """kornia.filters.sobel(x) for (B,C,H,W): F.pad(replicate) + the normalised Sobel pair as one convolution + the magnitude."""
    B, C, H, W = x.shape
    k = torch.tensor(np.stack([SOBEL_X, SOBEL_Y]), dtype=torch.float32, device=x.device)[:, None]
    g = F.conv2d(F.pad(x.reshape(B * C, 1, H, W), (1, 1, 1, 1), mode="replicate"), k).view(B, C, 2, H, W)
    gx, gy = g[:, :, 0], g[:, :, 1]
    return torch.sqrt(gx * gx + gy * gy + EPS)


def composition(depth_b1hw, q=0.95, dilate=True):
    """get_edge_mask as written (utils/generic_utils.py:286-292) on `sobel32`: (mask (B,1,H,W) float, S, thresholds (B,))."""
    S = sobel32(1 / depth_b1hw).float()
    thr = torch.nanquantile(S.flatten(1), q, 1)
    mask = (S > thr.reshape(-1, 1, 1, 1)).float()
    if dilate:
        mask = F.max_pool2d(mask, 5, 1, 2)
    return mask, S, thr


def losses32(pred, rendered, depth, edge_mask, reg_weight, positive_weight=1.0):
    """bd_model.py:451-495 with phase != "train", as written: (binary_loss/0, reg_loss/0, total) as 0-d fp32 tensors, or (None, None, 0)
    for an empty mask."""
    bce = torch.nn.BCEWithLogitsLoss(reduction="none", pos_weight=torch.tensor((positive_weight,)).float().to(pred.device))
    target = (rendered < depth).float()
    mask = (depth > 0) * (rendered > 0)
    if not mask.sum():
        return None, None, torch.abs(pred - pred).mean()
    binary_loss = bce(pred[mask], target[mask]).mean()
    reg_mask = (edge_mask * mask).bool() if edge_mask is not None else mask
    reg_loss = (2 * (0.5 - torch.abs(torch.sigmoid(pred[reg_mask]) - 0.5))).mean()
    total = 0.0 + binary_loss
    if reg_weight > 0.0:
        total = total + reg_loss * reg_weight
    return binary_loss, reg_loss, total


# ---- the contract in fp64 --------------------------------------------------------------------------------------------------------------
def sobel64(depth_b1hw):
    """(B,1,H,W) -> S (B,1,H,W) fp64: every tap multiplied, the zero ones too (0 * inf = NaN)."""
    d = np.asarray(depth_b1hw, dtype=np.float64)
    H, W = d.shape[-2:]
    with np.errstate(all="ignore"):
        x = 1.0 / d
        rows = [np.clip(np.arange(H) + t - 1, 0, H - 1) for t in range(3)]
        cols = [np.clip(np.arange(W) + t - 1, 0, W - 1) for t in range(3)]
        gx, gy = np.zeros_like(x), np.zeros_like(x)
        for i in range(3):
            for j in range(3):
                nb = x[..., rows[i], :][..., cols[j]]
                gx, gy = gx + SOBEL_X[i, j] * nb, gy + SOBEL_Y[i, j] * nb
        return np.sqrt(gx * gx + gy * gy + EPS)


def order_statistics(values, q):
    """torch.nanquantile's choice for one image: (n, k_lo, k_hi, weight, v_lo, v_hi) with the rank formed in fp32 as torch forms it;
    v_lo = v_hi = NaN when n == 0."""
    v = np.asarray(values).reshape(-1)
    v = np.sort(v[~np.isnan(v)])
    n = v.size
    rank = np.float32(q) * np.float32(n - 1)
    rank = np.float32(0.0) if rank < 0 else rank
    lo, hi = int(rank), int(np.ceil(rank))
    if n == 0:
        return 0, 0, 0, 0.0, float("nan"), float("nan")
    return n, lo, hi, float(rank - np.float32(lo)), v[lo], v[hi]


def lerp(a, b, w):
    """at::lerp."""
    with np.errstate(all="ignore"):
        diff = b - a
        return a + w * diff if w < 0.5 else b - diff * (1.0 - w)


def quantile64(S, q):
    """(B,...) -> (B,) fp64 thresholds."""
    out = []
    for s in np.asarray(S, dtype=np.float64):
        _, _, _, w, a, b = order_statistics(s, q)
        out.append(lerp(np.float64(a), np.float64(b), w))
    return np.array(out)


def mask64(depth_b1hw, q=0.95, S=None):
    """The undilated mask of the fp64 contract, S64 (computed here unless given), thr64 and the band |S64 - thr64| <= BAND * thr64."""
    S = sobel64(depth_b1hw) if S is None else S
    thr = quantile64(S, q)
    t = thr.reshape(-1, 1, 1, 1)
    with np.errstate(all="ignore"):
        mask = S > t
        band = np.abs(S - t) <= BAND * t
    return mask, S, thr, band


def dilate(mask):
    """5x5, stride 1, padding 2 max-pool of a (B,1,H,W) 0/1 array as an OR over the in-image window."""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape[-2:]
    p = np.zeros(m.shape[:-2] + (H + 4, W + 4), dtype=bool)
    p[..., 2:H + 2, 2:W + 2] = m
    out = np.zeros_like(m)
    for dy in range(5):
        for dx in range(5):
            out |= p[..., dy:dy + H, dx:dx + W]
    return out


def losses64(pred, rendered, depth, edge_mask, reg_weight, positive_weight=1.0):
    """The same branch in fp64: (count mask, count reg_mask, binary_loss/0, reg_loss/0, total); NaN means where a mask is empty, total 0
    for an empty mask."""
    x, r, d = (np.asarray(t, dtype=np.float64) for t in (pred, rendered, depth))
    d = np.broadcast_to(d, x.shape)
    m = (d > 0) & (r > 0)
    rm = m & (np.broadcast_to(np.asarray(edge_mask), x.shape) != 0) if edge_mask is not None else m
    t = (r < d).astype(np.float64)
    soft = np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0.0)
    bce = (1 - t) * x + (1 + (positive_weight - 1) * t) * soft
    sig = np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))
    reg = 2 * (0.5 - np.abs(sig - 0.5))
    with np.errstate(all="ignore"):
        bl = bce[m].sum() / m.sum() if m.sum() else float("nan")
        rl = reg[rm].sum() / rm.sum() if rm.sum() else float("nan")
    total = 0.0
    if m.sum():
        total = bl + (rl * reg_weight if reg_weight > 0 else 0.0)
    return int(m.sum()), int(rm.sum()), bl, rl, total
