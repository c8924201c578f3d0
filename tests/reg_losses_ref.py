"""Reference for DepthModel's validation losses (include/idh_geometry.h: idh_reg_val_losses_fwd, csrc/reg_losses.hip):
closed-form inputs, the torch fp32 composition that the reference's ``DepthModel.compute_losses`` executes
(experiment_modules/depth_model.py:472-540 with losses.py:77-140 and :143-261), and an fp64 numpy restatement of the contract that also
returns the element counts behind every mean.  Everything works for any B, h, w.

``kornia.filters.blur_pool2d(x, 3)`` and ``kornia.filters.spatial_gradient(x)`` were restated from the documented definition of kornia
0.6.7 (blur_pool2d: the 3x3 binomial kernel / 16 as a per-channel convolution with zero padding 1 and stride 2; spatial_gradient: Sobel,
order 1, normalised by 8, replicate border); kornia is not installed, so neither form here is machine-checked against it.  Everything
else IS pinned to the reference's own code: tests/golden/gen_golden_reg_losses.py runs ``DepthModel.compute_losses`` itself with the two
restatements below standing in for kornia's functions.

A NaN anywhere in the ground truth reaches, through three levels of a 3x3 blur at stride 2 and a 3x3 Sobel, level-3 gradients 31 pixels
away: ``inputs`` keeps the NaNs in the left quarter of the image so that every level has finite gradients to average."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import mv_consistency_ref as MV
import normals_ref as NR
from normals_ref import SOBEL_X, SOBEL_Y, field

KEYS = ("loss", "si_loss", "grad_loss", "abs_loss", "normals_loss", "ms_loss", "inv_abs_loss", "log_l1_loss", "mv_loss")
COUNT_KEYS = ("grad_s0", "grad_s1", "grad_s2", "grad_s3", "mask_b", "mask_b_limit", "normals")
BLUR = np.outer([1.0, 2.0, 1.0], [1.0, 2.0, 1.0]) / 16.0
STRIP = 0.05  # the predicted depth of the strip that `pred > 0.1` leaves out


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _hashed(h, w, fraction, mult):
    """(h,w) bool: `fraction` of the pixels, at positions fixed by a multiplicative hash of the index."""
    idx = np.arange(h * w, dtype=np.uint64)
    return ((idx * np.uint64(mult)) % np.uint64(1000) < np.uint64(int(1000 * fraction))).reshape(h, w)


def pyramid_sizes(h, w, n=4):
    out = [(h, w)]
    for _ in range(n - 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


@functools.lru_cache(maxsize=None)
def _inputs(B, h, w, K, sizes, settle):
    r = np.random.default_rng(1000 * h + w)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    clean = field(B, h, w).double().numpy()  # (B,1,h,w)
    pred = clean * (1 + 0.1 * np.sin(0.7 * x + 0.45 * y + np.arange(B).reshape(B, 1, 1, 1)))
    pred[..., -2:] = STRIP
    # cameras and source depths: the helpers of the multi-view fixtures; the sources see a smooth surface between 1.5 and 4.5
    invK, E, sK, sE, sd = [], [], [], [], []
    for b in range(B):
        Kc, T = MV._camera(r, h, w, 0.4)
        invK.append(np.linalg.inv(Kc)), E.append(T)
        cams = [MV._camera(r, h, w, 1.0) for _ in range(K)]
        sK.append(np.stack([c[0] for c in cams])), sE.append(np.stack([np.linalg.inv(c[1]) for c in cams]))
        sd.append(np.stack([3.0 + 1.5 * np.sin(0.23 * x + 0.31 * y + b + 2 * k) for k in range(K)])[:, None])
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    invK, E, sK, sE, sd = f32(np.stack(invK)), f32(np.stack(E)), f32(np.stack(sK)), f32(np.stack(sE)), f32(np.stack(sd))
    sd[:, :, 0, :, 0] = 0.0  # a column of holes in every source
    gt, pred = f32(clean), f32(pred)
    # no projection within rounding of a tap border, no gate comparison within rounding of its threshold: nudge such pixels (both maps)
    for step in range(16 if settle else 0):
        amb = MV.check(pred, invK, E, sd, sK, sE, gate_depth=gt)["ambiguous_pixel"]
        if not amb.any():
            break
        nudge = np.float32(1 + 0.0017 * (step + 1))
        gt[:, 0], pred[:, 0] = np.where(amb, gt[:, 0] * nudge, gt[:, 0]), np.where(amb & (pred[:, 0] != np.float32(STRIP)), pred[:, 0] * nudge, pred[:, 0])
    clean32 = gt.copy()
    nan = _hashed(h, w, 0.10, 2654435761) & (x < w // 4)
    nan[h // 3:h // 3 + 4, 1:5] = True
    gt[..., nan] = np.nan
    mask_b = np.isfinite(gt) & ~_hashed(h, w, 0.05, 40503)[None, None]
    outputs = {"depth_pred_s0_b1hw": pred}
    for i, (hi, wi) in enumerate(sizes):
        if hi is None:
            continue
        yi, xi = np.meshgrid(np.arange(hi, dtype=np.float64), np.arange(wi, dtype=np.float64), indexing="ij")
        base = np.log(clean32.astype(np.float64)) if (hi, wi) == (h, w) else np.log(field(B, hi, wi).double().numpy())
        outputs[f"log_depth_pred_s{i}_b1hw"] = f32(base + 0.04 * (i + 2) * np.cos(0.21 * xi * (i + 1) + 0.17 * yi + i))
    n_gt = NR.dense(gt, invK)[0]
    n_pred = NR.dense(pred, invK)[0]
    n_pred[:, 1][np.broadcast_to(_hashed(h, w, 0.03, 69069), (B, h, w))] = np.nan
    outputs["normals_pred_b3hw"] = f32(n_pred)
    cur = {"depth_b1hw": gt, "mask_b_b1hw": mask_b, "mask_b1hw": mask_b.astype(np.float32), "normals_b3hw": f32(n_gt), "invK_s0_b44": invK,
           "world_T_cam_b44": E}
    src = {"depth_b1hw": sd, "K_s0_b44": sK, "cam_T_world_b44": sE}
    return cur, src, outputs


def inputs(B=2, h=24, w=32, K=2, sizes=None, scales=(0, 1, 2, 3), settle=True):
    """(cur_data, src_data, outputs) of ``compute_losses`` as CPU tensors, closed forms of the indices (a golden need not store them).
    gt: ``normals_ref.field`` with a NaN patch and hash-scattered NaNs in its left quarter; pred: gt (1 + 0.1 sin(..)) with a strip of
    0.05 on the right; mask_b: finite gt minus a hashed 5 %; the log-depth scales (``sizes[i]``: default h, w halved i times, which must
    divide h, w) each a closed form of its own; normals: ``normals_ref.dense`` of the two depths, 3 % of pred's pixels NaN in one channel
    on top of the footprints of gt's NaNs; K source views whose projections the fixture keeps off the tap borders (``settle=False``
    skips that: for timing at sizes where the fp64 check is slow)."""
    sizes = tuple(sizes) if sizes is not None else tuple((h >> i, w >> i) for i in range(4))
    sizes = tuple(s if i in scales else (None, None) for i, s in enumerate(sizes))
    cur, src, outputs = _inputs(B, h, w, K, sizes, settle)
    t = lambda d: {k: torch.from_numpy(v.copy()) for k, v in d.items()}
    return t(cur), t(src), t(outputs)


# ---- what the reference executes, in torch fp32 ----------------------------------------------------------------------------------------
def blur_pool32(x, kernel_size=3, stride=2):
    """kornia.filters.blur_pool2d(x, 3) for (B,C,H,W)."""
    assert kernel_size == 3 and stride == 2
    C = x.shape[1]
    k = torch.tensor(BLUR, dtype=x.dtype, device=x.device).expand(C, 1, 3, 3).contiguous()
    return F.conv2d(x, k, padding=1, stride=2, groups=C)


def spatial_gradient32(x):
    """kornia.filters.spatial_gradient(x) for (B,C,H,W): (B,C,2,H,W)."""
    B, C, H, W = x.shape
    k = torch.tensor(np.stack([SOBEL_X, SOBEL_Y]), dtype=x.dtype, device=x.device)[:, None]
    return F.conv2d(F.pad(x.reshape(B * C, 1, H, W), (1, 1, 1, 1), mode="replicate"), k).view(B, C, 2, H, W)


def grad_loss32(depth_gt, depth_pred, num_scales=4):
    """MSGradientLoss.forward (losses.py:83-101)."""
    pyr_p, pyr_g = [depth_pred], [depth_gt]
    for _ in range(num_scales - 1):
        pyr_p.append(blur_pool32(pyr_p[-1])), pyr_g.append(blur_pool32(pyr_g[-1]))
    total = torch.tensor(0, dtype=depth_gt.dtype, device=depth_gt.device)
    for p, g in zip(pyr_p, pyr_g):
        gg = spatial_gradient32(g)
        m = gg.isfinite().all(dim=1, keepdim=True)
        total += torch.mean(torch.abs(spatial_gradient32(p).masked_select(m) - gg.masked_select(m)))
    return total


def normals_loss32(n_gt, n_pred):
    """NormalsLoss.forward (losses.py:120-140)."""
    m = torch.logical_and(n_gt.isfinite().all(dim=1, keepdim=True), n_pred.isfinite().all(dim=1, keepdim=True))
    p, g = n_pred.masked_fill(~m, 1.0), n_gt.masked_fill(~m, 1.0)
    return (0.5 * (1.0 - torch.einsum("bchw, bchw -> bhw", p, g)).unsqueeze(1)).masked_select(m).mean()


def mv_loss32(pred, cur, src_depth, invK, src_K, world_T_cam, src_cam_T_world):
    """MVDepthLoss.forward (losses.py:143-261) with BackprojectDepth and Project3D (utils/geometry_utils.py:55-89)."""
    B, _, h, w = cur.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=cur.device), torch.arange(w, device=cur.device), indexing="ij")
    pix = torch.stack([xs + 0.5, ys + 0.5, torch.ones_like(xs, dtype=cur.dtype)], 0).reshape(1, 3, -1).to(cur.dtype)
    one = torch.ones(B, 1, h * w, dtype=cur.dtype, device=cur.device)

    def project(depth, k):
        pts = world_T_cam @ torch.cat([depth.flatten(2) * torch.matmul(invK[:, :3, :3], pix), one], 1)
        c = (src_K[:, k] @ src_cam_T_world[:, k])[:, :3] @ pts
        z = torch.maximum(c[:, 2:], torch.full((1, 1, 1), 1e-5, dtype=cur.dtype, device=cur.device))
        return (c[:, :2] / z).view(B, 2, h, w), z.view(B, 1, h, w)

    K = src_depth.shape[1]
    total = 0
    for k in range(K):
        uv, z_gate = project(cur, k)
        grid = 2 * (uv.permute(0, 2, 3, 1) / torch.tensor([w, h]).view(1, 1, 1, 2).type_as(uv)) - 1
        s = F.grid_sample(src_depth[:, k], grid, padding_mode="zeros", mode="nearest", align_corners=False)
        valid = (z_gate < 1.05 * s) & (z_gate > 0) & (s > 0)
        z_pred = project(pred, k)[1]
        total = total + torch.abs(torch.log(s) - torch.log(z_pred)).masked_select(valid).nanmean()
    return total / K


def compute_losses32(cur_data, src_data, outputs, hypersim=False, si_lambda=0.85):
    """depth_model.py:472-540 as written, on the restatements above: the nine entries, 0-d tensors (python 0 under hypersim)."""
    gt, mask_b, pred, log_pred = cur_data["depth_b1hw"], cur_data["mask_b_b1hw"], outputs["depth_pred_s0_b1hw"], outputs["log_depth_pred_s0_b1hw"]
    l1 = torch.nn.L1Loss()
    log_gt = torch.log(gt)
    found, ms = False, 0
    for i in range(4):
        if f"log_depth_pred_s{i}_b1hw" in outputs:
            resized = F.interpolate(outputs[f"log_depth_pred_s{i}_b1hw"], size=gt.shape[-2:], mode="nearest")
            ms += l1(log_gt[mask_b], resized[mask_b]) / 2 ** i
            found = True
    if not found:
        raise Exception("Could not find a valid scale to compute si loss!")
    grad = 0 if hypersim else grad_loss32(gt, pred)
    ab = l1(gt[mask_b], pred[mask_b])
    d = log_gt[mask_b] - log_pred[mask_b]
    si = torch.sqrt((d ** 2).mean() - si_lambda * (d.mean() ** 2))
    limit = torch.logical_and(mask_b, pred > 0.1)
    inv = l1(1 / gt[limit], 1 / pred[limit])
    log_l1 = l1(log_gt[mask_b], log_pred[mask_b])
    nrm = 0 if hypersim else normals_loss32(cur_data["normals_b3hw"], outputs["normals_pred_b3hw"])
    mv = 0 if hypersim else mv_loss32(pred, gt, src_data["depth_b1hw"], cur_data["invK_s0_b44"], src_data["K_s0_b44"],
                                      cur_data["world_T_cam_b44"], src_data["cam_T_world_b44"])
    loss = ms + 1.0 * grad + 1.0 * nrm + 0.2 * mv
    return dict(zip(KEYS, (loss, si, grad, ab, nrm, ms, inv, log_l1, mv)))


# ---- the contract in fp64 --------------------------------------------------------------------------------------------------------------
def blur_pool64(x):
    """(B,H,W) fp64 -> (B,ceil(H/2),ceil(W/2)): zero padding 1, stride 2."""
    B, H, W = x.shape
    p = np.zeros((B, H + 2 + H % 2, W + 2 + W % 2))
    p[:, 1:H + 1, 1:W + 1] = x
    Hn, Wn = (H + 1) // 2, (W + 1) // 2
    with np.errstate(all="ignore"):
        return sum(BLUR[i, j] * p[:, i:i + 2 * Hn:2, j:j + 2 * Wn:2] for i in range(3) for j in range(3))


def spatial_gradient64(x):
    """(B,H,W) fp64 -> (gx, gy): every tap multiplied, the zero ones too (0 * NaN = 0 * inf = NaN)."""
    rows, cols = NR._taps(x.shape[1], x.shape[2])
    gx, gy = np.zeros_like(x), np.zeros_like(x)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                nb = x[:, rows[i]][:, :, cols[j]]
                gx, gy = gx + SOBEL_X[i, j] * nb, gy + SOBEL_Y[i, j] * nb
    return gx, gy


def _mean(values, mask):
    with np.errstate(all="ignore"):
        return values[mask].sum() / mask.sum() if mask.sum() else float("nan")


def grad_levels64(depth_gt, depth_pred, num_scales=4):
    """Per level (mean |g_pred - g_gt| over the finite gt gradient components, their number)."""
    g, p = np.asarray(depth_gt, np.float64)[:, 0], np.asarray(depth_pred, np.float64)[:, 0]
    out = []
    for level in range(num_scales):
        if level:
            g, p = blur_pool64(g), blur_pool64(p)
        gg, gp = np.stack(spatial_gradient64(g)), np.stack(spatial_gradient64(p))
        m = np.isfinite(gg)
        with np.errstate(all="ignore"):
            out.append((_mean(np.abs(gp - gg), m), int(m.sum())))
    return out


def losses64(cur_data, src_data, outputs, hypersim=False, si_lambda=0.85):
    """The contract in fp64 from the fp32 inputs: (values by KEYS, counts by COUNT_KEYS).  The cocktail is formed from the nine fp64 values."""
    f = lambda t: np.asarray(t, np.float32).astype(np.float64)
    gt, pred, mask_b = f(cur_data["depth_b1hw"]), f(outputs["depth_pred_s0_b1hw"]), np.asarray(cur_data["mask_b_b1hw"]).astype(bool)
    B, _, h, w = gt.shape
    counts = dict.fromkeys(COUNT_KEYS, 0)
    with np.errstate(all="ignore"):
        log_gt = np.log(gt)
        ms = 0.0
        for i in range(4):
            if f"log_depth_pred_s{i}_b1hw" in outputs:
                lp = f(outputs[f"log_depth_pred_s{i}_b1hw"])
                ry, rx = h // lp.shape[2], w // lp.shape[3]
                assert ry * lp.shape[2] == h and rx * lp.shape[3] == w
                up = lp[:, :, np.arange(h) // ry][:, :, :, np.arange(w) // rx]
                ms += _mean(np.abs(log_gt - up), mask_b) / 2 ** i
        d = log_gt - f(outputs["log_depth_pred_s0_b1hw"])
        lam = float(np.float32(si_lambda))
        si = np.sqrt(_mean(d * d, mask_b) - lam * _mean(d, mask_b) ** 2)
        limit = mask_b & (np.asarray(outputs["depth_pred_s0_b1hw"], np.float32) > np.float32(0.1))
        v = {"ms_loss": ms, "si_loss": si, "abs_loss": _mean(np.abs(gt - pred), mask_b), "log_l1_loss": _mean(np.abs(d), mask_b),
             "inv_abs_loss": _mean(np.abs(1 / gt - 1 / pred), limit)}
        counts["mask_b"], counts["mask_b_limit"] = int(mask_b.sum()), int(limit.sum())
        if hypersim:
            v.update(grad_loss=0.0, normals_loss=0.0, mv_loss=0.0)
        else:
            levels = grad_levels64(gt, pred)
            v["grad_loss"] = sum(m for m, _ in levels)
            for i, (_, n) in enumerate(levels):
                counts[f"grad_s{i}"] = n
            ng, npd = f(cur_data["normals_b3hw"]), f(outputs["normals_pred_b3hw"])
            m = np.isfinite(ng).all(1) & np.isfinite(npd).all(1)
            counts["normals"] = int(m.sum())
            v["normals_loss"] = _mean(0.5 * (1 - (np.where(m[:, None], ng, 1.0) * np.where(m[:, None], npd, 1.0)).sum(1)), m)
            v["mv_loss"] = MV.check(outputs["depth_pred_s0_b1hw"], cur_data["invK_s0_b44"], cur_data["world_T_cam_b44"], src_data["depth_b1hw"],
                                    src_data["K_s0_b44"], src_data["cam_T_world_b44"], gate_depth=cur_data["depth_b1hw"])["loss"]
        v["loss"] = v["ms_loss"] + v["grad_loss"] + v["normals_loss"] + float(np.float32(0.2)) * v["mv_loss"]
    return {k: float(v[k]) for k in KEYS}, counts
