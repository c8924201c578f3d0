"""fp64 restatement, case tables and derived bounds of the sparse occlusion queries (csrc/mlp_rays.hip, include/idh.h).

``idh_binary_mlp_rays_fwd`` is the fused form of one scale of ``BDModel.run_mlp_train`` (reference experiment_modules/bd_model.py:313-393):
rays in pixel-centre units of a grid -> ``(x / grid_w - 0.5) * 2`` -> ``F.grid_sample(bilinear, zeros, align_corners=False)`` of that scale's
feature map -> ``[depth | feature | (prior)]`` rows -> ``BinaryMLPNetwork``.  ``reference`` states that in float64 with torch's own
``grid_sample`` and ``nn.Sequential``; ``ray_bound`` is the elementwise bound the GPU result is held to.  Hostile buffers, ``PREFILL``
outputs and the layer terms of the bound are those of tests/mlp_op_ref.py.

Derivation of the feature-input error e_f (u = 2^-24; every fp32 operation returns its exact result times (1 + d), |d| <= u)
---------------------------------------------------------------------------------------------------------------------------
The kernel's coordinate chain (include/idh.h), per axis, with a = x / grid_w exactly and the exact ix* = a W - 0.5:
    t1 = fl(x / grid_w)      |t1 - a| <= u |t1|                           reaches ix with the factor d ix / d t1 = W
    t2 = fl(t1 - 0.5)        rounding <= u |t2|                           factor W
    g  = t2 * 2              exact
    t3 = fl(g + 1)           rounding <= u |t3|                           factor W / 2
    t4 = fl(t3 * W)          rounding <= u |t4|                           factor 1 / 2
    t5 = fl(t4 - 1)          rounding <= u |t5|                           factor 1 / 2
    ix = t5 * 0.5            exact
so  e_ix = u (W |t1| + W |t2| + W/2 |t3| + 1/2 |t4| + 1/2 |t5|), evaluated per ray with the float64 magnitudes of t1 .. t5 (``coord_error``;
at most u (W (5 |a| + 3.5) + 0.5)).  The fp64 reference takes the same fp32 rays and its own roundings (2^-53) are ignored.
Bilinear interpolation with zero padding is continuous and, inside a cell, linear in ix with a slope that is a convex combination of the
cell's two horizontal corner differences; so moving the sample from ix* to the kernel's ix changes channel c by at most Dx_c e_ix, Dx_c the
largest |F[y][x+1][c] - F[y][x][c]| over the corner pairs of every cell within e_ix of ix* (at most two per axis; outside the map F = 0) -
a ray ON a cell boundary is covered by taking both cells, not skipped.  The same in y, after the move in x: Dy_c e_iy.
At the kernel's own ix, iy the weights are wx0 = fl((x0 + 1) - ix), wx1 = fl(ix - x0) (x0 + 1 is exact), w = fl(wx wy): three roundings,
each relative to its result, so w_hat = w (1 + d)^3; the product fl(F w_hat) is a fourth; the sum of the (at most four) products is
accumulated in the order nw, ne, sw, se starting from 0: at most three more roundings of partial sums that are bounded by sum w |F|.
Written in the accumulation form of mlp_op_ref.logit_bound, 2 (K + c) u S with K = 4 roundings per product, c = ACC_C, S = sum w |F|
(the factor 2 is kept: it also absorbs evaluating S at ix* instead of ix, a second-order difference):
    e_f[c] = 2 (4 + ACC_C) u sum_k w_k |F_k[c]| + Dx_c e_ix + Dy_c e_iy
e_f enters layer 1 as |W1f| e_f; the remaining terms are logit_bound's.
"""
import numpy as np
import torch
import torch.nn.functional as F

import mlp_op_ref as R
from oracle import networks as onet

U, ACC_C, ELU_ERR, HID, NAN, PREFILL = R.U, R.ACC_C, R.ELU_ERR, R.HID, R.NAN, R.PREFILL
OK, EINVAL, EUNSUPPORTED = R.OK, R.EINVAL, R.EUNSUPPORTED

# ray_mlp_launch (csrc/mlp_rays.hip): more than 1024 work items run on 256 workgroups x 12 waves; with S = 1 an item is a 16-ray tile,
# so B * N = 3 * 16411 = 49233 rays are 3078 tiles > 3072 waves and the persistent loop takes a second round (as mlp_op_ref.PERSISTENT_HW)
PERSISTENT_B, PERSISTENT_N = 3, 16411
LAUNCHED_WAVES = 256 * 12


class RayCase:
    """layout: "wide" (feat_cs = Cf + 12, base 16 floats in: 16-byte aligned rows, dwordx4 loads), "base1" (Cf + 4, base 1 float in:
    4-byte-only base), "odd" (Cf + 1: a row stride that is no multiple of 4).  prior: None | "tensor" | -1.0.  grid_mul: the rays' grid is
    grid_mul x the map."""

    def __init__(self, cf, B, H, W, N, S, step, prior, layout, grid_mul):
        self.cf, self.B, self.H, self.W, self.N, self.S, self.step, self.prior, self.layout, self.grid_mul = cf, B, H, W, N, S, step, prior, layout, grid_mul
        pn = "noprior" if prior is None else (prior if isinstance(prior, str) else f"const{prior:g}")
        self.name = f"rays-c{cf}-b{B}-{H}x{W}-n{N}s{S}-step{step}-{pn}-{layout}-g{grid_mul}"

    has_prior = R.LogitCase.has_prior

    @property
    def grid(self):
        return (self.H * self.grid_mul, self.W * self.grid_mul)  # (grid_h, grid_w)

    @property
    def Nq(self):
        return (self.N + self.step - 1) // self.step

    @property
    def large(self):
        return self.N > 4096


RAY_CASES = [RayCase(*a) for a in (
    (4, 1, 5, 7, 1, 1, 1, None, "wide", 1),
    (20, 3, 5, 7, 15, 3, 2, "tensor", "base1", 2),
    (64, 1, 12, 16, 16, 3, 1, -1.0, "wide", 2),
    (64, 3, 12, 16, 37, 3, 3, "tensor", "odd", 1),
    (68, 3, 5, 7, 17, 1, 4, None, "base1", 1),
    (128, 1, 12, 16, 37, 3, 2, "tensor", "wide", 2),
    (256, 3, 12, 16, 37, 1, 4, -1.0, "base1", 1),
    (256, 1, 5, 7, 17, 3, 3, None, "wide", 2),
    (20, 1, 12, 16, 37, 3, 1, None, "odd", 1),
    (64, PERSISTENT_B, 5, 7, PERSISTENT_N, 1, 1, None, "wide", 1),
)]
assert len({c.name for c in RAY_CASES}) == len(RAY_CASES)

KINDS = ("generic", "centre", "edge0", "generic", "edgeW", "band1", "generic", "far", "cell", "band2", "generic")  # 11: coprime with every ray_step


def case_rays(case):
    """(B, N, 2) fp32 rays in units of the case's grid; ray j is of kind KINDS[j % 11]:
    generic - anywhere inside the map, at least 0.05 px (map units) from every cell boundary;
    centre  - a map pixel centre: weights exactly 1, 0, 0, 0;        edge0 / edgeW - on the outer edge x = 0 / x = grid_w;
    band1   - inside the half-pixel band at the left (two corners out);  band2 - in the top-left corner's band (three corners out);
    far     - more than 1 px (map units) outside: no corner, all-zero feature;  cell - ix an exact integer (a cell boundary) inside the map."""
    g = torch.Generator().manual_seed(R._seed(case.name) ^ 0x5A5A)
    B, N, H, W, m = case.B, case.N, case.H, case.W, case.grid_mul
    r = torch.rand((B, N, 4), generator=g, dtype=torch.float64)
    px = torch.floor(r[..., 0] * (W - 1)).clamp(max=W - 2)  # a cell with all four corners inside
    py = torch.floor(r[..., 1] * (H - 1)).clamp(max=H - 2)
    fx, fy = 0.05 + 0.9 * r[..., 2], 0.05 + 0.9 * r[..., 3]
    kind = torch.arange(N) % len(KINDS)
    ix = torch.empty(B, N, dtype=torch.float64)  # map sample coordinates: pixel (i) is ix = i
    iy = torch.empty(B, N, dtype=torch.float64)
    for k, name in enumerate(KINDS):
        sel = (kind == k).expand(B, N)
        x, y = px + fx, py + fy
        if name == "centre":
            x, y = px, py
        elif name == "edge0":
            x = torch.full_like(x, -0.5)
        elif name == "edgeW":
            x = torch.full_like(x, W - 0.5)
        elif name == "band1":
            x = -0.5 + 0.45 * fx
        elif name == "band2":
            x, y = -0.5 + 0.45 * fx, -0.5 + 0.45 * fy
        elif name == "far":
            x, y = torch.where(r[..., 2] < 0.5, -1.5 - fx, W + 0.5 + fx), py + fy
        elif name == "cell":
            x = torch.where(px + 1 <= W - 2, px + 1, px)  # an interior cell boundary whose cell still has four corners inside
        ix[sel], iy[sel] = x[sel], y[sel]
    rays = torch.stack([(ix + 0.5) * m, (iy + 0.5) * m], -1)  # ix = x W / grid_w - 0.5  <=>  x = (ix + 0.5) grid_w / W
    return rays.float()


def case_inputs(case):
    """feat (B,Cf,H,W), rays (B,N,2), depths (B,N,S), prior (B,N,S) | None - CPU fp32, seeded by the case name."""
    s = R._seed(case.name)
    import implicit_depth_amd.synthetic as syn

    feat = syn.randn((case.B, case.cf, case.H, case.W), s, "feat")
    depths = 0.5 + 7.5 * torch.rand((case.B, case.N, case.S), generator=torch.Generator().manual_seed(s))
    depths.view(-1)[-1] = 80.0
    depths.view(-1)[0] = 0.0
    prior = torch.tanh(syn.randn((case.B, case.N, case.S), s, "prior")) if case.prior == "tensor" else None
    return feat, case_rays(case), depths, prior


# ------------------------------------------------------------------------------------------------------------------
# fp64 restatement
# ------------------------------------------------------------------------------------------------------------------
def sample64(feat, rays, grid, align_corners=False, mode="bilinear"):
    """F.grid_sample in float64, the rays normalised as bd_model.py:325-326: (B, C, N)."""
    gh, gw = grid
    r = rays.double()
    g = torch.stack([(r[..., 0] / gw - 0.5) * 2, (r[..., 1] / gh - 0.5) * 2], -1).unsqueeze(2)  # B, N, 1, 2
    return F.grid_sample(feat.double(), g, mode=mode, padding_mode="zeros", align_corners=align_corners).squeeze(-1)


def mlp64(w, x, scale=0):
    """The scale's nn.Sequential (Linear, ELU, Linear, ELU, Linear) in float64 on rows x (..., Cin)."""
    k = f"mlps.s{scale}."
    h = onet.elu(x @ w[k + "0.weight"].t() + w[k + "0.bias"])
    h = onet.elu(h @ w[k + "2.weight"].t() + w[k + "2.bias"])
    return (h @ w[k + "4.weight"].t() + w[k + "4.bias"])[..., 0]


def reference(w, feat, rays, depths, prior, grid, step=1, scale=0, **sample_kw):
    """(B, Nq, S) fp64: one scale of run_mlp_train.  prior: None | float | (B,N,S)."""
    r, d = rays[:, ::step], depths[:, ::step].double()
    f = sample64(feat, r, grid, **sample_kw).permute(0, 2, 1)  # B, Nq, C
    cols = [d.unsqueeze(-1), f.unsqueeze(2).expand(-1, -1, d.shape[2], -1)]
    if prior is not None:
        p = prior[:, ::step].double() if isinstance(prior, torch.Tensor) else torch.full_like(d, float(np.float32(prior)))
        cols.append(p.unsqueeze(-1))
    return mlp64(w, torch.cat(cols, -1), scale)


# ------------------------------------------------------------------------------------------------------------------
# the derived bound
# ------------------------------------------------------------------------------------------------------------------
def coord_error(x, gsize, size):
    """(ix*, e_ix) of the module docstring for fp32 coordinates x (float64 tensor), grid size gsize, map size `size`."""
    t1 = x / gsize
    t2 = t1 - 0.5
    t3 = 2 * t2 + 1
    t4 = t3 * size
    t5 = t4 - 1
    e = U * (size * t1.abs() + size * t2.abs() + 0.5 * size * t3.abs() + 0.5 * t4.abs() + 0.5 * t5.abs())
    return t5 * 0.5, e


def feature_error(feat, rays, grid):
    """(f (B,Nq,C) fp64 sampled features, e_f (B,Nq,C)) for rays (B,Nq,2)."""
    B, C, H, W = feat.shape
    gh, gw = grid
    f64 = feat.double()
    ix, e_ix = coord_error(rays[..., 0].double(), gw, W)
    iy, e_iy = coord_error(rays[..., 1].double(), gh, H)
    f = sample64(feat, rays, grid).permute(0, 2, 1)
    S = sample64(feat.abs(), rays, grid).permute(0, 2, 1)  # sum w |F|
    pad = F.pad(f64, (2, 2, 2, 2))  # F = 0 outside; cell index c in [-2, size] -> padded index c + 2
    dxm = (pad[..., :, 1:] - pad[..., :, :-1]).abs()  # [y][x]: |F[y][x+1] - F[y][x]|, padded coordinates
    dym = (pad[..., 1:, :] - pad[..., :-1, :]).abs()
    bi = torch.arange(B).view(B, 1)
    Dx = torch.zeros_like(f)
    Dy = torch.zeros_like(f)
    cxs = [torch.floor(ix - e_ix).clamp(-2, W).long() + 2, torch.floor(ix + e_ix).clamp(-2, W).long() + 2]
    cys = [torch.floor(iy - e_iy).clamp(-2, H).long() + 2, torch.floor(iy + e_iy).clamp(-2, H).long() + 2]
    for cx in cxs:
        for cy in cys:
            for dy in (0, 1):  # the cell's two horizontal corner pairs (rows cy, cy + 1) ...
                Dx = torch.maximum(Dx, dxm[bi, :, cy + dy, cx])
            for dx in (0, 1):  # ... and its two vertical ones
                Dy = torch.maximum(Dy, dym[bi, :, cy, cx + dx])
    e_f = 2 * (4 + ACC_C) * U * S + Dx * e_ix.unsqueeze(-1) + Dy * e_iy.unsqueeze(-1)
    return f, e_f


def ray_bound(w, feat, rays, depths, prior, grid, step=1, scale=0, elu=onet.elu):
    """(fp64 logits, elementwise bound), both (B, Nq, S): mlp_op_ref.logit_bound's fp32 terms with e_f entering layer 1 as |W1f| e_f."""
    c = ACC_C
    acc = lambda K, S: 2 * (K + c) * U * S
    k = f"mlps.s{scale}."
    W1, b1, W2, b2, W3, b3 = (w[k + n] for n in ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"))
    cf = feat.shape[1]
    f, e_f = feature_error(feat, rays[:, ::step], grid)  # B, Nq, C
    d = depths[:, ::step].double().unsqueeze(-1)  # B, Nq, S, 1
    W1f, wd = W1[:, 1:1 + cf], W1[:, 0]
    pre = (f @ W1f.t() + b1).unsqueeze(2)  # B, Nq, 1, 128
    Spre = ((f.abs() + e_f) @ W1f.abs().t() + b1.abs()).unsqueeze(2)
    e_in = (e_f @ W1f.abs().t()).unsqueeze(2)
    a1 = pre + d * wd
    S1 = Spre + d.abs() * wd.abs()
    if prior is not None:
        p = (prior[:, ::step].double() if isinstance(prior, torch.Tensor) else torch.full_like(d[..., 0], float(np.float32(prior)))).unsqueeze(-1)
        wp = W1[:, 1 + cf]
        a1, S1 = a1 + p * wp, S1 + p.abs() * wp.abs()
    e_h1 = e_in + acc(cf + 3, S1) + ELU_ERR
    h1 = elu(a1)
    h1m = h1.abs() + e_h1
    a2 = h1 @ W2.t() + b2
    S2 = h1m @ W2.abs().t() + b2.abs()
    e_h2 = e_h1 @ W2.abs().t() + acc(HID, S2) + ELU_ERR
    h2 = elu(a2)
    w3 = W3[0]
    logit = h2 @ w3 + b3[0]
    S3 = (h2.abs() + e_h2) @ w3.abs() + b3[0].abs()
    tol = e_h2 @ w3.abs() + acc(HID, S3) + U * logit.abs()
    return logit, tol


def corners_in_range(case_or_shape, rays, grid):
    """(B, N) bool: all four corners of the ray's cell lie inside the map (float64 coordinates)."""
    H, W = (case_or_shape.H, case_or_shape.W) if hasattr(case_or_shape, "H") else case_or_shape
    ix = rays[..., 0].double() * W / grid[1] - 0.5
    iy = rays[..., 1].double() * H / grid[0] - 0.5
    x0, y0 = torch.floor(ix), torch.floor(iy)
    return (x0 >= 0) & (x0 <= W - 2) & (y0 >= 0) & (y0 <= H - 2)


# ------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------
LAYOUTS = {"wide": (12, 16), "base1": (4, 1), "odd": (1, 0)}  # (feat_cs - Cf, base offset in floats)


def feature_buffer(case, feat):
    """NaN-filled CPU buffer holding the map as NHWC rows of the case's layout: (flat buffer, base offset in floats, feat_cs).  Every float
    outside the Cf channels of the B H W rows is NaN: the floats before the base, channels [Cf, feat_cs) and two whole rows behind."""
    B, cf, H, W = feat.shape
    extra, off = LAYOUTS[case.layout]
    cs = cf + extra
    rows = feat.permute(0, 2, 3, 1).reshape(B * H * W, cf)
    buf = torch.full((off + (B * H * W + 2) * cs,), NAN)
    buf[off: off + B * H * W * cs].view(B * H * W, cs)[:, :cf] = rows
    return buf, off, cs


def run_rays(L, case, m, feat, rays, depths, prior, device="cuda"):
    """One launch of idh_binary_mlp_rays_fwd into a prefilled output: (rc, mlp_op_ref.Out)."""
    from implicit_depth_amd import _lib

    buf, off, cs = feature_buffer(case, feat)
    fbuf = buf.to(device)
    w1p, w2p, vecs = R.pack_net(m, case.cf, case.has_prior, False, device)
    rd, dd = rays.contiguous().to(device), depths.contiguous().to(device)
    pd = prior.contiguous().to(device) if prior is not None else None
    out = R.Out(case.B * case.Nq * case.S, device)
    gh, gw = case.grid
    rc = L.idh_binary_mlp_rays_fwd(fbuf.data_ptr() + 4 * off, cs, case.cf, case.B, case.H, case.W, rd.data_ptr(), dd.data_ptr(), _lib.ptr(pd),
                                   int(case.has_prior), float(case.prior) if isinstance(case.prior, float) else 0.0, case.N, case.S, case.step,
                                   gw, gh, w1p.data_ptr(), w2p.data_ptr(), vecs.data_ptr(), out.ptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


# ------------------------------------------------------------------------------------------------------------------
# idh_project_points_fwd
# ------------------------------------------------------------------------------------------------------------------
PROJ_B, PROJ_H, PROJ_W, PROJ_N = 3, 12, 16, 37
PROJ_MARGIN = 1e-3  # px: no point of the table lies this close to a validity or rounding boundary in float64


def projection_inputs():
    """fp32 CPU tensors: points (B,N,3), cam_T_world, K, prior_pred (B,1,H,W), prior_cam_T_world, prior_K, built by back-projecting chosen
    (u, v, z) in float64 through the first camera: interior points, points outside the image on every side, points on the image edge
    (u = 0, v = 0 within fp32 rounding is avoided: the edge points sit 0.01 px inside / outside), z < 0."""
    import implicit_depth_amd.synthetic as syn

    B, H, W, N = PROJ_B, PROJ_H, PROJ_W, PROJ_N
    g = torch.Generator().manual_seed(R._seed("project-points"))
    r = torch.rand((B, N, 3), generator=g, dtype=torch.float64)
    u = 0.3 + r[..., 0] * (W - 0.6)
    v = 0.3 + r[..., 1] * (H - 0.6)
    z = 0.8 + 4 * r[..., 2]
    j = torch.arange(N)
    u = torch.where(j % 9 == 1, -1.7 - r[..., 0], u)
    u = torch.where(j % 9 == 2, W + 0.6 + r[..., 0], u)
    v = torch.where(j % 9 == 3, -0.8 - r[..., 1], v)
    v = torch.where(j % 9 == 4, H + 2.2 + r[..., 1], v)
    u = torch.where(j % 9 == 5, torch.where(r[..., 0] < 0.5, 0.01, -0.01), u)  # on the image edge, either side
    v = torch.where(j % 9 == 6, torch.where(r[..., 1] < 0.5, H - 0.01, H + 0.01), v)
    z = torch.where(j % 9 == 7, -z, z)  # behind the camera
    Ks, cTw, pcTw = [], [], []
    for b in range(B):
        Ks.append(syn.intrinsics(W, H))
        c = syn.source_pose(b + 1)  # world_T_cam
        cTw.append(torch.linalg.inv(c))
        pcTw.append(torch.linalg.inv(c @ syn.source_pose(b + 3)))
    K, cTw, pcTw = torch.stack(Ks).double(), torch.stack(cTw).double(), torch.stack(pcTw).double()
    wTc = torch.linalg.inv(cTw)
    prior = torch.rand((B, 1, H, W), generator=g)
    for _ in range(16):  # a point that lands within the margin of a boundary (in practice: of a texel boundary of the prior view) is moved along its ray
        cam = torch.stack([(u - K[:, 0, 2, None]) / K[:, 0, 0, None] * z, (v - K[:, 1, 2, None]) / K[:, 1, 1, None] * z, z], -1)  # B, N, 3
        pts = (cam @ wTc[:, :3, :3].transpose(1, 2) + wTc[:, None, :3, 3]).float()
        ref = projection_reference(pts, cTw.float(), K.float(), H, W)
        _, sx, sy, pcz = prior_nearest_reference(pts, pcTw.float(), K.float(), prior, H, W)
        near = near_boundary_mask(ref, sx, sy, pcz, H, W, 2 * PROJ_MARGIN)
        if not near.any():
            break
        z = torch.where(near, z * 1.0371, z)
    return pts, cTw.float(), K.float(), prior, pcTw.float(), K.float()


def projection_reference(pts, cTw, K, H, W):
    """float64 Project3D (geometry_utils.py:77-89) on the fp32 inputs, with the elementwise bound of the kernel's fp32 chain:
    P = K T by 4-term fma dots: eP = 4u |K||T|;  c = P[:3] (X, 1) by 4-term fma chains: ec = eP (|X|, 1) + 4u |P| (|X|, 1);
    z = max(c_z, 1e-5) is 1-Lipschitz: ez = ec_z (+ the rounding of 1e-5f itself, u 1e-5; that alone where c_z + ec_z < 1e-5);  u = c_x / z: eu = (ec_x + |u| ez) / (z - ez) + u |u|.
    Twice that is allowed for second-order terms.  Returns dict(rays, depth, cz, e_rays, e_depth)."""
    Kd, T, X = K.double(), cTw.double(), pts.double()
    P = (Kd @ T)[:, :3]
    eP = 4 * U * (Kd.abs() @ T.abs())[:, :3]
    Xh = torch.cat([X, torch.ones_like(X[..., :1])], -1)  # B, N, 4
    c = Xh @ P.transpose(1, 2)
    ec = Xh.abs() @ eP.transpose(1, 2) + 4 * U * (Xh.abs() @ P.abs().transpose(1, 2))
    z = c[..., 2].clamp_min(1e-5)
    ez = torch.where(c[..., 2] + ec[..., 2] < 1e-5, torch.zeros_like(z), ec[..., 2]) + U * 1e-5  # well behind the camera both sides clamp to the same 1e-5f
    den = (z - ez).clamp_min(1e-30)
    uv = c[..., :2] / z.unsqueeze(-1)
    euv = (ec[..., :2] + uv.abs() * ez.unsqueeze(-1)) / den.unsqueeze(-1) + U * uv.abs()
    return {"rays": uv, "depth": z, "cz": c[..., 2], "e_rays": 2 * euv, "e_depth": 2 * ez, "e_cz": ec[..., 2]}


def prior_nearest_reference(pts, pcTw, pK, prior, H, W):
    """float64 nearest sample of BDModel.sample_prior (bd_model.py:395-410) at the points projected into the prior camera; -1 where z <= 0 or
    outside.  Returns (values (B,N), sx, sy, cz): sx = u - 0.5 the un-normalised sample coordinate."""
    ref = projection_reference(pts, pcTw, pK, H, W)
    sx, sy = ref["rays"][..., 0] - 0.5, ref["rays"][..., 1] - 0.5
    xr, yr = torch.round(sx), torch.round(sy)  # no ties in the table (PROJ_MARGIN)
    ok = (ref["cz"] > 0) & (xr >= 0) & (xr <= W - 1) & (yr >= 0) & (yr <= H - 1)
    bi = torch.arange(pts.shape[0]).view(-1, 1)
    val = prior.double()[bi, 0, yr.clamp(0, H - 1).long(), xr.clamp(0, W - 1).long()]
    return torch.where(ok, val, torch.full_like(val, -1.0)), sx, sy, ref["cz"]


def near_boundary_share(ref, psx, psy, pcz, H, W, margin=PROJ_MARGIN):
    """Share of points within `margin` of a boundary: the table is built so that this is 0."""
    return near_boundary_mask(ref, psx, psy, pcz, H, W, margin).double().mean().item()


def near_boundary_mask(ref, psx, psy, pcz, H, W, margin=PROJ_MARGIN):
    """Points within `margin` of a boundary that decides `valid` (u = 0, u = W, v = 0, v = H, z = 0) or the prior's texel
    (sx = k + 0.5, prior z = 0)."""
    u, v = ref["rays"][..., 0], ref["rays"][..., 1]
    inz = ref["cz"] > 0
    near = (ref["cz"].abs() < margin) | (inz & ((u.abs() < margin) | ((u - W).abs() < margin) | (v.abs() < margin) | ((v - H).abs() < margin)))
    tie = lambda s: ((s - 0.5) - torch.round(s - 0.5)).abs() < margin
    near |= (pcz.abs() < margin) | ((pcz > 0) & (tie(psx) | tie(psy)))
    return near


# ------------------------------------------------------------------------------------------------------------------
# the golden of BDModel.run_mlp_train (tests/golden/ray_query.npz, written by tests/golden/gen_golden_rays.py)
# ------------------------------------------------------------------------------------------------------------------
GOLDEN_SEED, GOLDEN_B, GOLDEN_N, GOLDEN_S, GOLDEN_GRID, GOLDEN_S0 = 4120, 2, 37, 3, (16, 16), 8
GOLDEN_CHANNELS = [64, 64, 128, 256]


def golden_inputs():
    """What the generator fed the reference, from synthetic.py seeds: feature maps {s: (2, C_s, 8 >> s, 8 >> s)}, rays (2,37,2) in units of
    the 16 x 16 grid reaching 2 px outside on every side, depths (2,37,3).  The weights are golden_net()'s."""
    import implicit_depth_amd.synthetic as syn

    feats = {s: syn.randn((GOLDEN_B, c, GOLDEN_S0 >> s, GOLDEN_S0 >> s), GOLDEN_SEED, f"feature_s{s}") for s, c in enumerate(GOLDEN_CHANNELS)}
    g = torch.Generator().manual_seed(GOLDEN_SEED)
    gh, gw = GOLDEN_GRID
    rays = torch.rand((GOLDEN_B, GOLDEN_N, 2), generator=g) * torch.tensor([gw + 4.0, gh + 4.0]) - 2.0
    depths = 0.5 + 7.5 * torch.rand((GOLDEN_B, GOLDEN_N, GOLDEN_S), generator=g)
    return feats, rays, depths


def golden_net(cls=None):
    """BinaryMLPNetwork([64, 64, 128, 256]) filled by synthetic.fill_state_dict; cls: the reference's class in the generator."""
    import implicit_depth_amd.synthetic as syn

    if cls is None:
        from implicit_depth_amd import networks as net

        cls = net.BinaryMLPNetwork
    m = cls(GOLDEN_CHANNELS, mlp_size=HID, use_prior=False)
    syn.fill_state_dict(m, seed=GOLDEN_SEED, gain=1.2)
    return m
