"""fp64 restatement, case table and derived bounds of the dense occlusion query in a moving camera (idh_binary_mlp_view_fwd, view_mlp_k in
csrc/mlp_rays.hip; include/idh.h states the fp32 expression).

Per pixel of a depth map rendered in ANY camera: ``BackprojectDepth`` (reference utils/geometry_utils.py:55-63) in that camera, its
``world_T_cam``, ``Project3D`` (:77-89) into the keyframe camera, ``F.grid_sample(bilinear, zeros, align_corners=False)`` of feature_s0 and
``BinaryMLPNetwork`` on ``[z | feature | (prior)]`` with z the point's depth in the KEYFRAME camera; the prior is the nearest sample of
``BDModel.sample_prior`` (experiment_modules/bd_model.py:405-409).  The case machinery (layouts, hostile buffers, the gather's and the MLP's
error terms) is that of tests/ray_query_ref.py and tests/mlp_op_ref.py, imported and not edited.

Derivation of the coordinate errors (u = 2^-24; an fma rounds once; a chain of k roundings of terms t_j errs by at most k u sum |t_j|)
--------------------------------------------------------------------------------------------------------------------------------------
x = col + 0.5, y = row + 0.5 are exact in fp32.
    c_i = fma(iK_i0, x, fma(iK_i1, y, iK_i2))          2 roundings      e_c = 2 u (|iK_i0| x + |iK_i1| y + |iK_i2|)
    X_i = d c_i                                        1 rounding       e_X = d e_c + u |X_i|
    p_i = fma(T_i0, X_0, fma(T_i1, X_1, fma(T_i2, X_2, T_i3)))   3 roundings, inputs off by e_X
                                                                        e_p = |T_i,:3| e_X + 3 u (|T_i,:3| |X| + |T_i3|)
The projection is ray_query_ref.projection_reference's (P = K T by 4-term fma dots: eP = 4 u |K||T|; c = P (p, 1) by 3 fmas after P's own
4: ec = eP (|p|, 1) + 4 u |P| (|p|, 1)) with the point's own error passed through: + |P_:3| e_p (and eP e_p, second order, kept).
z = max(c_z, 1e-5), (u, v) = c_xy / z and their errors e_z, e_uv exactly as there, including its factor 2 for second-order terms.
``points`` / ``depth`` are held to 2 e_p / 2 e_z.  For the logit, e_uv enters the gather's coordinate error (grid = map: d ix / d u = 1)
next to the five roundings ray_query_ref.coord_error counts, the largest corner difference of the cells in reach multiplies it, and e_z
enters layer 1 as |wd| e_z; everything else is ray_query_ref.ray_bound.

Validity (d finite and > 0, c_z > 0, 0 <= u < W, 0 <= v < H) and the prior's nearest texel are discontinuous: a pixel whose float64
projection lies within PROJ_MARGIN (ray_query_ref's 1e-3 px; 1e-3 m for c_z) of such a boundary is left out of every comparison.  The share
left out is capped at NEAR_CAP = 1 % per case; tests/test_view_query_cpu.py asserts the cap - and that the fp32 chain's own error is far
below the margin - on this float64 reference alone.
"""
import math

import numpy as np
import torch

import mlp_op_ref as R
import ray_query_ref as Q
from oracle import networks as onet

U, ACC_C, ELU_ERR, HID, NAN = R.U, R.ACC_C, R.ELU_ERR, R.HID, R.NAN
OK, EINVAL, EUNSUPPORTED = R.OK, R.EINVAL, R.EUNSUPPORTED
PROJ_MARGIN = Q.PROJ_MARGIN
NEAR_CAP = 0.01
CAMERAS = ("identity", "moved", "behind", "own")


class ViewCase:
    """A (B,P,h,w) depth map in camera ``camera`` against a (B,H,W,cf) keyframe map.  camera: "identity" - the keyframe's own pose and
    intrinsics (scaled to h x w); "moved" - translated and rotated, part of the view leaves the keyframe's image; "behind" - rotated by
    149 degrees, every point behind the keyframe camera; "own" - its own intrinsics (a wider lens, the principal point off the centre) at its own resolution, moved a little.
    prior: None | "map" (nearest sample of a (B,1,H,W) prediction in a third camera) | -1.0 (the constant).  layout: ray_query_ref.LAYOUTS."""

    def __init__(self, cf, B, H, W, P, h, w, camera, prior, layout, fill=0.0):
        assert camera in CAMERAS and layout in Q.LAYOUTS
        self.cf, self.B, self.H, self.W, self.P, self.h, self.w, self.camera, self.prior, self.layout, self.fill = cf, B, H, W, P, h, w, camera, prior, layout, fill
        pn = "noprior" if prior is None else (prior if isinstance(prior, str) else f"const{prior:g}")
        self.name = f"view-c{cf}-b{B}-{H}x{W}-p{P}-{h}x{w}-{camera}-{pn}-{layout}"

    has_prior = R.LogitCase.has_prior

    @property
    def rays(self):
        return self.B * self.P * self.h * self.w


VIEW_CASES = [ViewCase(*a) for a in (
    (64, 1, 12, 16, 1, 12, 16, "identity", None, "wide"),
    (64, 2, 12, 16, 3, 7, 9, "moved", "map", "base1", -7.5),      # 378 rays: no multiple of 16, tiles straddle planes and batches
    (64, 1, 24, 32, 1, 5, 3, "moved", -1.0, "base1", 2.25),        # 15 rays: one partial tile
    (64, 2, 12, 16, 2, 7, 9, "behind", "map", "wide", -3.0),      # every pixel invalid
    (64, 1, 24, 32, 2, 15, 20, "own", "map", "wide"),
    (64, 2, 24, 32, 1, 15, 20, "own", None, "odd", 1.0),
    (128, 2, 12, 16, 1, 7, 9, "moved", "map", "base1", -7.5),     # W1f not in LDS
    (64, 1, 12, 16, 1, 201, 245, "moved", None, "wide"),          # 49 245 rays = 3078 tiles > 256 x 12 waves: a second round
)]
assert len({c.name for c in VIEW_CASES}) == len(VIEW_CASES)
LARGE = [c for c in VIEW_CASES if c.rays > 4096]


def _rot(axis, theta):
    c, s = math.cos(theta), math.sin(theta)
    T = torch.eye(4, dtype=torch.float64)
    i, j = {"x": (1, 2), "y": (2, 0)}[axis]
    T[i, i], T[i, j], T[j, i], T[j, j] = c, -s, s, c
    return T


def relative_pose(camera, b=0):
    """key_T_view (4,4) float64: the view camera's pose in the keyframe camera's frame."""
    if camera == "identity":
        return torch.eye(4, dtype=torch.float64)
    if camera == "behind":
        T = _rot("y", math.radians(149.0) + 0.02 * b)
        T[:3, 3] = torch.tensor([0.05, 0.0, -0.1], dtype=torch.float64)
        return T
    if camera == "moved":
        T = _rot("y", 0.31 + 0.04 * b) @ _rot("x", -0.12)
        T[:3, 3] = torch.tensor([0.35 + 0.05 * b, -0.12, 0.2], dtype=torch.float64)
        return T
    T = _rot("y", -0.05 - 0.01 * b) @ _rot("x", 0.03)
    T[:3, 3] = torch.tensor([-0.08, 0.04, 0.05 * b], dtype=torch.float64)
    return T


def cameras(camera, B, H, W, h, w):
    """fp32 (B,4,4) each: view invK (at h x w), view world_T_cam, keyframe cam_T_world, keyframe K (at H x W), prior cam_T_world, prior K."""
    import implicit_depth_amd.synthetic as syn

    K = syn.intrinsics(W, H)
    Kv = syn.intrinsics(w, h)
    if camera == "own":  # a camera of its own: the 480 x 640 intrinsics at h x w with a wider lens and a principal point off the centre
        Kv = Kv.clone()
        Kv[0, 0], Kv[1, 1] = 0.8 * Kv[0, 0], 0.84 * Kv[1, 1]
        Kv[0, 2], Kv[1, 2] = Kv[0, 2] + 0.3, Kv[1, 2] - 0.2
    iK, wTc, cTw, Ks, pcTw = [], [], [], [], []
    for b in range(B):
        key = syn.source_pose(b + 1)  # the keyframe's world_T_cam
        iK.append(torch.linalg.inv(Kv))
        wTc.append(key @ relative_pose(camera, b))
        cTw.append(torch.linalg.inv(key))
        Ks.append(K)
        pcTw.append(torch.linalg.inv(key @ syn.source_pose(b + 3, big_rotation=True)))  # turned by 0.6 rad: part of the keyframe's image has no prior
    f = lambda ts: torch.stack(ts).float()
    return f(iK), f(wTc), f(cTw), f(Ks), f(pcTw), f(Ks)


def rendered_map(B, P, h, w, seed, hostile=True):
    """(B,P,h,w) fp32 depths in 1 .. 4 m with holes (0) at every 13th pixel and - ``hostile`` - a negative value, +-inf and NaN."""
    d = 1.0 + 3.0 * torch.rand((B, P, h, w), generator=torch.Generator().manual_seed(seed))
    flat = d.view(-1)
    flat[5::13] = 0.0
    if hostile:
        n = flat.numel()
        for i, v in enumerate((0.0, -1.5, float("inf"), NAN, float("-inf"))):
            flat[(i * 3) % n] = v
            if n > 64:
                flat[n - 1 - i * 2] = v
    return d


def case_inputs(case):
    """feat (B,cf,H,W), rendered (B,P,h,w), the six matrices of ``cameras``, prior map (B,1,H,W) | None - CPU fp32, seeded by the case name."""
    import implicit_depth_amd.synthetic as syn

    s = R._seed(case.name)
    feat = syn.randn((case.B, case.cf, case.H, case.W), s, "feat")
    cams = cameras(case.camera, case.B, case.H, case.W, case.h, case.w)
    prior = torch.sigmoid(syn.randn((case.B, 1, case.H, case.W), s, "prior")) if case.prior == "map" else None
    return feat, rendered_map(case.B, case.P, case.h, case.w, s), cams, prior


# ------------------------------------------------------------------------------------------------------------------
# fp64 restatement of the coordinate chain, with the fp32 chain's error bounds
# ------------------------------------------------------------------------------------------------------------------
def _project64(p, e_p, cTw, K):
    """Project3D in float64 on points (B,N,3) that carry the error e_p: ray_query_ref.projection_reference with the input error passed on."""
    Kd, T = K.double(), cTw.double()
    Pm = (Kd @ T)[:, :3]
    eP = 4 * U * (Kd.abs() @ T.abs())[:, :3]
    one = torch.ones_like(p[..., :1])
    ph, pa = torch.cat([p, one], -1), torch.cat([p.abs() + e_p, one], -1)
    c = ph @ Pm.transpose(1, 2)
    ec = pa @ eP.transpose(1, 2) + 4 * U * (ph.abs() @ Pm.abs().transpose(1, 2)) + e_p @ Pm[:, :, :3].abs().transpose(1, 2)
    z = c[..., 2].clamp_min(1e-5)
    ez = torch.where(c[..., 2] + ec[..., 2] < 1e-5, torch.zeros_like(z), ec[..., 2]) + U * 1e-5
    den = (z - ez).clamp_min(1e-30)
    uv = c[..., :2] / z.unsqueeze(-1)
    euv = (ec[..., :2] + uv.abs() * ez.unsqueeze(-1)) / den.unsqueeze(-1) + U * uv.abs()
    return {"uv": uv, "z": z, "cz": c[..., 2], "e_uv": 2 * euv, "e_z": 2 * ez, "e_cz": ec[..., 2]}


def chain64(rendered, cams, H, W, prior=None):
    """The chain up to the MLP's inputs, in float64 on the fp32 inputs, every tensor flattened to N = P h w pixels per batch element:
    dok (B,N) - the depth is finite and positive (the others are asked as d = 0); points (B,N,3) world points, uv (B,N,2), z, cz (B,N),
    valid (B,N); e_points, e_uv, e_z the fp32 chain's bounds; prior (B,N) nearest sample | None; near (B,N) - within PROJ_MARGIN of a
    boundary that decides valid or the prior's texel."""
    iK, wTc, cTw, K, pcTw, pK = (m.double() for m in cams)
    B, P, h, w = rendered.shape
    dr = rendered.double()
    dok = torch.isfinite(dr) & (dr > 0)
    d = torch.where(dok, dr, torch.zeros_like(dr)).reshape(B, P, h * w, 1)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64) + 0.5, torch.arange(w, dtype=torch.float64) + 0.5, indexing="ij")
    pix = torch.stack([xx.reshape(-1), yy.reshape(-1), torch.ones(h * w, dtype=torch.float64)], -1)  # hw, 3
    c = pix @ iK[:, :3, :3].transpose(1, 2)  # B, hw, 3
    e_c = 2 * U * (pix @ iK[:, :3, :3].abs().transpose(1, 2))
    X = d * c.unsqueeze(1)  # B, P, hw, 3
    e_X = d * e_c.unsqueeze(1) + U * X.abs()
    Rm, t = wTc[:, :3, :3], wTc[:, :3, 3]
    Ra = Rm.abs().transpose(1, 2).unsqueeze(1)
    p = X @ Rm.transpose(1, 2).unsqueeze(1) + t.view(B, 1, 1, 3)
    e_p = e_X @ Ra + 3 * U * (X.abs() @ Ra + t.abs().view(B, 1, 1, 3))
    p, e_p, dok = p.reshape(B, -1, 3), e_p.reshape(B, -1, 3), dok.reshape(B, -1)
    key = _project64(p, e_p, cTw, K)
    u, v, cz = key["uv"][..., 0], key["uv"][..., 1], key["cz"]
    valid = dok & (cz > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    m = PROJ_MARGIN
    near = dok & ((cz.abs() < m) | ((cz > 0) & ((u.abs() < m) | ((u - W).abs() < m) | (v.abs() < m) | ((v - H).abs() < m))))
    out = {"dok": dok, "points": p, "e_points": 2 * e_p, "uv": key["uv"], "z": key["z"], "cz": cz, "valid": valid, "e_uv": key["e_uv"],
           "e_z": key["e_z"], "e_cz": key["e_cz"], "prior": None}
    if prior is not None:
        pr = _project64(p, e_p, pcTw, pK)
        sx, sy, pcz = pr["uv"][..., 0] - 0.5, pr["uv"][..., 1] - 0.5, pr["cz"]
        xr, yr = torch.round(sx), torch.round(sy)  # a tie lies inside the margin and is left out
        ok = (pcz > 0) & (xr >= 0) & (xr <= W - 1) & (yr >= 0) & (yr <= H - 1)
        val = prior.double()[torch.arange(B).view(B, 1), 0, yr.clamp(0, H - 1).long(), xr.clamp(0, W - 1).long()]
        out["prior"] = torch.where(ok, val, torch.full_like(val, -1.0))
        tie = lambda s: ((s - 0.5) - torch.round(s - 0.5)).abs() < m
        near = near | (valid & ((pcz.abs() < m) | ((pcz > 0) & (tie(sx) | tie(sy)))))  # only a valid pixel reads the prior
        out.update(e_prior_uv=pr["e_uv"], e_prior_cz=pr["e_cz"], prior_cz=pcz, prior_uv=pr["uv"])
    out["near"] = near
    return out


def _prior_arg(case_prior, ch):
    return ch["prior"] if ch["prior"] is not None else (float(case_prior) if isinstance(case_prior, float) else None)


def reference(w, feat, rendered, cams, prior_map=None, prior_const=None, fill=0.0):
    """float64 restatement: (logits (B,P,h,w) with ``fill`` at the invalid pixels, chain64's dictionary).  ``prior_const``: a float for a
    prior-enabled network without a map."""
    B, _, H, W = feat.shape
    ch = chain64(rendered, cams, H, W, prior_map)
    f = Q.sample64(feat, ch["uv"], (H, W)).permute(0, 2, 1)  # B, N, C
    cols = [ch["z"].unsqueeze(-1), f]
    pv = ch["prior"] if ch["prior"] is not None else (None if prior_const is None else torch.full_like(ch["z"], float(np.float32(prior_const))))
    if pv is not None:
        cols.append(pv.unsqueeze(-1))
    logit = Q.mlp64(w, torch.cat(cols, -1))
    return torch.where(ch["valid"], logit, torch.full_like(logit, fill)).view(rendered.shape), ch


# ------------------------------------------------------------------------------------------------------------------
# the derived bound
# ------------------------------------------------------------------------------------------------------------------
def feature_error(feat, uv, e_uv):
    """ray_query_ref.feature_error at float64 sample points (B,N,2) in map pixel units that themselves carry the error e_uv (B,N,2)."""
    import torch.nn.functional as F

    B, C, H, W = feat.shape
    ix, e_ix = Q.coord_error(uv[..., 0], W, W)
    iy, e_iy = Q.coord_error(uv[..., 1], H, H)
    e_ix, e_iy = e_ix + e_uv[..., 0], e_iy + e_uv[..., 1]  # d ix / d u = W / grid_w = 1
    f = Q.sample64(feat, uv, (H, W)).permute(0, 2, 1)
    S = Q.sample64(feat.abs(), uv, (H, W)).permute(0, 2, 1)
    pad = F.pad(feat.double(), (2, 2, 2, 2))
    dxm = (pad[..., :, 1:] - pad[..., :, :-1]).abs()
    dym = (pad[..., 1:, :] - pad[..., :-1, :]).abs()
    bi = torch.arange(B).view(B, 1)
    Dx, Dy = torch.zeros_like(f), torch.zeros_like(f)
    cxs = [torch.floor(ix - e_ix).clamp(-2, W).long() + 2, torch.floor(ix + e_ix).clamp(-2, W).long() + 2]
    cys = [torch.floor(iy - e_iy).clamp(-2, H).long() + 2, torch.floor(iy + e_iy).clamp(-2, H).long() + 2]
    for cx in cxs:
        for cy in cys:
            for dy in (0, 1):
                Dx = torch.maximum(Dx, dxm[bi, :, cy + dy, cx])
            for dx in (0, 1):
                Dy = torch.maximum(Dy, dym[bi, :, cy, cx + dx])
    return f, 2 * (4 + ACC_C) * U * S + Dx * e_ix.unsqueeze(-1) + Dy * e_iy.unsqueeze(-1)


def view_bound(w, feat, ch, prior_const=None, elu=onet.elu):
    """(fp64 logits, elementwise bound), both (B,N), for every pixel as if it were valid: ray_query_ref.ray_bound's terms with the sample
    point's error e_uv inside e_f and the depth's error entering layer 1 as |wd| e_z."""
    acc = lambda K, S: 2 * (K + ACC_C) * U * S
    W1, b1, W2, b2, W3, b3 = (w["mlps.s0." + n] for n in ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"))
    cf = feat.shape[1]
    f, e_f = feature_error(feat, ch["uv"], ch["e_uv"])
    d, e_d = ch["z"].unsqueeze(-1), ch["e_z"].unsqueeze(-1)
    W1f, wd = W1[:, 1:1 + cf], W1[:, 0]
    a1 = f @ W1f.t() + b1 + d * wd
    S1 = (f.abs() + e_f) @ W1f.abs().t() + b1.abs() + (d.abs() + e_d) * wd.abs()
    e_in = e_f @ W1f.abs().t() + e_d * wd.abs()
    pv = ch["prior"] if ch["prior"] is not None else (None if prior_const is None else torch.full_like(ch["z"], float(np.float32(prior_const))))
    if pv is not None:
        wp = W1[:, 1 + cf]
        a1, S1 = a1 + pv.unsqueeze(-1) * wp, S1 + pv.abs().unsqueeze(-1) * wp.abs()
    e_h1 = e_in + acc(cf + 3, S1) + ELU_ERR
    h1 = elu(a1)
    a2 = h1 @ W2.t() + b2
    S2 = (h1.abs() + e_h1) @ W2.abs().t() + b2.abs()
    e_h2 = e_h1 @ W2.abs().t() + acc(HID, S2) + ELU_ERR
    h2 = elu(a2)
    w3 = W3[0]
    logit = h2 @ w3 + b3[0]
    S3 = (h2.abs() + e_h2) @ w3.abs() + b3[0].abs()
    return logit, e_h2 @ w3.abs() + acc(HID, S3) + U * logit.abs()


# ------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------
def run_view(L, case, m, feat, rendered, cams, prior_map, device="cuda", outputs=(True, True, True)):
    """One launch of idh_binary_mlp_view_fwd into prefilled outputs: (rc, logits Out, valid uint8 buffer with 8 guard bytes either side,
    depth Out | None, points Out | None).  ``outputs``: which of (valid, view_depth, view_points) are asked for."""
    from implicit_depth_amd import _lib

    buf, off, cs = Q.feature_buffer(case, feat)
    fbuf = buf.to(device)
    w1p, w2p, vecs = R.pack_net(m, case.cf, case.has_prior, False, device)
    rd = rendered.contiguous().to(device)
    c = [t.contiguous().to(device) for t in cams]
    pm = prior_map.contiguous().to(device) if prior_map is not None else None
    n = case.rays
    logits = R.Out(n, device)
    valid = torch.full((n + 16,), 0x5A, dtype=torch.uint8, device=device) if outputs[0] else None
    depth = R.Out(n, device) if outputs[1] else None
    points = R.Out(3 * n, device) if outputs[2] else None
    rc = L.idh_binary_mlp_view_fwd(fbuf.data_ptr() + 4 * off, cs, case.cf, case.B, case.H, case.W, rd.data_ptr(), case.P, case.h, case.w,
                                   c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), c[3].data_ptr(), _lib.ptr(pm),
                                   c[4].data_ptr() if pm is not None else None, c[5].data_ptr() if pm is not None else None, int(case.has_prior),
                                   float(case.prior) if isinstance(case.prior, float) else 0.0, w1p.data_ptr(), w2p.data_ptr(), vecs.data_ptr(),
                                   float(case.fill), logits.ptr, valid.data_ptr() + 8 if valid is not None else None,
                                   depth.ptr if depth else None, points.ptr if points else None, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, logits, valid, depth, points


# ------------------------------------------------------------------------------------------------------------------
# the golden of the reference's own modules (tests/golden/view_query.npz, written by tests/golden/gen_golden_view.py)
# ------------------------------------------------------------------------------------------------------------------
GOLDEN_CAMERAS = ("moved", "own")
GOLDEN_H, GOLDEN_W = 9, 11  # the view maps; the keyframe map is ray_query_ref.golden_inputs()'s 8 x 8 feature_s0, B = 2


def golden_inputs(camera):
    """(feature_s0 (2,64,8,8), rendered (2,1,9,11) with holes, the six matrices) of one golden camera; the net is ray_query_ref.golden_net()."""
    feats, _, _ = Q.golden_inputs()
    S = Q.GOLDEN_S0
    rendered = rendered_map(Q.GOLDEN_B, 1, GOLDEN_H, GOLDEN_W, Q.GOLDEN_SEED + CAMERAS.index(camera), hostile=False)
    return feats[0], rendered, cameras(camera, Q.GOLDEN_B, S, S, GOLDEN_H, GOLDEN_W)
