"""Case table, inputs, fp64 simulation and device call of the ray depth search (idh_binary_mlp_rays_search_fwd, csrc/mlp_rays.hip).

The search is the rule of mlp_op_ref (``first_query``, ``thresholds_at``, ``search_step``) on the rays, features and derived bound of
ray_query_ref (``case_rays``, ``reference``, ``ray_bound``): both are imported as they are.  A ``SearchRayCase`` carries the attributes
both expect (an S = 1, ray_step = 1 RayCase that is also a SearchCase).

Hit points (include/idh.h), u = 2^-24, an fma chain of n operations errs by at most n u times the sum of the magnitudes of its terms:
    c_i = fma(iK[4i], x, fma(iK[4i+1], y, iK[4i+2]))     two fmas:       e_c = 2 u (|iK0 x| + |iK1 y| + |iK2|)
    X_i = d * c_i                                        one more:       e_X = |d| e_c + u |d c_i|      <= 3 u |d| sum|terms of c_i|
    p_i = fma(T0, X0, fma(T1, X1, fma(T2, X2, T3)))      three fmas:     e_p = sum_j |T_ij| e_Xj + 3 u (sum_j |T_ij| |X_j| + |T_i3|)
evaluated in float64 at the kernel's own depth d, at the fp32 rays and matrices (``points_reference``).
"""
import numpy as np
import torch

import implicit_depth_amd.synthetic as syn
import mlp_op_ref as R
import ray_query_ref as Q

U = R.U
ITERS = R.SEARCH_ITERS
FAR = -1.0e4  # stands in for a non-finite ray in the fp64 reference: more than a pixel outside, no corner, f = 0


class SearchRayCase:
    """prior: None | "tensor" ((B,N)) | a float constant; thr: a constant threshold or a key of mlp_op_ref.TABLES; nonfinite: overwrite
    ray (0, 5) with NaN and ray (B - 1, 7) with +inf."""

    S, step = 1, 1

    def __init__(self, cf, B, H, W, N, prior, layout, grid_mul, thr, lo, hi, nonfinite=False):
        self.cf, self.B, self.H, self.W, self.N, self.prior, self.layout, self.grid_mul = cf, B, H, W, N, prior, layout, grid_mul
        self.thr, self.lo, self.hi, self.nonfinite = thr, lo, hi, nonfinite
        pn = "noprior" if prior is None else (prior if isinstance(prior, str) else f"const{prior:g}")
        self.name = f"raysearch-c{cf}-b{B}-{H}x{W}-n{N}-{pn}-{layout}-g{grid_mul}-thr{thr}-{lo:g}to{hi:g}"

    has_prior = R.LogitCase.has_prior
    table = R.SearchCase.table
    grid = Q.RayCase.grid

    @property
    def Nq(self):
        return self.N

    @property
    def large(self):
        return self.N > 4096


CASES = [SearchRayCase(*a) for a in (
    (4, 1, 5, 7, 1, None, "wide", 1, 0.5, 0.5, 8.0),
    (20, 3, 5, 7, 15, "tensor", "base1", 2, "edge", 0.5, 8.0),
    (64, 1, 12, 16, 16, -1.0, "wide", 2, 0.3, 0.5, 8.0),
    (64, 3, 12, 16, 37, "tensor", "odd", 1, "clamp", 1.0, 3.0, True),
    (68, 3, 5, 7, 17, None, "base1", 1, "one", 0.5, 8.0),
    (256, 1, 12, 16, 37, None, "wide", 2, 0.5, 0.5, 8.0),
    (64, Q.PERSISTENT_B, 5, 7, Q.PERSISTENT_N, None, "wide", 1, 0.5, 0.5, 8.0),
)]
assert len({c.name for c in CASES}) == len(CASES)


def case_inputs(case):
    """feat (B,Cf,H,W), rays (B,N,2), prior (B,N) | None - CPU fp32, seeded by the case name."""
    s = R._seed(case.name)
    feat = syn.randn((case.B, case.cf, case.H, case.W), s, "feat")
    rays = Q.case_rays(case)
    if case.nonfinite:
        rays[0, 5, 0] = float("nan")
        rays[case.B - 1, 7] = float("inf")
    prior = torch.tanh(syn.randn((case.B, case.N), s, "prior")) if case.prior == "tensor" else None
    return feat, rays, prior


def finite_rays(rays):
    """The rays the fp64 reference sees: a non-finite ray has no corner (include/idh.h), as a ray far outside the map."""
    bad = ~torch.isfinite(rays).all(-1, keepdim=True)
    return torch.where(bad, torch.full_like(rays, FAR), rays)


def prior_arg(case, prior):
    """The prior as ray_query_ref.reference / ray_bound take it: None | float | (B,N,1)."""
    return prior.unsqueeze(-1) if prior is not None else case.prior


def logits64(case, w, feat, rays, q, prior):
    """fp64 logits (B,N) of the MLP at the fp32 queries q (numpy or tensor, (B,N))."""
    d = torch.as_tensor(q).view(case.B, case.N, 1)
    return Q.reference(w, feat, finite_rays(rays), d, prior_arg(case, prior), case.grid)[..., 0]


def search_net(case):
    """mlp_op_ref.search_net's recipe on the rays: depth column of W1 tripled, b3 shifted so that the fp64 logit of the first query minus
    its threshold has median 0 over the rays."""
    m = R.make_net(case.cf, case.has_prior, R._seed(case.name), depth_gain=3.0)
    feat, rays, prior = case_inputs(case)
    q0 = np.full((case.B, case.N), R.first_query(case), dtype=np.float32)
    ref = logits64(case, R.weights64(m), feat, rays, q0, prior)
    shift = (ref - torch.from_numpy(R.thresholds_at(case, q0)[0].astype(np.float64))).median().item()
    with torch.no_grad():
        m.mlps["s0"][4].bias -= shift
    return m


def simulate(case, w, feat, rays, prior, iters=ITERS):
    """The search with the fp64 MLP deciding (queries kept in fp32): (final depth (B,N) fp32, flags (B,N) uint8, per-step dicts)."""
    shape = (case.B, case.N)
    lo = np.full(shape, case.lo, dtype=np.float32)
    hi = np.full(shape, case.hi, dtype=np.float32)
    q = np.full(shape, R.first_query(case), dtype=np.float32)
    flags = np.zeros(shape, np.uint8)
    steps = []
    for _ in range(iters):
        logit = logits64(case, w, feat, rays, q, prior).numpy()
        thr, idx = R.thresholds_at(case, q)
        vis = logit < thr
        steps.append({"q": q.copy(), "idx": idx, "vis": vis, "margin": np.abs(logit - thr)})
        flags |= np.where(vis, 1, 2).astype(np.uint8)
        lo, hi, q = R.search_step(case, lo, hi, q, logit, thr.astype(np.float64))
    return q, flags, steps


class ByteOut:
    """n bytes at an odd offset inside a prefilled uint8 buffer."""

    FILL, OFF = 0x5A, 5

    def __init__(self, n, device="cuda"):
        self.n = n
        self.buf = torch.full((n + 2 * self.OFF + 6,), self.FILL, dtype=torch.uint8, device=device)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.OFF

    def read(self):
        raw = self.buf.cpu()
        clean = bool((raw[:self.OFF] == self.FILL).all() and (raw[self.OFF + self.n:] == self.FILL).all())
        return raw[self.OFF: self.OFF + self.n].clone(), clean


class Device:
    """The case's device-side inputs, built once: hostile feature buffer (ray_query_ref.feature_buffer), packed weights with NaN in the
    unused vectors (mlp_op_ref.pack_net), rays, prior, Thresholder table."""

    def __init__(self, case, m, feat, rays, prior, device="cuda"):
        buf, self.off, self.cs = Q.feature_buffer(case, feat)
        self.fbuf = buf.to(device)
        self.w1p, self.w2p, self.vecs = R.pack_net(m, case.cf, case.has_prior, False, device)
        self.rays = rays.contiguous().to(device)
        self.prior = prior.contiguous().to(device) if prior is not None else None
        self.bins = self.thr_logits = None
        if case.table:
            self.bins, self.thr_logits = (t.to(device) for t in R.table_tensors(case))


def run_search(L, case, dev, iters, invK=None, wTc=None, want_flags=True, want_points=None):
    """One launch into prefilled outputs: (rc, depth Out, logits Out, flags ByteOut | None, points Out | None)."""
    from implicit_depth_amd import _lib

    M = case.B * case.N
    want_points = invK is not None if want_points is None else want_points
    depth, logits = R.Out(M), R.Out(M)
    flags = ByteOut(M) if want_flags else None
    points = R.Out(3 * M) if want_points else None
    gh, gw = case.grid
    rc = L.idh_binary_mlp_rays_search_fwd(
        dev.fbuf.data_ptr() + 4 * dev.off, dev.cs, case.cf, case.B, case.H, case.W, dev.rays.data_ptr(), _lib.ptr(dev.prior), int(case.has_prior),
        float(case.prior) if isinstance(case.prior, float) else 0.0, case.N, gw, gh, dev.w1p.data_ptr(), dev.w2p.data_ptr(), dev.vecs.data_ptr(),
        iters, case.lo, case.hi, 0.5 if case.table else case.thr, _lib.ptr(dev.bins), _lib.ptr(dev.thr_logits),
        0 if dev.bins is None else dev.bins.numel(), _lib.ptr(invK), _lib.ptr(wTc), depth.ptr, logits.ptr, flags.ptr if flags else None,
        points.ptr if points else None, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, depth, logits, flags, points


# ------------------------------------------------------------------------------------------------------------------
# hit points
# ------------------------------------------------------------------------------------------------------------------
def camera_matrices(case):
    """fp32 (invK (B,4,4) at the resolution of the case's grid, world_T_cam (B,4,4)), different per batch element."""
    gh, gw = case.grid
    iK = torch.stack([torch.linalg.inv(syn.intrinsics(gw + 2 * b, gh + b)) for b in range(case.B)]).float()
    wTc = torch.stack([syn.source_pose(b + 1) for b in range(case.B)]).float()
    return iK, wTc


def points_reference(rays, depth, invK, wTc=None):
    """(points (B,N,3) fp64, elementwise bound) of the module docstring, at fp32 inputs."""
    x, y, d = rays[..., 0].double(), rays[..., 1].double(), depth.double()
    iK = invK.double()
    t = torch.stack([iK[:, :3, 0, None] * x[:, None], iK[:, :3, 1, None] * y[:, None], iK[:, :3, 2, None].expand(-1, -1, x.shape[1])], -1)  # B,3,N,3
    c, Sc = t.sum(-1), t.abs().sum(-1)  # B,3,N
    X = (d[:, None] * c).permute(0, 2, 1)  # B,N,3
    eX = (d.abs()[:, None] * 2 * U * Sc + U * (d[:, None] * c).abs()).permute(0, 2, 1)
    if wTc is None:
        return X, eX
    T = wTc.double()
    Rm, tv = T[:, :3, :3], T[:, :3, 3]
    p = X @ Rm.transpose(1, 2) + tv[:, None]
    e = eX @ Rm.abs().transpose(1, 2) + 3 * U * (X.abs() @ Rm.abs().transpose(1, 2) + tv.abs()[:, None])
    return p, e
