"""Case table, inputs, fp64 simulation and device call of the depth search in a moving camera (idh_binary_mlp_view_search_fwd, view_search_k
in csrc/mlp_rays.hip; include/idh.h states the fp32 expressions).

A ray is a pixel of the LIVE camera (or an entry of a ray list in that camera's pixel-centre units); the query q_n is the z-depth in that
camera, and one step of the search is one pixel of idh_binary_mlp_view_fwd on ``rendered = q_n``: the fp64 simulation below is
``view_query_ref.reference`` per step, with fp64 deciding and the queries kept in fp32; the rule is mlp_op_ref's (``first_query``,
``thresholds_at`` - keyed by the probe's KEYFRAME z -, ``search_step``), the derived logit bound is ``view_query_ref.view_bound``, and an
invalid probe's logit is ``fill``.  All three modules are imported as they are.

The list form has no grid, so ``chain64_rays`` restates ``view_query_ref.chain64`` for arbitrary (x, y) - the same terms, with |x|, |y| in
the bound of c_i; tests/test_view_search_cpu.py checks that it reproduces ``chain64`` exactly at pixel centres.

Hit points: ray_search_ref's derivation (c_i: two fmas, X_i = d c_i: one rounding, p_i: three fmas) at the kernel's own depth.
"""
import numpy as np
import torch

import implicit_depth_amd.synthetic as syn
import mlp_op_ref as R
import ray_query_ref as Q
import ray_search_ref as S
import view_query_ref as V

U = R.U
ITERS = R.SEARCH_ITERS
PROJ_MARGIN, NEAR_CAP = V.PROJ_MARGIN, V.NEAR_CAP
LIST_N = 37


class ViewSearchCase:
    """An h x w grid of the live camera ``camera`` (view_query_ref.CAMERAS), or - ``listed`` - LIST_N rays in the pixel-centre units of that
    h x w image, against a (B,H,W,cf) keyframe map.  prior: None | "map" | a float constant; thr: a constant threshold or a key of
    mlp_op_ref.TABLES; layout: ray_query_ref.LAYOUTS.  The attributes are those view_query_ref.run_view and mlp_op_ref's rule expect."""

    P = 1

    def __init__(self, cf, B, H, W, h, w, camera, prior, layout, thr=0.5, lo=0.5, hi=8.0, fill=0.0, iters=ITERS, listed=False, list_n=None, zoom=1.0):
        assert camera in V.CAMERAS and layout in Q.LAYOUTS
        self.cf, self.B, self.H, self.W, self.h, self.w, self.camera, self.prior, self.layout = cf, B, H, W, h, w, camera, prior, layout
        self.thr, self.lo, self.hi, self.fill, self.iters, self.listed, self.list_n, self.zoom = thr, lo, hi, fill, iters, listed, list_n or LIST_N, zoom
        pn = "noprior" if prior is None else (prior if isinstance(prior, str) else f"const{prior:g}")
        self.name = (f"viewsearch-c{cf}-b{B}-{H}x{W}-{'list' if listed else 'grid'}{h}x{w}-{camera}-{pn}-{layout}-thr{thr}-{lo:g}to{hi:g}"
                     f"-fill{fill:g}-it{iters}-z{zoom:g}")

    has_prior = R.LogitCase.has_prior
    table = R.SearchCase.table

    @property
    def N(self):
        return self.list_n if self.listed else self.h * self.w

    @property
    def rays(self):  # (view_query_ref.run_view's name for the number of pixels of a launch)
        return self.B * self.N

    @property
    def shape(self):
        return (self.B, self.N)


# Where the probes go (the reason for ``zoom`` and for the sign of ``fill``).  Along a live ray the keyframe projection runs on a straight line
# from the epipole (q -> 0) to the ray's vanishing point (q -> inf).  A ray that crosses the border of the keyframe's image between two
# probes that the rule keeps returning to - `fill` sends it one way, the MLP on the valid side the other - converges ONTO the border: by
# step n its probe lies within |du/dq| (hi - lo) 2^-n px of it, and PROJ_MARGIN = 1e-3 px is reached at steps 10 - 12 on a 24 x 32 map
# (|du/dq| ~ 4 px/m).  So the "moved" cases look through a longer lens, which puts the vanishing points inside the keyframe's image or to
# its right (rotation 0.31 - 0.35 rad: 0.29 - 0.33 W right of the centre) with the epipole outside on the right (t = (0.35, -0.12, 0.2):
# 2.1 W): a ray is invalid near and valid far, or never valid, and a negative `fill` ("visible": hi moves, the next probe is nearer) never
# comes back.  They still mix valid and invalid probes on a ray.  The CROSSING case keeps the lens and takes a 96 x 128 map (|du/dq| ~ 15 px/m
# at the border: a converging probe is within the margin with probability ~ 4 % at step 12) and 16 columns, so that a tile is a row of the
# view: its rays do converge onto the border, and it has tiles without a valid probe at some steps only.  The prior's nearest texel adds
# ties (0.4 % of the probes on average).  tests/test_view_search_cpu.py asserts the cap per case and step, on the fp64 simulation alone.
CASES = [ViewSearchCase(*a, **k) for a, k in (
    ((64, 1, 24, 32, 5, 3, "moved", -1.0, "base1"), dict(fill=-2.25, zoom=4.0)),                           # 15 rays: one partial tile
    ((64, 2, 12, 16, 7, 9, "moved", "map", "base1"), dict(thr="edge", fill=-7.5, zoom=2.0)),               # 126 rays: tiles straddle the batch elements
    ((64, 2, 12, 16, 7, 9, "behind", "map", "wide"), dict(fill=-3.0)),                                     # every probe invalid
    ((64, 2, 96, 128, 15, 16, "moved", None, "wide"), dict(fill=-6.0)),                                    # rays that leave the keyframe's frustum inside [lo, hi]
    ((128, 1, 12, 16, 7, 9, "moved", -1.0, "base1"), dict(fill=-7.0, zoom=4.0)),                           # W1f not in LDS
    ((64, 2, 24, 32, 6, 5, "own", None, "odd"), dict(fill=1.0, zoom=2.0)),                                 # dword loads
    ((64, 1, 12, 16, 5, 3, "own", None, "wide"), dict(iters=1)),
    ((64, 1, 12, 16, 7, 9, "own", "map", "wide"), dict(thr="clamp", lo=1.0, hi=3.0, fill=3.0, zoom=2.0)),
    ((64, 1, 12, 16, 12, 16, "moved", None, "wide"), dict(thr="one", fill=-1.5, listed=True, zoom=4.0)),   # pixel centres, off-centre rays, rays outside the live image
    ((64, 1, 12, 16, 101, 163, "moved", None, "wide"), dict(fill=-1.0, zoom=4.0)),                         # 16 463 rays = 1029 tiles > 1024: the persistent 12-wave form
)]
assert len({c.name for c in CASES}) == len(CASES)
LARGE = [c for c in CASES if c.rays > 4096]
SMALL = [c for c in CASES if c not in LARGE]
CROSSING = CASES[3]
LISTED = CASES[8]


def pixel_centres(B, h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5, indexing="ij")
    return torch.stack([xs, ys], -1).view(1, h * w, 2).expand(B, -1, -1).contiguous()


def list_rays(case):
    """(B, LIST_N, 2): 12 pixel centres, 13 rays anywhere inside the h x w image, 12 rays up to 6 px outside it."""
    g = torch.Generator().manual_seed(R._seed(case.name) & 0x7FFFFFFF)
    size = torch.tensor([float(case.w), float(case.h)])
    centres = torch.floor(torch.rand((case.B, 12, 2), generator=g) * size) + 0.5
    inside = torch.rand((case.B, 13, 2), generator=g) * size
    side = torch.rand((case.B, 12, 2), generator=g) < 0.5
    off = 0.25 + 5.75 * torch.rand((case.B, 12, 2), generator=g)
    outside = torch.where(side, -off, size + off)
    return torch.cat([centres, inside, outside], 1).float().contiguous()


def cameras(case):
    """view_query_ref.cameras with the live lens ``zoom`` times longer (a power of two: exact in fp32), the principal point kept."""
    cams = V.cameras(case.camera, case.B, case.H, case.W, case.h, case.w)
    iK = cams[0].clone()
    iK[:, :2, :3] /= case.zoom
    return (iK,) + tuple(cams[1:])


def case_inputs(case):
    """feat (B,cf,H,W), rays (B,N,2) in the live camera's pixel-centre units (the pixel centres in grid form), the six matrices of
    view_query_ref.cameras, prior map (B,1,H,W) | None - CPU fp32, seeded by the case name."""
    s = R._seed(case.name)
    feat = syn.randn((case.B, case.cf, case.H, case.W), s, "feat")
    cams = cameras(case)
    prior = torch.sigmoid(syn.randn((case.B, 1, case.H, case.W), s, "prior")) if case.prior == "map" else None
    rays = list_rays(case) if case.listed else pixel_centres(case.B, case.h, case.w)
    return feat, rays, cams, prior


def prior_const(case):
    return float(case.prior) if isinstance(case.prior, float) else None


# ------------------------------------------------------------------------------------------------------------------
# fp64: one step, and the whole search
# ------------------------------------------------------------------------------------------------------------------
def chain64_rays(rays, q, cams, H, W, prior=None):
    """view_query_ref.chain64 for rays (B,N,2) at arbitrary (x, y) and depths q (B,N), all finite and positive: the same dictionary."""
    iK, wTc, cTw, K, pcTw, pK = (m.double() for m in cams)
    B, N = q.shape
    pix = torch.cat([rays.double(), torch.ones(B, N, 1, dtype=torch.float64)], -1)
    c = pix @ iK[:, :3, :3].transpose(1, 2)
    e_c = 2 * U * (pix.abs() @ iK[:, :3, :3].abs().transpose(1, 2))
    d = q.double().unsqueeze(-1)
    X = d * c
    e_X = d * e_c + U * X.abs()
    Rm, t = wTc[:, :3, :3], wTc[:, :3, 3]
    Ra = Rm.abs().transpose(1, 2)
    p = X @ Rm.transpose(1, 2) + t.view(B, 1, 3)
    e_p = e_X @ Ra + 3 * U * (X.abs() @ Ra + t.abs().view(B, 1, 3))
    dok = torch.ones(B, N, dtype=torch.bool)
    key = V._project64(p, e_p, cTw, K)
    u, v, cz = key["uv"][..., 0], key["uv"][..., 1], key["cz"]
    valid = (cz > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    m = PROJ_MARGIN
    near = (cz.abs() < m) | ((cz > 0) & ((u.abs() < m) | ((u - W).abs() < m) | (v.abs() < m) | ((v - H).abs() < m)))
    out = {"dok": dok, "points": p, "e_points": 2 * e_p, "uv": key["uv"], "z": key["z"], "cz": cz, "valid": valid, "e_uv": key["e_uv"],
           "e_z": key["e_z"], "e_cz": key["e_cz"], "prior": None}
    if prior is not None:
        pr = V._project64(p, e_p, pcTw, pK)
        sx, sy, pcz = pr["uv"][..., 0] - 0.5, pr["uv"][..., 1] - 0.5, pr["cz"]
        xr, yr = torch.round(sx), torch.round(sy)
        ok = (pcz > 0) & (xr >= 0) & (xr <= W - 1) & (yr >= 0) & (yr <= H - 1)
        val = prior.double()[torch.arange(B).view(B, 1), 0, yr.clamp(0, H - 1).long(), xr.clamp(0, W - 1).long()]
        out["prior"] = torch.where(ok, val, torch.full_like(val, -1.0))
        tie = lambda s: ((s - 0.5) - torch.round(s - 0.5)).abs() < m
        near = near | (valid & ((pcz.abs() < m) | ((pcz > 0) & (tie(sx) | tie(sy)))))
        out.update(e_prior_uv=pr["e_uv"], e_prior_cz=pr["e_cz"], prior_cz=pcz, prior_uv=pr["uv"])
    out["near"] = near
    return out


def step64(case, w, feat, rays, cams, prior, q):
    """One probe per ray at the fp32 queries q (B,N; numpy or tensor): (fp64 logits (B,N) with ``fill`` at the invalid probes, the chain's
    dictionary).  Grid form: view_query_ref.reference on the map rendered = q; list form: the same chain at the rays' own (x, y)."""
    q = torch.as_tensor(q).view(case.B, case.N)
    if not case.listed:
        logit, ch = V.reference(w, feat, q.view(case.B, 1, case.h, case.w), cams, prior, prior_const(case), case.fill)
        return logit.view(case.B, case.N), ch
    ch = chain64_rays(rays, q, cams, case.H, case.W, prior)
    f = Q.sample64(feat, ch["uv"], (case.H, case.W)).permute(0, 2, 1)
    cols = [ch["z"].unsqueeze(-1), f]
    pc = prior_const(case)
    pv = ch["prior"] if ch["prior"] is not None else (None if pc is None else torch.full_like(ch["z"], float(np.float32(pc))))
    if pv is not None:
        cols.append(pv.unsqueeze(-1))
    logit = Q.mlp64(w, torch.cat(cols, -1))
    return torch.where(ch["valid"], logit, torch.full_like(logit, case.fill)), ch


def search_net(case):
    """ray_search_ref.search_net's recipe: the depth column of W1 tripled, b3 shifted so that the fp64 logit of the first query minus its
    threshold has median 0 over the rays whose first probe is valid (an invalid probe's logit is ``fill`` whatever the network)."""
    m = R.make_net(case.cf, case.has_prior, R._seed(case.name), depth_gain=3.0)
    feat, rays, cams, prior = case_inputs(case)
    q0 = np.full(case.shape, R.first_query(case), dtype=np.float32)
    ref, ch = step64(case, R.weights64(m), feat, rays, cams, prior, q0)
    if ch["valid"].any():
        thr = torch.from_numpy(R.thresholds_at(case, ch["z"].float().numpy())[0].astype(np.float64))
        shift = (ref - thr)[ch["valid"]].median().item()
        with torch.no_grad():
            m.mlps["s0"][4].bias -= shift
    return m


def simulate(case, w, feat, rays, cams, prior, iters=None):
    """The search with the fp64 chain deciding (queries kept in fp32, the threshold looked up at the fp32 value of the fp64 keyframe z):
    (final depth (B,N) fp32, flags (B,N) uint8, per-step dicts {q, z, valid, near, vis, margin, idx})."""
    iters = case.iters if iters is None else iters
    lo = np.full(case.shape, case.lo, dtype=np.float32)
    hi = np.full(case.shape, case.hi, dtype=np.float32)
    q = np.full(case.shape, R.first_query(case), dtype=np.float32)
    flags = np.zeros(case.shape, np.uint8)
    steps = []
    for _ in range(iters):
        logit, ch = step64(case, w, feat, rays, cams, prior, q)
        logit, valid = logit.numpy(), ch["valid"].numpy()
        thr, idx = R.thresholds_at(case, ch["z"].float().numpy())
        vis = logit < thr
        steps.append({"q": q.copy(), "z": ch["z"].numpy(), "valid": valid, "near": ch["near"].numpy(), "vis": vis, "idx": idx,
                      "margin": np.abs(logit - thr), "uv": ch["uv"].numpy()})
        flags |= (np.where(vis, 1, 2) | np.where(valid, 0, 4)).astype(np.uint8)
        lo, hi, q = R.search_step(case, lo, hi, q, logit, thr.astype(np.float64))
    return q, flags, steps


def points_reference(rays, depth, cams):
    """World points of depth (B,N) along rays (B,N,2) of the live camera: ray_search_ref.points_reference with the view's invK / world_T_cam."""
    return S.points_reference(rays, depth, cams[0], cams[1])


# ------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------
class Device:
    """The case's device-side inputs, built once: hostile feature buffer (every float outside the map's rows and channels is NaN, two
    poisoned rows behind it), packed weights, matrices, prior map, rays, Thresholder table."""

    def __init__(self, case, m, feat, rays, cams, prior, device="cuda"):
        buf, self.off, self.cs = Q.feature_buffer(case, feat)
        self.fbuf = buf.to(device)
        self.w1p, self.w2p, self.vecs = R.pack_net(m, case.cf, case.has_prior, False, device)
        self.cams = [t.contiguous().to(device) for t in cams]
        self.prior = prior.contiguous().to(device) if prior is not None else None
        self.rays = rays.contiguous().to(device)
        self.bins = self.thr_logits = None
        if case.table:
            self.bins, self.thr_logits = (t.to(device) for t in R.table_tensors(case))


def run_view_search(L, case, dev, iters=None, want_flags=True, want_points=True, listed=None):
    """One launch into prefilled outputs: (rc, depth Out, logits Out, flags ByteOut | None, points Out | None).  ``listed``: pass the rays
    as a list (default: the case's own form; a grid case's rays are its pixel centres, so both forms are legal for it)."""
    from implicit_depth_amd import _lib

    listed = case.listed if listed is None else listed
    M = case.rays
    depth, logits = R.Out(M), R.Out(M)
    flags = S.ByteOut(M) if want_flags else None
    points = R.Out(3 * M) if want_points else None
    c, pm = dev.cams, dev.prior
    rc = L.idh_binary_mlp_view_search_fwd(
        dev.fbuf.data_ptr() + 4 * dev.off, dev.cs, case.cf, case.B, case.H, case.W, 0 if listed else case.h, 0 if listed else case.w,
        dev.rays.data_ptr() if listed else None, case.N if listed else 0, c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), c[3].data_ptr(),
        _lib.ptr(pm), c[4].data_ptr() if pm is not None else None, c[5].data_ptr() if pm is not None else None, int(case.has_prior),
        float(case.prior) if isinstance(case.prior, float) else 0.0, dev.w1p.data_ptr(), dev.w2p.data_ptr(), dev.vecs.data_ptr(),
        case.iters if iters is None else iters, case.lo, case.hi, 0.5 if case.table else case.thr, _lib.ptr(dev.bins), _lib.ptr(dev.thr_logits),
        0 if dev.bins is None else dev.bins.numel(), float(case.fill), depth.ptr, logits.ptr, flags.ptr if flags else None,
        points.ptr if points else None, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, depth, logits, flags, points


def probe_by_view_fwd(L, case, m, feat, cams, prior, q):
    """What one step is by definition: idh_binary_mlp_view_fwd on the map rendered = q (grid form).  (pred with fill, keyframe z, valid) as
    numpy (B,N)."""
    rd = torch.as_tensor(q).view(case.B, 1, case.h, case.w)
    rc, logits, valid, depth, _ = V.run_view(L, case, m, feat, rd, cams, prior, outputs=(True, True, False))
    assert rc == R.OK
    (gl, c1), (gz, c2) = logits.read(), depth.read()
    assert c1 and c2
    n = case.rays
    return gl.view(case.shape).numpy(), gz.view(case.shape).numpy(), valid.cpu()[8:8 + n].view(case.shape).numpy().astype(bool)


def probe_by_points(L, case, m, feat, cams, prior, points):
    """The same step for a ray list, whose rays no depth map can express: idh_project_points_fwd + idh_binary_mlp_rays_fwd (S = 1) on the
    world points of the probes - the bits idh_binary_mlp_view_fwd is documented to carry (include/idh.h) - with ``fill`` patched in."""
    B, N = case.shape
    pts = points.view(B, N, 3).contiguous().cuda()
    c = [t.contiguous().cuda() for t in cams]
    pm = prior.contiguous().cuda() if prior is not None else None
    rays, depth = torch.empty(B, N, 2, device="cuda"), torch.empty(B, N, device="cuda")
    valid = torch.empty(B, N, dtype=torch.uint8, device="cuda")
    pout = torch.empty(B, N, device="cuda") if pm is not None else None
    from implicit_depth_amd import _lib

    rc = L.idh_project_points_fwd(pts.data_ptr(), c[2].data_ptr(), c[3].data_ptr(), B, N, case.H, case.W, rays.data_ptr(), depth.data_ptr(),
                                  valid.data_ptr(), _lib.ptr(pm), c[4].data_ptr() if pm is not None else None,
                                  c[5].data_ptr() if pm is not None else None, _lib.ptr(pout), _lib.stream_ptr())
    assert rc == R.OK
    torch.cuda.synchronize()
    v = valid.cpu().bool()
    # an invalid probe reads nothing: ask it far outside the map, its logit is replaced by fill
    r = torch.where(v.unsqueeze(-1), rays.cpu(), torch.full((B, N, 2), S.FAR))
    pr = pout.cpu().unsqueeze(-1) if pout is not None else None

    class _Rays:  # the attributes ray_query_ref.run_rays reads
        cf, B, H, W, layout, step, S, prior = case.cf, case.B, case.H, case.W, case.layout, 1, 1, ("tensor" if pout is not None else case.prior)
        N = Nq = case.N
        has_prior = case.has_prior
        grid = (case.H, case.W)

    rc, out = Q.run_rays(L, _Rays, m, feat, r, depth.cpu().unsqueeze(-1), pr)
    assert rc == R.OK
    lg, clean = out.read()
    assert clean
    lg = torch.where(v, lg.view(B, N), torch.full((B, N), float(np.float32(case.fill))))
    return lg.numpy(), depth.cpu().numpy(), v.numpy()


def compose(case, probe, iters=None):
    """The composition a caller had before: ``iters`` single probes with the fp32 rule between them.  ``probe(q, n)`` -> (pred with fill,
    keyframe z, valid).  Returns (depth, last logit, flags, per-step dicts {q, logit, z, valid})."""
    iters = case.iters if iters is None else iters
    lo = np.full(case.shape, case.lo, dtype=np.float32)
    hi = np.full(case.shape, case.hi, dtype=np.float32)
    q = np.full(case.shape, R.first_query(case), dtype=np.float32)
    flags = np.zeros(case.shape, np.uint8)
    steps, logit = [], None
    for n in range(iters):
        logit, z, valid = probe(q, n)
        thr, _ = R.thresholds_at(case, z)
        steps.append({"q": q.copy(), "logit": logit.copy(), "z": z.copy(), "valid": valid.copy()})
        flags |= (np.where(logit < thr, 1, 2) | np.where(valid, 0, 4)).astype(np.uint8)
        lo, hi, q = R.search_step(case, lo, hi, q, logit, thr)
    return q, logit, flags, steps


# ------------------------------------------------------------------------------------------------------------------
# the golden of the reference's own modules (tests/golden/view_search.npz, written by tests/golden/gen_golden_view_search.py)
# ------------------------------------------------------------------------------------------------------------------
GOLDEN_B, GOLDEN_H, GOLDEN_W, GOLDEN_h, GOLDEN_w, GOLDEN_SEED = 2, 12, 16, 7, 9, 4242
GOLDEN_CASE = ViewSearchCase(64, GOLDEN_B, GOLDEN_H, GOLDEN_W, GOLDEN_h, GOLDEN_w, "moved", None, "wide")


def golden_inputs():
    """(feature_s0 (2,64,12,16), the six matrices of the moved view at 7 x 9); the net is ``golden_net``."""
    feat = syn.randn((GOLDEN_B, 64, GOLDEN_H, GOLDEN_W), GOLDEN_SEED, "golden_view_search_feat")
    return feat, V.cameras("moved", GOLDEN_B, GOLDEN_H, GOLDEN_W, GOLDEN_h, GOLDEN_w)


def golden_net(cls=None):
    """ray_query_ref.golden_net with the depth column of W1 tripled and b3 shifted by ``search_net``'s recipe on the golden inputs (fp64,
    decided on this module alone), so that the first-step decisions split."""
    m = Q.golden_net(cls) if cls is not None else Q.golden_net()
    feat, cams = golden_inputs()
    case = GOLDEN_CASE
    with torch.no_grad():
        m.mlps["s0"][0].weight[:, 0] *= 3.0
    w = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    q0 = np.full(case.shape, R.first_query(case), dtype=np.float32)
    ref, ch = step64(case, w, feat, pixel_centres(case.B, case.h, case.w), cams, None, q0)
    with torch.no_grad():
        m.mlps["s0"][4].bias -= ref[ch["valid"]].median().item()  # thr = logit(0.5) = 0
    return m
