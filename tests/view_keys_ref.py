"""Case table, inputs, fp64 first-valid reference and device calls of the occlusion and depth queries in a moving camera against SEVERAL
remembered keyframes (idh_binary_mlp_view_keys_fwd / idh_binary_mlp_view_keys_search_fwd, view_keys_k / view_keys_search_k in
csrc/mlp_rays.hip; include/idh.h states the fp32 expressions).

A pixel of the live view is projected into the keys ``key_slots[0..M-1]`` in turn and asked in the FIRST key in which it is valid; the
prior, the four feature corners and the MLP are the selected key's alone.  Per key the chain is ``view_query_ref.chain64`` (dense form) or
``view_search_ref.chain64_rays`` (ray list), the derived logit bound is ``view_query_ref.view_bound`` on the selected key's map, the search
rule is mlp_op_ref's; all four modules (view_query_ref, view_search_ref, ray_query_ref, mlp_op_ref) are imported as they are.

Geometry.  The keys are a ring of ``n_slots`` slots; slot s holds the keyframe pose yawed by KEY_YAW[s] (-0.5, 0, +0.5 rad; the keyframe's
horizontal field of view is 2 x 0.506 rad, so the three images tile 2 rad side by side) and moved by KEY_T[s] (centimetres).  The live
camera ("pan") stands at the keyframe pose, moved a little, behind a lens half as long: its image is wider and taller than the three
keys together are tall, so in every order each key answers a part of the view and the top and bottom bands have no key.  "behind" turns
the live camera by 149 degrees: no key sees any pixel.

A pixel is left out of the bound comparisons when its projection lies within PROJ_MARGIN of a validity or prior-texel boundary in ANY
key up to and including the selected one (every key when none is selected): there the fp32 chain may select another key.  The share is
capped at NEAR_CAP per case (and per step of the search); tests/test_view_keys_cpu.py asserts the cap on the fp64 chain alone.
"""
import numpy as np
import torch

import implicit_depth_amd.synthetic as syn
import mlp_op_ref as R
import ray_query_ref as Q
import ray_search_ref as S
import view_query_ref as V
import view_search_ref as VS

OK, EINVAL, EUNSUPPORTED = R.OK, R.EINVAL, R.EUNSUPPORTED
PROJ_MARGIN, NEAR_CAP = V.PROJ_MARGIN, V.NEAR_CAP
NONE = 255
KEY_YAW = (-0.5, 0.0, 0.5, 0.21)
KEY_T = ((0.03, -0.01, 0.02), (-0.02, 0.015, -0.01), (0.01, 0.02, 0.03), (0.0, -0.02, 0.01))
# the live camera under the pan: yaw, pitch (rad) and translation (m) against the keyframe pose - chosen, on the fp64 chain alone, so that
# the margin caps of tests/test_view_keys_cpu.py hold (a 63-ray case allows no probe on a prior-texel tie in twelve steps)
VIEW_YAW, VIEW_PITCH, VIEW_T = -0.023, -0.049, (0.009, 0.013, 0.02)
MIN_SHARE = 0.05  # of the pixels, for every key and for "none", in the main cases


class _Keys:
    """What the two case classes share: ``slots`` - the keys in priority order, slots of a ring of ``n_slots`` -, ``pose`` "pan" | "behind",
    ``stride_pad`` - floats between the end of a slot's (B,H,W,cs) block and the next block (None: two rows)."""

    def _keys(self, slots, n_slots, pose, stride_pad):
        self.slots = tuple(slots)
        self.n_slots = max(self.slots) + 1 if n_slots is None else n_slots
        self.pose, self.stride_pad = pose, stride_pad
        assert pose in ("pan", "behind") and len(set(self.slots)) == len(self.slots) and all(0 <= s < self.n_slots <= len(KEY_YAW) for s in self.slots)
        self.name += f"-{pose}-keys{''.join(map(str, self.slots))}of{self.n_slots}" + ("" if stride_pad is None else f"-pad{stride_pad}")

    @property
    def M(self):
        return len(self.slots)

    @property
    def main(self):
        """The cases on which the selection is asserted to be exercised: three keys under the pan."""
        return self.pose == "pan" and self.M == 3


class KeysCase(V.ViewCase, _Keys):
    """A (B,P,h,w) depth map of the live camera against the keys ``slots``; the other attributes are view_query_ref.ViewCase's."""

    def __init__(self, cf, B, H, W, P, h, w, prior, layout, fill=0.0, slots=(0, 1, 2), n_slots=None, pose="pan", stride_pad=None):
        V.ViewCase.__init__(self, cf, B, H, W, P, h, w, "moved" if pose == "pan" else "behind", prior, layout, fill)
        self._keys(slots, n_slots, pose, stride_pad)


class KeysSearchCase(VS.ViewSearchCase, _Keys):
    """An h x w grid (or LIST_N listed rays) of the live camera against the keys ``slots``; the rest is view_search_ref.ViewSearchCase's."""

    def __init__(self, cf, B, H, W, h, w, prior, layout, slots=(0, 1, 2), n_slots=None, pose="pan", stride_pad=None, **kw):
        VS.ViewSearchCase.__init__(self, cf, B, H, W, h, w, "moved" if pose == "pan" else "behind", prior, layout, **kw)
        self._keys(slots, n_slots, pose, stride_pad)


CASES = [KeysCase(*a, **k) for a, k in (
    ((64, 2, 12, 16, 3, 7, 9, "map", "base1", -7.5), {}),                                   # 378 rays: no multiple of 16, tiles straddle planes and batches
    ((64, 1, 24, 32, 1, 5, 3, -1.0, "base1", 2.25), {}),                                    # 15 rays: one partial tile
    ((64, 1, 12, 16, 1, 7, 9, "map", "wide"), dict(slots=(1,))),                            # M = 1
    ((64, 1, 24, 32, 2, 15, 20, "map", "wide", -2.0), dict(slots=(2, 1, 0), n_slots=4)),    # a permutation of 3 slots of a 4-slot ring
    ((64, 2, 12, 16, 2, 7, 9, "map", "wide", -3.0), dict(pose="behind")),                   # no key sees a pixel: all fill
    ((64, 2, 24, 32, 1, 15, 20, None, "odd", 1.0), dict(slots=(1, 2, 0))),                  # dword loads
    ((64, 1, 24, 32, 1, 15, 20, None, "wide", 0.5), dict(slots=(1, 0, 2), stride_pad=153)), # aligned rows, a key stride that is not: dword loads
    ((128, 2, 12, 16, 1, 7, 9, "map", "base1", -7.5), {}),                                  # W1f not in LDS
    ((64, 1, 12, 16, 1, 201, 245, None, "wide"), dict(slots=(0, 2))),                       # 49 245 rays = 3078 tiles > 1024: the persistent form
)]
SEARCH_CASES = [KeysSearchCase(*a, **k) for a, k in (
    ((64, 2, 12, 16, 7, 9, "map", "base1"), dict(thr="edge", fill=-7.5)),                          # 126 rays: tiles straddle the batch elements
    ((64, 1, 24, 32, 5, 3, -1.0, "base1"), dict(fill=-2.25)),                                      # 15 rays: one partial tile
    ((64, 1, 12, 16, 7, 9, "map", "wide"), dict(slots=(1,), thr="clamp", lo=1.0, hi=3.0, fill=3.0)),  # M = 1
    ((64, 1, 24, 32, 15, 20, "map", "wide"), dict(slots=(2, 1, 0), n_slots=4, fill=-6.0)),         # a permutation of 3 slots of a 4-slot ring
    ((64, 2, 12, 16, 7, 9, "map", "wide"), dict(pose="behind", fill=-3.0)),                        # every probe without a key
    ((64, 2, 24, 32, 6, 5, None, "odd"), dict(slots=(1, 2, 0), fill=1.0)),                         # dword loads
    ((128, 1, 12, 16, 7, 9, -1.0, "base1"), dict(fill=-7.0)),                                      # W1f not in LDS
    ((64, 1, 12, 16, 12, 16, None, "wide"), dict(thr="one", fill=-1.5, listed=True)),              # a ray list: centres, off-centre rays, rays outside the live image
    ((64, 1, 12, 16, 101, 163, None, "wide"), dict(slots=(0, 2), fill=-1.0)),                      # 16 463 rays = 1029 tiles > 1024: the persistent form
)]
assert len({c.name for c in CASES + SEARCH_CASES}) == len(CASES) + len(SEARCH_CASES)
LARGE = [c for c in CASES + SEARCH_CASES if c.rays > 4096]
LISTED = SEARCH_CASES[7]


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def _key_pose(slot, b):
    """world_T_cam (4,4) float64 of the key in ``slot``, batch element b: view_query_ref's keyframe pose, yawed and moved a little."""
    T = V._rot("y", KEY_YAW[slot] + 0.01 * b)
    T[:3, 3] = torch.tensor(KEY_T[slot], dtype=torch.float64)
    return syn.source_pose(b + 1) @ T


def _view_pose(case, b):
    if case.pose == "behind":
        return syn.source_pose(b + 1) @ V.relative_pose("behind", b)
    T = V._rot("y", VIEW_YAW + 0.04 * b) @ V._rot("x", VIEW_PITCH)
    T[:3, 3] = torch.tensor(VIEW_T, dtype=torch.float64)
    return syn.source_pose(b + 1) @ T


def cameras(case):
    """(view invK (B,4,4) at h x w behind a lens half as long, view world_T_cam (B,4,4), key cam_T_world, key K, prior cam_T_world, prior K:
    rings (n_slots,B,4,4)), fp32.  Slots the case does not use hold NaN."""
    B, n = case.B, case.n_slots
    Kv = syn.intrinsics(case.w, case.h).clone()
    Kv[0, 0], Kv[1, 1] = 0.5 * Kv[0, 0], 0.5 * Kv[1, 1]
    iK = torch.linalg.inv(Kv).expand(B, 4, 4)
    wTc = torch.stack([_view_pose(case, b) for b in range(B)])
    K = syn.intrinsics(case.W, case.H)
    cTw, Ks, pcTw = (torch.full((n, B, 4, 4), float("nan"), dtype=torch.float64) for _ in range(3))
    for s in case.slots:
        for b in range(B):
            key = _key_pose(s, b)
            cTw[s, b] = torch.linalg.inv(key)
            Ks[s, b] = K
            pcTw[s, b] = torch.linalg.inv(key @ syn.source_pose(b + 3 + s, big_rotation=True))  # turned by 0.6 rad: part of the key's image has no prior
    f = lambda t: t.float().contiguous()
    return f(iK), f(wTc), f(cTw), f(Ks), f(pcTw), f(Ks)


def key_cams(cams, slot):
    """The six matrices of view_query_ref.cameras for the key in ``slot``."""
    return (cams[0], cams[1]) + tuple(c[slot] for c in cams[2:])


def case_inputs(case):
    """feats (n_slots,B,cf,H,W), rendered (B,P,h,w) (dense cases) or rays (B,N,2) (search cases), the cameras of ``cameras``, prior ring
    (n_slots,B,1,H,W) | None - CPU fp32, seeded by the case name.  Slots the case does not use hold NaN."""
    s = R._seed(case.name)
    n, B = case.n_slots, case.B
    feats = torch.full((n, B, case.cf, case.H, case.W), R.NAN)
    prior = torch.full((n, B, 1, case.H, case.W), R.NAN) if case.prior == "map" else None
    for k in case.slots:
        feats[k] = syn.randn((B, case.cf, case.H, case.W), s, f"feat{k}")
        if prior is not None:
            prior[k] = torch.sigmoid(syn.randn((B, 1, case.H, case.W), s, f"prior{k}"))
    if isinstance(case, KeysSearchCase):
        third = VS.list_rays(case) if case.listed else VS.pixel_centres(B, case.h, case.w)
    else:
        third = V.rendered_map(B, case.P, case.h, case.w, s)
    return feats, third, cameras(case), prior


def prior_const(case):
    return float(case.prior) if isinstance(case.prior, float) else None


# ------------------------------------------------------------------------------------------------------------------
# fp64: the first valid key
# ------------------------------------------------------------------------------------------------------------------
def select(chains):
    """From the per-key chain dictionaries (priority order): sel (B,N) int64 - the first key whose ``valid`` holds, NONE where there is
    none -, near (B,N) - within the margin of a boundary in a key up to and including the selected one -, and the selected key's dictionary
    (uv, z, e_uv, e_z, prior, valid; key 0's entries where none is selected)."""
    valid = torch.stack([c["valid"] for c in chains])
    M = valid.shape[0]
    first = torch.where(valid.any(0), valid.float().argmax(0), torch.full(valid.shape[1:], M))  # M: none
    upto = torch.arange(M).view(M, 1, 1) <= first.clamp(max=M - 1).unsqueeze(0)
    near = (torch.stack([c["near"] for c in chains]) & upto).any(0)
    pick = first.clamp(max=M - 1) * (first < M)
    ch = {}
    for k in ("uv", "z", "cz", "e_uv", "e_z", "prior", "valid"):
        if chains[0][k] is None:
            ch[k] = None
            continue
        st = torch.stack([c[k] for c in chains])
        idx = pick.view(1, *pick.shape, *([1] * (st.dim() - 3))).expand(1, *st.shape[1:])
        ch[k] = st.gather(0, idx)[0]
    ch["dok"], ch["points"], ch["e_points"] = chains[0]["dok"], chains[0]["points"], chains[0]["e_points"]
    sel = torch.where(first < M, first, torch.full_like(first, NONE))
    return sel, near, ch


def _logits64(case, w, feats, ch, sel):
    """The MLP on [z_sel | feat_sel(u_sel, v_sel) | prior_sel], once per pixel: each key's map is sampled at the selected coordinates and
    the rows of its own pixels are kept."""
    f = torch.zeros(ch["z"].shape + (case.cf,), dtype=torch.float64)
    for m, slot in enumerate(case.slots):
        fm = Q.sample64(feats[slot], ch["uv"], (case.H, case.W)).permute(0, 2, 1)
        f = torch.where((sel == m).unsqueeze(-1), fm, f)
    cols = [ch["z"].unsqueeze(-1), f]
    pc = prior_const(case)
    pv = ch["prior"] if ch["prior"] is not None else (None if pc is None else torch.full_like(ch["z"], float(np.float32(pc))))
    if pv is not None:
        cols.append(pv.unsqueeze(-1))
    logit = Q.mlp64(w, torch.cat(cols, -1))
    return torch.where(sel != NONE, logit, torch.full_like(logit, case.fill))


def chains_dense(case, rendered, cams, prior):
    return [V.chain64(rendered, key_cams(cams, s), case.H, case.W, None if prior is None else prior[s]) for s in case.slots]


def reference(case, w, feats, rendered, cams, prior):
    """fp64 first-valid reference of the dense form: (logits (B,P,h,w) with ``fill`` where no key is valid, sel (B,N), near (B,N), the
    selected chain, the per-key chains)."""
    chains = chains_dense(case, rendered, cams, prior)
    sel, near, ch = select(chains)
    return _logits64(case, w, feats, ch, sel).view(rendered.shape), sel, near, ch, chains


def bound(case, w, feats, chains, sel):
    """(fp64 logits, bound) (B,N) of every pixel as if its selected key were valid: view_query_ref.view_bound per key, selected."""
    ref, tol = torch.zeros(sel.shape, dtype=torch.float64), torch.zeros(sel.shape, dtype=torch.float64)
    for m, slot in enumerate(case.slots):
        if bool((sel == m).any()):
            r, t = V.view_bound(w, feats[slot], chains[m], prior_const(case))
            ref, tol = torch.where(sel == m, r, ref), torch.where(sel == m, t, tol)
    return ref, tol


def step64(case, w, feats, rays, cams, prior, q):
    """One probe per ray of a search case at the fp32 queries q (B,N): (fp64 logits with ``fill`` where no key is valid, sel, near, the
    selected chain - its "z" is key 0's where none is valid -, the per-key chains)."""
    q = torch.as_tensor(q).view(case.B, case.N)
    chains = []
    for s in case.slots:
        pm = None if prior is None else prior[s]
        if case.listed:
            chains.append(VS.chain64_rays(rays, q, key_cams(cams, s), case.H, case.W, pm))
        else:
            chains.append(V.chain64(q.view(case.B, 1, case.h, case.w), key_cams(cams, s), case.H, case.W, pm))
    sel, near, ch = select(chains)
    return _logits64(case, w, feats, ch, sel), sel, near, ch, chains


def search_net(case):
    """view_search_ref.search_net's recipe on the first-valid chain: the depth column of W1 tripled, b3 shifted so that the fp64 logit of the
    first query minus its threshold has median 0 over the rays whose first probe has a key."""
    m = R.make_net(case.cf, case.has_prior, R._seed(case.name), depth_gain=3.0)
    feats, rays, cams, prior = case_inputs(case)
    q0 = np.full(case.shape, R.first_query(case), dtype=np.float32)
    ref, sel, _, ch, _ = step64(case, R.weights64(m), feats, rays, cams, prior, q0)
    if bool((sel != NONE).any()):
        thr = torch.from_numpy(R.thresholds_at(case, ch["z"].float().numpy())[0].astype(np.float64))
        with torch.no_grad():
            m.mlps["s0"][4].bias -= (ref - thr)[sel != NONE].median().item()
    return m


def simulate(case, w, feats, rays, cams, prior):
    """The search with the fp64 chain deciding (queries kept in fp32): (final depth (B,N) fp32, flags uint8, per-step dicts {q, sel, near})."""
    lo = np.full(case.shape, case.lo, dtype=np.float32)
    hi = np.full(case.shape, case.hi, dtype=np.float32)
    q = np.full(case.shape, R.first_query(case), dtype=np.float32)
    flags = np.zeros(case.shape, np.uint8)
    steps = []
    for _ in range(case.iters):
        logit, sel, near, ch, _ = step64(case, w, feats, rays, cams, prior, q)
        logit = logit.numpy()
        thr, _ = R.thresholds_at(case, ch["z"].float().numpy())
        steps.append({"q": q.copy(), "sel": sel.numpy(), "near": near.numpy()})
        flags |= (np.where(logit < thr, 1, 2) | np.where(sel.numpy() != NONE, 0, 4)).astype(np.uint8)
        lo, hi, q = R.search_step(case, lo, hi, q, logit, thr.astype(np.float64))
    return q, flags, steps


def first_valid(logits, valids, depths, fill):
    """The torch select of the composition: per pixel the first launch whose valid byte is 1.  ``logits`` / ``valids`` / ``depths``:
    lists over the keys.  Returns (logits with ``fill`` where none is valid, key uint8 with NONE, depth: the selected key's, key 0's where
    none is valid)."""
    out = torch.full_like(logits[0], fill)
    key = torch.full(valids[0].shape, NONE, dtype=torch.uint8, device=valids[0].device)
    depth = depths[0].clone()
    for m in reversed(range(len(logits))):
        v = valids[m].bool()
        out, depth = torch.where(v, logits[m], out), torch.where(v, depths[m], depth)
        key = torch.where(v, torch.full_like(key, m), key)
    return out, key, depth


# ------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------
class _Block:
    """One key of a case as a single-key case: every attribute view_query_ref / view_search_ref / ray_query_ref read is the case's own."""

    def __init__(self, case):
        self._case = case

    def __getattr__(self, k):
        return getattr(self._case, k)


def ring_buffer(case, feats):
    """NaN-filled CPU buffer holding the ring in the case's layout: (flat buffer, base offset in floats, feat_cs, key_stride in floats).
    A slot's block is ray_query_ref.feature_buffer's; everything between the blocks, and every unused slot, is NaN."""
    extra, off = Q.LAYOUTS[case.layout]
    cs = case.cf + extra
    block = case.B * case.H * case.W * cs
    stride = block + (2 * cs if case.stride_pad is None else case.stride_pad)
    buf = torch.full((off + case.n_slots * stride + 2 * cs,), R.NAN)
    for s in case.slots:
        one, o, c = Q.feature_buffer(case, feats[s])
        assert (o, c) == (off, cs)
        buf[off + s * stride: off + s * stride + block] = one[off: off + block]
    return buf, off, cs, stride


class Device:
    """A case's device-side inputs, built once: the hostile ring, packed weights, cameras, prior ring, third input (rendered map or rays),
    Thresholder table, the key_slots array."""

    def __init__(self, case, m, feats, third, cams, prior, device="cuda"):
        import ctypes as C

        buf, self.off, self.cs, self.stride = ring_buffer(case, feats)
        self.fbuf = buf.to(device)
        self.w1p, self.w2p, self.vecs = R.pack_net(m, case.cf, case.has_prior, False, device)
        self.cams = [t.contiguous().to(device) for t in cams]
        self.prior = prior.contiguous().to(device) if prior is not None else None
        self.third = third.contiguous().to(device)
        self.slots = (C.c_int * case.M)(*case.slots)
        self.bins = self.thr_logits = None
        if getattr(case, "table", None):
            self.bins, self.thr_logits = (t.to(device) for t in R.table_tensors(case))


def run_keys(L, case, dev, rendered=None, outputs=(True, True, True), slots=None, fbuf=None):
    """One launch of idh_binary_mlp_view_keys_fwd into prefilled outputs: (rc, logits Out, key ByteOut | None, depth Out | None, points
    Out | None).  ``rendered``: another (B,P,h,w) map on the device (the search's composition); ``slots``: another key order;
    ``fbuf``: another ring buffer of the same geometry."""
    from implicit_depth_amd import _lib
    import ctypes as C

    rd = dev.third if rendered is None else rendered
    n = rd.numel()
    P = rd.shape[1]
    logits = R.Out(n)
    key = S.ByteOut(n) if outputs[0] else None
    depth = R.Out(n) if outputs[1] else None
    points = R.Out(3 * n) if outputs[2] else None
    c, pm = dev.cams, dev.prior
    ks = dev.slots if slots is None else (C.c_int * len(slots))(*slots)
    fb = dev.fbuf if fbuf is None else fbuf
    rc = L.idh_binary_mlp_view_keys_fwd(
        fb.data_ptr() + 4 * dev.off, dev.cs, case.cf, case.B, case.H, case.W, dev.stride, case.n_slots, ks, len(ks), rd.data_ptr(), P,
        rd.shape[2], rd.shape[3], c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), c[3].data_ptr(), _lib.ptr(pm),
        c[4].data_ptr() if pm is not None else None, c[5].data_ptr() if pm is not None else None, int(case.has_prior),
        float(case.prior) if isinstance(case.prior, float) else 0.0, dev.w1p.data_ptr(), dev.w2p.data_ptr(), dev.vecs.data_ptr(),
        float(case.fill), logits.ptr, key.ptr if key else None, depth.ptr if depth else None, points.ptr if points else None, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, logits, key, depth, points


def run_keys_search(L, case, dev, iters=None, want_flags=True, want_points=True, want_key=True, listed=None, fbuf=None):
    """One launch of idh_binary_mlp_view_keys_search_fwd: (rc, depth Out, logits Out, flags ByteOut | None, points Out | None, key ByteOut | None)."""
    from implicit_depth_amd import _lib

    listed = case.listed if listed is None else listed
    n = case.rays
    depth, logits = R.Out(n), R.Out(n)
    flags = S.ByteOut(n) if want_flags else None
    points = R.Out(3 * n) if want_points else None
    key = S.ByteOut(n) if want_key else None
    c, pm = dev.cams, dev.prior
    fb = dev.fbuf if fbuf is None else fbuf
    rc = L.idh_binary_mlp_view_keys_search_fwd(
        fb.data_ptr() + 4 * dev.off, dev.cs, case.cf, case.B, case.H, case.W, dev.stride, case.n_slots, dev.slots, case.M,
        0 if listed else case.h, 0 if listed else case.w, dev.third.data_ptr() if listed else None, case.N if listed else 0,
        c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), c[3].data_ptr(), _lib.ptr(pm), c[4].data_ptr() if pm is not None else None,
        c[5].data_ptr() if pm is not None else None, int(case.has_prior), float(case.prior) if isinstance(case.prior, float) else 0.0,
        dev.w1p.data_ptr(), dev.w2p.data_ptr(), dev.vecs.data_ptr(), case.iters if iters is None else iters, case.lo, case.hi,
        0.5 if case.table else case.thr, _lib.ptr(dev.bins), _lib.ptr(dev.thr_logits), 0 if dev.bins is None else dev.bins.numel(),
        float(case.fill), depth.ptr, logits.ptr, flags.ptr if flags else None, points.ptr if points else None, key.ptr if key else None,
        _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, depth, logits, flags, points, key


def run_single(L, case, m, feats, rendered, cams, prior, slot):
    """The parent commit's launch for one key: view_query_ref.run_view (idh_binary_mlp_view_fwd) on that key's own map, cameras and prior.
    Returns CPU tensors (logits (n,), valid (n,) uint8, depth (n,), points (3n,))."""
    rc, logits, valid, depth, points = V.run_view(L, _Block(case), m, feats[slot], rendered, key_cams(cams, slot), None if prior is None else prior[slot])
    assert rc == OK
    (gl, c1), (gz, c2), (gp, c3) = logits.read(), depth.read(), points.read()
    raw = valid.cpu()
    n = case.rays
    assert c1 and c2 and c3 and bool((raw[:8] == 0x5A).all() and (raw[8 + n:] == 0x5A).all())
    return gl, raw[8:8 + n].clone(), gz, gp
