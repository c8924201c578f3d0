"""Case table, inputs, the march rule in numpy fp32, its fp64 simulation and the device calls of the first-hit queries in a moving camera
(idh_binary_mlp_view_march_fwd / idh_binary_mlp_view_keys_march_fwd, view_march_k / view_keys_march_k in csrc/mlp_rays.hip; include/idh.h
states the rule).

A probe is what it is in view_search_ref / view_keys_ref - one pixel of idh_binary_mlp_view_fwd (idh_binary_mlp_view_keys_fwd) on the map
rendered = q - so the fp64 chain (``step64``), the derived logit bound (``view_query_ref.view_bound``), the margin rule, the hostile
feature buffers, ``Device`` and ``Out`` are those modules', imported as they are.  What is new is the rule between the probes: ``March``
below restates it per global step exactly as the header does (a ray that is done is frozen); ``brute_force`` restates it once more, ray by
ray in Python scalars, for the CPU test.
"""
import numpy as np
import torch

import mlp_op_ref as R
import ray_query_ref as Q
import ray_search_ref as S
import view_keys_ref as VK
import view_query_ref as V
import view_search_ref as VS

OK, EINVAL, EUNSUPPORTED = R.OK, R.EINVAL, R.EUNSUPPORTED
PROJ_MARGIN, NEAR_CAP = V.PROJ_MARGIN, V.NEAR_CAP
NONE = 255
F32 = np.float32


class _March:
    def _march(self, n_march, refine, spacing, salt):
        self.n_march, self.refine, self.spacing, self.salt = n_march, refine, spacing, salt
        self.name += f"-march{n_march}{spacing}-R{refine}"


class MarchCase(VS.ViewSearchCase, _March):
    """view_search_ref.ViewSearchCase (``iters`` is unused) with ``n_march`` samples from ``lo`` to ``hi`` (``spacing``) and ``refine`` steps."""

    keys = False

    def __init__(self, *a, n_march=9, refine=6, spacing="linear", salt="", **k):
        VS.ViewSearchCase.__init__(self, *a, **k)
        self._march(n_march, refine, spacing, salt)


class KeysMarchCase(VK.KeysSearchCase, _March):
    keys = True

    def __init__(self, *a, n_march=9, refine=6, spacing="linear", salt="", **k):
        VK.KeysSearchCase.__init__(self, *a, **k)
        self._march(n_march, refine, spacing, salt)


CASES = [MarchCase(*a, **k) for a, k in (
    ((64, 2, 12, 16, 7, 9, "moved", "map", "base1"), dict(salt="91", thr="edge", fill=7.5, zoom=2.0)),                  # A: 126 rays, tiles straddle the batch elements
    ((64, 2, 96, 128, 15, 16, "moved", None, "wide"), dict(salt="14", fill=6.0)),                             # B: a tile is a row of the view
    ((64, 2, 12, 16, 7, 9, "moved", "map", "base1"), dict(salt="2", thr="edge", fill=-7.5, zoom=2.0)),       # A with fill < 0: whole tiles finish at s = 0 or 1
    ((64, 1, 24, 32, 5, 3, "moved", -1.0, "base1"), dict(salt="4", fill=2.25, zoom=4.0)),                              # 15 rays: one partial tile
    ((128, 1, 12, 16, 7, 9, "moved", -1.0, "base1"), dict(salt="6", fill=7.0, zoom=4.0)),                              # W1f not in LDS
    ((64, 2, 24, 32, 6, 5, "moved", None, "odd"), dict(salt="7", fill=1.0, zoom=2.0)),                                 # dword loads
    ((64, 2, 12, 16, 7, 9, "behind", "map", "wide"), dict(fill=3.0)),                                        # every probe invalid: all "none"
    ((64, 1, 12, 16, 12, 16, "moved", None, "wide"), dict(salt="1", thr="one", fill=1.5, listed=True, zoom=4.0)),      # the 37-ray list
    ((64, 1, 12, 16, 5, 3, "own", None, "wide"), dict(n_march=1)),
    ((64, 1, 12, 16, 7, 9, "moved", None, "wide"), dict(refine=0, fill=4.0, zoom=2.0)),
    ((64, 1, 12, 16, 7, 9, "moved", None, "wide"), dict(salt="5", spacing="inverse", fill=4.0, zoom=2.0)),
    ((64, 1, 12, 16, 7, 9, "own", "map", "wide"), dict(salt="12", thr="clamp", lo=1.0, hi=3.0, fill=3.0, zoom=2.0)),
    ((64, 1, 12, 16, 101, 163, "moved", None, "wide"), dict(fill=1.0, zoom=4.0, n_march=5, refine=3)),       # 1029 tiles > 1024: the persistent form
)]
KEYS_CASES = [KeysMarchCase(*a, **k) for a, k in (
    ((64, 2, 12, 16, 7, 9, "map", "base1"), dict(salt="1", thr="edge", fill=7.5)),                                     # M = 3 under the pan
    ((64, 1, 24, 32, 5, 3, -1.0, "base1"), dict(fill=-2.25)),                                                # 15 rays: one partial tile
    ((64, 1, 12, 16, 7, 9, "map", "wide"), dict(salt="3", slots=(1,), fill=3.0)),                                      # M = 1
    ((64, 1, 24, 32, 15, 20, "map", "wide"), dict(salt="9", slots=(2, 1, 0), n_slots=4, fill=6.0)),                    # a permutation of a 4-slot ring, slot 3 all NaN
    ((64, 1, 12, 16, 201, 245, None, "wide"), dict(salt="1", slots=(0, 2), fill=1.0, n_march=4, refine=2)),  # 3078 tiles: the persistent form
)]
assert len({c.name for c in CASES + KEYS_CASES}) == len(CASES) + len(KEYS_CASES)
A, B, A_NEG, LISTED = CASES[0], CASES[1], CASES[2], CASES[7]
LARGE = [c for c in CASES + KEYS_CASES if c.rays > 4096]
SMALL = [c for c in CASES + KEYS_CASES if c not in LARGE]
# ``salt`` is appended to the seed of a case's network (``march_net``).  The geometry of a case fixes which probes lie within PROJ_MARGIN of a
# prior-texel tie or of the image border at the shared samples - a whole row of the view can sit near one at one sample - and the network
# decides which rays are still marching there; the salts were chosen, on the fp64 chain alone, as the first for which at most NEAR_CAP of the probes
# EVALUATED at a step lie inside the margin - none at all at a step with fewer than 100 rays still going - and (main cases) the conditions
# below hold.  tests/test_view_march_cpu.py asserts both.
# the conditions the main cases must meet on the fp64 chain alone (tests/test_view_march_cpu.py)
MIN_BRACKETED, MIN_NONE, MIN_RECROSS, MIN_FIRST = 0.20, 0.05, 0.05, 0.05
MIN_DECIDED_RECROSS = 0.05  # of the rays: what test (7) of tests/test_view_march_gpu.py is asserted on (decided_recross)


def samples(case, n_march=None):
    """The march depths in numpy fp32, every operation rounded to fp32: t_i = i / (n - 1); "linear": lo + (hi - lo) t_i; "inverse":
    1 / (1 / lo + (1 / hi - 1 / lo) t_i); the ends are lo and hi themselves; n = 1: [lo]."""
    n = case.n_march
    lo, hi = F32(case.lo), F32(case.hi)
    if n == 1:
        out = np.array([lo], dtype=F32)
    else:
        t = np.arange(n, dtype=F32) / F32(n - 1)
        if case.spacing == "linear":
            out = (lo + (hi - lo) * t).astype(F32)
        else:
            one = F32(1.0)
            out = (one / (one / lo + (one / hi - one / lo) * t)).astype(F32)
        out[0], out[-1] = lo, hi
    assert out.dtype == F32 and np.isfinite(out).all() and (out > 0).all() and (np.diff(out) > 0).all()
    return out[: n if n_march is None else n_march]


# ------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------
class March:
    """The rule of include/idh.h per global step, in numpy fp32, for all rays at once.  st: -1 marching, n > 0 refining with n steps
    left, 0 done.  ``queries()`` gives the depth every ray asks at this step (a done ray's is its final depth: it is carried, frozen);
    ``update`` takes that step's logits (fp32 or fp64), thresholds, validity and - keys form - selected key, for every ray."""

    def __init__(self, case, q_s, refine=None):
        sh = case.shape
        self.q_s, self.n, self.R = np.asarray(q_s, dtype=F32), len(q_s), case.refine if refine is None else refine
        self.st = np.full(sh, -1, np.int64)
        self.lo, self.hi, self.sd = (np.zeros(sh, F32) for _ in range(3))
        self.logit = np.zeros(sh, np.float64)
        self.flags, self.hit, self.key = np.zeros(sh, np.uint8), np.full(sh, NONE, np.uint8), np.full(sh, NONE, np.uint8)
        self.it = 0

    @property
    def active(self):
        return self.st != 0

    def more(self):
        return self.it < self.n + self.R and bool(self.active.any())

    def queries(self):
        return np.where(self.st < 0, self.q_s[min(self.it, self.n - 1)], self.sd).astype(F32)

    def update(self, logit, thr, valid, key=None):
        a, q, it = self.active, self.queries(), self.it
        marching = self.st < 0
        behind = logit < thr
        nhi, nlo = np.where(behind, q, self.hi).astype(F32), np.where(behind, self.lo, q).astype(F32)
        bracket = marching & behind & (it > 0)
        nst = np.where(marching, np.where(behind, self.R if it > 0 else 0, 0 if it == self.n - 1 else -1), self.st - 1)
        nsd = np.where(bracket | ~marching, ((nhi + nlo) * F32(0.5)).astype(F32), q).astype(F32)
        self.flags = np.where(a, self.flags | np.where(behind, 1, 2).astype(np.uint8) | np.where(valid, 0, 4).astype(np.uint8), self.flags).astype(np.uint8)
        self.hit = np.where(a & marching & behind, it, self.hit).astype(np.uint8)
        self.logit = np.where(a, logit, self.logit)
        if key is not None:
            self.key = np.where(a, key, self.key).astype(np.uint8)
        self.hi, self.lo, self.sd, self.st = (np.where(a, n, o) for n, o in ((nhi, self.hi), (nlo, self.lo), (nsd, self.sd), (nst, self.st)))
        self.it += 1
        return a


def run_rule(case, probe, q_s=None, refine=None):
    """The composition: one ``probe(q)`` -> {logit, z, valid, key | None, ...} over ALL rays per global step, the rule between them.
    Returns (March at its end, per-step records: the probe's dictionary plus q, active, thr, idx)."""
    mc = March(case, samples(case) if q_s is None else q_s, refine)
    steps = []
    while mc.more():
        q = mc.queries()
        p = dict(probe(q))
        thr, idx = R.thresholds_at(case, np.asarray(p["z"], dtype=F32))
        p.update(q=q, thr=thr, idx=idx, it=mc.it, marching=mc.st < 0)
        p["active"] = mc.update(p["logit"], thr, p["valid"], p.get("key"))
        steps.append(p)
    return mc, steps


def brute_force(case, q_s, table, refine_probe):
    """The header's rule once more, ray by ray in Python scalars.  ``table``: {behind, valid} (n_march, rays) at the shared samples;
    ``refine_probe(q (rays,) fp32) -> (behind, valid)`` evaluates one query per ray (only the bracketed rays' entries are used).
    Returns (depth, flags, hit) as flat arrays."""
    n, R_, rays = len(q_s), case.refine, case.rays
    depth, flags, hit = np.zeros(rays, F32), np.zeros(rays, np.uint8), np.full(rays, NONE, np.uint8)
    lo, hi = np.zeros(rays, F32), np.zeros(rays, F32)
    bracketed = []
    for r in range(rays):
        s_star, f = None, 0
        for s in range(n):
            if not table["valid"][s, r]:
                f |= 4
            if table["behind"][s, r]:
                s_star = s
                break
        if s_star is None:
            depth[r], f = q_s[n - 1], f | 2
        elif s_star == 0:
            depth[r], f, hit[r] = q_s[0], f | 1, 0
        else:
            lo[r], hi[r], f, hit[r] = q_s[s_star - 1], q_s[s_star], f | 3, s_star
            bracketed.append(r)
        flags[r] = f
    for _ in range(R_):
        q = ((hi + lo) * F32(0.5)).astype(F32)
        behind, valid = refine_probe(q)
        for r in bracketed:
            if behind[r]:
                hi[r] = q[r]
            else:
                lo[r] = q[r]
            if not valid[r]:
                flags[r] |= 4
    for r in bracketed:
        depth[r] = (hi[r] + lo[r]) * F32(0.5)
    return depth, flags, hit


# ------------------------------------------------------------------------------------------------------------------
# inputs, network, fp64
# ------------------------------------------------------------------------------------------------------------------
def case_inputs(case):
    """(feat | feats ring, rays, cameras, prior | prior ring): view_search_ref's / view_keys_ref's, seeded by the case name."""
    return VK.case_inputs(case) if case.keys else VS.case_inputs(case)


def probe64(case, w, inputs, with_bound=False):
    """probe(q) on the fp64 chain: {logit (``fill`` at an invalid probe), z, valid, near, key, and - ``with_bound`` - tol: the derived fp32
    logit bound at a valid probe}."""
    feat, rays, cams, prior = inputs

    def probe(q):
        if case.keys:
            logit, sel, near, ch, chains = VK.step64(case, w, feat, rays, cams, prior, q)
            out = {"logit": logit.numpy(), "z": ch["z"].numpy(), "valid": (sel != NONE).numpy(), "near": near.numpy(), "key": sel.numpy().astype(np.uint8)}
            if with_bound:
                out["tol"] = VK.bound(case, w, feat, chains, sel)[1].numpy()
        else:
            logit, ch = VS.step64(case, w, feat, rays, cams, prior, q)
            out = {"logit": logit.numpy(), "z": ch["z"].numpy(), "valid": ch["valid"].numpy(), "near": ch["near"].numpy(), "key": None,
                   "uv": ch["uv"].numpy(), "prior_uv": ch["prior_uv"].numpy() if prior is not None else None}
            if with_bound:
                out["tol"] = V.view_bound(w, feat, ch, VS.prior_const(case))[1].numpy()
        return out
    return probe


def sample_table(case, w, inputs, with_bound=False):
    """Every ray at every shared sample on the fp64 chain, reached or not: per-key arrays stacked to (n_march, B, N), plus thr, behind, margin."""
    probe, rows = probe64(case, w, inputs, with_bound), []
    for q in samples(case):
        p = probe(np.full(case.shape, q, dtype=F32))
        p["thr"] = R.thresholds_at(case, p["z"].astype(F32))[0]
        rows.append(p)
    t = {k: np.stack([r[k] for r in rows]) for k in rows[0] if rows[0][k] is not None}
    t["behind"] = t["logit"] < t["thr"]
    t["margin"] = np.abs(t["logit"] - t["thr"])
    return t


def march_net(case):
    """view_search_ref.search_net's recipe on the march samples: the depth column of W1 tripled, b3 shifted by the median of (fp64 logit -
    threshold) over the valid probes of all rays at all shared samples."""
    m = R.make_net(case.cf, case.has_prior, R._seed(case.name + "march" + case.salt), depth_gain=3.0)
    t = sample_table(case, R.weights64(m), case_inputs(case))
    if t["valid"].any():
        with torch.no_grad():
            m.mlps["s0"][4].bias -= float(np.median((t["logit"] - t["thr"])[t["valid"]]))
    return m


def simulate(case, w, inputs, with_bound=False):
    """The march with the fp64 chain deciding (queries kept in fp32): (March, per-step records)."""
    return run_rule(case, probe64(case, w, inputs, with_bound))


def shares(hit, flags):
    """(bracketed, none, s* = 0) shares of the rays."""
    return float(((flags & 3) == 3).mean()), float((hit == NONE).mean()), float((hit == 0).mean())


def recross(table, hit):
    """Rays that are in front again at some shared sample after their first hit."""
    n = table["behind"].shape[0]
    after = np.arange(n).reshape(n, 1, 1) > hit.astype(np.int64)[None]
    return (hit != NONE) & (after & ~table["behind"]).any(0)


def decided_recross(case, w, inputs):
    """The rays of test (7): in front again at some shared sample after their first hit (s* >= 1), and decided beyond both bounds at every
    probe they evaluate - |logit - thr| above the derived fp32 logit bound (an invalid probe's `fill` is exact), the probe not within
    PROJ_MARGIN of a validity or prior-texel boundary, and the keyframe z not on an edge of the Thresholder table.  On the fp64 chain
    alone.  Returns (rays mask, sure mask, the simulation's March)."""
    sim, steps = simulate(case, w, inputs, with_bound=True)
    sure = np.ones(case.shape, bool)
    for st in steps:
        decided = ~st["near"] & (~st["valid"] | (np.abs(st["logit"] - st["thr"]) > st["tol"]))
        if case.table:
            decided &= np.abs(st["z"][..., None] - np.asarray(case.table[0])).min(-1) > 1e-5
        sure &= decided | ~st["active"]
    rays = recross(sample_table(case, w, inputs), sim.hit) & sure & (sim.hit >= 1) & (sim.hit != NONE)
    return rays, sure, sim


# ------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------
def device(case, m, inputs):
    """view_search_ref.Device / view_keys_ref.Device (hostile feature buffers) plus the march depths between two NaN guards."""
    dev = VK.Device(case, m, *inputs) if case.keys else VS.Device(case, m, *inputs)
    q_s = samples(case)
    dev.march_buf = torch.cat([torch.full((4,), R.NAN), torch.from_numpy(q_s), torch.full((4,), R.NAN)]).cuda()
    dev.march_ptr = dev.march_buf.data_ptr() + 16
    return dev


def run_march(L, case, dev, n_march=None, refine=None, want=(True, True, True, True), listed=None, fbuf=None):
    """One launch into prefilled outputs: (rc, depth Out, logits Out, flags ByteOut | None, hit_step ByteOut | None, points Out | None,
    key ByteOut | None); ``want`` = (flags, hit_step, points, key).  ``n_march``: only the first samples; ``listed`` / ``fbuf`` as the parents'."""
    from implicit_depth_amd import _lib

    listed = case.listed if listed is None else listed
    n = case.rays
    depth, logits = R.Out(n), R.Out(n)
    flags = S.ByteOut(n) if want[0] else None
    hit = S.ByteOut(n) if want[1] else None
    points = R.Out(3 * n) if want[2] else None
    key = S.ByteOut(n) if want[3] and case.keys else None
    c, pm = dev.cams, dev.prior
    fb = dev.fbuf if fbuf is None else fbuf
    rays = (dev.third if case.keys else dev.rays).data_ptr() if listed else None
    head = (fb.data_ptr() + 4 * dev.off, dev.cs, case.cf, case.B, case.H, case.W)
    if case.keys:
        head += (dev.stride, case.n_slots, dev.slots, case.M)
    tail = (0 if listed else case.h, 0 if listed else case.w, rays, case.N if listed else 0, c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(),
            c[3].data_ptr(), _lib.ptr(pm), c[4].data_ptr() if pm is not None else None, c[5].data_ptr() if pm is not None else None,
            int(case.has_prior), float(case.prior) if isinstance(case.prior, float) else 0.0, dev.w1p.data_ptr(), dev.w2p.data_ptr(),
            dev.vecs.data_ptr(), dev.march_ptr, case.n_march if n_march is None else n_march, case.refine if refine is None else refine,
            0.5 if case.table else case.thr, _lib.ptr(dev.bins), _lib.ptr(dev.thr_logits), 0 if dev.bins is None else dev.bins.numel(),
            float(case.fill), depth.ptr, logits.ptr, flags.ptr if flags else None, hit.ptr if hit else None, points.ptr if points else None)
    if case.keys:
        rc = L.idh_binary_mlp_view_keys_march_fwd(*head, *tail, key.ptr if key else None, _lib.stream_ptr())
    else:
        rc = L.idh_binary_mlp_view_march_fwd(*head, *tail, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, depth, logits, flags, hit, points, key


# ------------------------------------------------------------------------------------------------------------------
# the golden of the reference's own modules (tests/golden/view_march.npz, written by tests/golden/gen_golden_view_march.py)
# ------------------------------------------------------------------------------------------------------------------
GOLDEN_N_MARCH, GOLDEN_REFINE = 9, 6
GOLDEN_CASE = MarchCase(64, VS.GOLDEN_B, VS.GOLDEN_H, VS.GOLDEN_W, VS.GOLDEN_h, VS.GOLDEN_w, "moved", None, "wide", n_march=GOLDEN_N_MARCH,
                        refine=GOLDEN_REFINE)


def golden_net(cls=None):
    """ray_query_ref.golden_net with the depth column of W1 tripled and b3 shifted by ``march_net``'s recipe on the golden inputs."""
    m = Q.golden_net(cls) if cls is not None else Q.golden_net()
    feat, cams = VS.golden_inputs()
    case = GOLDEN_CASE
    with torch.no_grad():
        m.mlps["s0"][0].weight[:, 0] *= 3.0
    w = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    t = sample_table(case, w, (feat, VS.pixel_centres(case.B, case.h, case.w), cams, None))
    with torch.no_grad():
        m.mlps["s0"][4].bias -= float(np.median(t["logit"][t["valid"]]))  # thr = logit(0.5) = 0
    return m
