"""First-hit depth in a moving camera on the GPU: idh_binary_mlp_view_march_fwd / idh_binary_mlp_view_keys_march_fwd called by hand on
hostile buffers (tests/view_march_ref.py: case table, rule, fp64 simulation, device calls), against the host composition they replace - one
idh_binary_mlp_view_fwd (idh_binary_mlp_view_keys_fwd) launch per global step on the per-ray map rendered = q with the rule in numpy fp32
between the launches -, against the fp64 chain by teacher forcing, against the reference's own modules (tests/golden/view_march.npz), and
through mlp / HotPath.query_view_first_hit(_keys) / StreamingSession.first_hit_for_view / raycast_first_hit."""
import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import view_march_ref as VM
from conftest import TOL, load_golden
from test_ray_query_gpu import _build, _frame, _fwd, _model, BUFFER
from test_view_search_gpu import _bits, _hold, _points32, _thresholder

V, VS, VK, Q, R, S = VM.V, VM.VS, VM.VK, VM.Q, VM.R, VM.S
pytestmark = pytest.mark.gpu
_CACHE = {}
F32 = np.float32


def _lib():
    from implicit_depth_amd import _lib as L

    return L.lib()


def _setup(case):
    """Inputs, network and device buffers of a case, built once and shared by the tests."""
    if case.name not in _CACHE:
        inputs = VM.case_inputs(case)
        m = VM.march_net(case)
        _CACHE[case.name] = (inputs, m, VM.device(case, m, inputs))
    return _CACHE[case.name]


def _run(case, dev, **kw):
    """One launch: {d, l, f, h, p, k} as CPU tensors of the case's shape (None where not asked for); every guard word checked."""
    rc, *outs = VM.run_march(_lib(), case, dev, **kw)
    assert rc == VM.OK
    res = {}
    for name, o in zip("dlfhpk", outs):
        if o is None:
            res[name] = None
            continue
        v, clean = o.read()
        assert clean, f"a store landed outside output {name}"
        res[name] = v.view(*case.shape, 3) if name == "p" else v.view(case.shape)
    return res


def _same(got, want, what):
    diff = _bits(got) != _bits(torch.as_tensor(want))
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.numel()} differ in bits, first at {tuple(diff.nonzero()[0].tolist())}"


def _probe(case, inputs, m, dev):
    """probe(q) of view_march_ref.run_rule: one global step as the parent commit computes it, over ALL rays.  Grid form:
    idh_binary_mlp_view_fwd (keys: idh_binary_mlp_view_keys_fwd) on the map rendered = q; ray list, whose rays no depth map expresses:
    idh_project_points_fwd + idh_binary_mlp_rays_fwd on the probes' exactly rounded world points."""
    feat, rays, cams, prior = inputs
    if case.keys:
        assert not case.listed

        def keys(q):
            rd = torch.as_tensor(q).view(case.B, 1, case.h, case.w).cuda()
            rc, lo, ko, do, _ = VK.run_keys(_lib(), case, dev, rendered=rd, outputs=(True, True, False))
            assert rc == VM.OK
            (l, c1), (k, c2), (d, c3) = lo.read(), ko.read(), do.read()
            assert c1 and c2 and c3
            k = k.view(case.shape).numpy()
            return {"logit": l.view(case.shape).numpy(), "z": d.view(case.shape).numpy(), "valid": k != VM.NONE, "key": k}
        return keys

    def single(q):
        if case.listed:
            l, z, v = VS.probe_by_points(_lib(), case, m, feat, cams, prior, _points32(rays, q, cams))
        else:
            l, z, v = VS.probe_by_view_fwd(_lib(), case, m, feat, cams, prior, q)
        return {"logit": l, "z": z, "valid": v, "key": None}
    return single


def _check_against(case, got, mc, rays, cams, what):
    _same(got["d"], mc.sd, f"{what} depth")
    _same(got["l"], mc.logit.astype(F32), f"{what} last logit")
    for name, want in (("f", mc.flags), ("h", mc.hit)) + ((("k", mc.key),) if case.keys else ()):
        assert torch.equal(got[name], torch.from_numpy(want)), f"{what}: {int((got[name] != torch.from_numpy(want)).sum())} of output {name} differ"
    _same(got["p"], _points32(rays, got["d"].numpy(), cams), f"{what} points")


# ---- 1. the host composition, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", VM.CASES + VM.KEYS_CASES, ids=lambda c: c.name)
def test_bit_identity_with_the_host_composition(case):
    """depth, last logit, flags, hit_step, key and points equal at most n_march + R single-probe launches of the parent commit's kernels
    with the rule of include/idh.h in numpy fp32 between them; rays that are done are carried with their state frozen."""
    inputs, m, dev = _setup(case)
    mc, steps = VM.run_rule(case, _probe(case, inputs, m, dev))
    got = _run(case, dev)
    _check_against(case, got, mc, inputs[1], inputs[2], case.name)
    br, none, first = VM.shares(mc.hit, mc.flags)
    tiles = np.pad(np.stack([s["active"].reshape(-1) for s in steps]), ((0, 0), (0, -case.rays % 16))).reshape(len(steps), -1, 16).any(-1)
    print(f"{case.name}: {case.rays} rays equal in bits; bracketed {br:.2f}, none {none:.2f}, s* = 0 {first:.2f}; "
          f"{len(steps)} global steps, {tiles.sum(0).mean():.2f} per tile")
    if case in VM.SMALL:  # the margin rule on the kernel's own queries: per step at most NEAR_CAP of the probes evaluated lie inside the margin
        p64 = VM.probe64(case, R.weights64(m), inputs)
        for st in steps:
            near = p64(st["q"])["near"] & st["active"]
            assert near.sum() <= VM.NEAR_CAP * st["active"].sum(), (case.name, st["it"], int(near.sum()), int(st["active"].sum()))
    again = _run(case, dev)  # a second launch gives the same bits
    for k in got:
        assert (got[k] is None and again[k] is None) or torch.equal(_bits(got[k]), _bits(again[k])), k
    q_s = VM.samples(case)
    if getattr(case, "camera", None) == "behind":
        assert (mc.flags == 6).all() and (mc.hit == VM.NONE).all() and (got["d"].numpy() == q_s[-1]).all() and (got["l"].numpy() == F32(case.fill)).all()
    if case.refine == 0:
        hb = mc.hit[(mc.flags & 3) == 3].astype(int)
        assert len(hb) and (got["d"].numpy()[(mc.flags & 3) == 3] == ((q_s[hb] + q_s[hb - 1]) * F32(0.5)).astype(F32)).all()  # the bracket's midpoint


# ---- 2. teacher forcing -----------------------------------------------------------------------------------------------------------
FORCED = [VM.A, VM.B, VM.A_NEG, VM.CASES[3], VM.LISTED, VM.CASES[10], VM.KEYS_CASES[0], VM.KEYS_CASES[3]]


@pytest.mark.parametrize("case", FORCED, ids=lambda c: c.name)
def test_march_by_teacher_forcing(case):
    """Runs with n_march = 1 .. n (R = 0) and R = 1 .. R expose every logit the full run evaluates: in each of them some rays' LAST probe is
    new.  (a) that logit lies within the derived bound of the fp64 chain at the kernel's own query, and is `fill`, exactly, at an invalid
    probe (probes within PROJ_MARGIN of a boundary left out: test_bit_identity_with_the_host_composition caps their share per step); (b) every output of every run is
    bitwise the fp32 rule replayed on the kernel's own logits, with the keyframe z, validity and key the parent's dense kernel gives."""
    inputs, m, dev = _setup(case)
    w = R.weights64(m)
    probe32, p64 = _probe(case, inputs, m, dev), VM.probe64(case, w, inputs, with_bound=True)
    n, Rr, sh = case.n_march, case.refine, case.shape
    q_s = VM.samples(case)
    fill = F32(case.fill)
    names = ("logit", "z", "valid", "key")
    store = {("m", s): None for s in range(n)}  # probe identity -> {known, logit, z, valid, key}
    store.update({("r", j): None for j in range(Rr)})
    for key in store:
        store[key] = {"known": np.zeros(sh, bool), "logit": np.zeros(sh, F32), "z": np.ones(sh, F32), "valid": np.zeros(sh, bool), "key": np.full(sh, VM.NONE, np.uint8)}
    worst, checked = 0.0, 0

    def replay(nm, rf, fresh=None):
        """The rule on the stored probes; a ray whose next probe is not stored yet takes it from ``fresh`` - or, without ``fresh``, is
        stopped there and its query returned."""
        mc = VM.March(case, q_s[:nm], rf)
        q_new, new = np.zeros(sh, F32), np.zeros(sh, bool)
        while mc.more():
            q, a, marching = mc.queries(), mc.active, mc.st < 0
            cur = {k: np.zeros(sh, store[("m", 0)][k].dtype) for k in names + ("known",)}
            for ident, mask in [(("m", min(mc.it, nm - 1)), marching)] + [(("r", j), ~marching & (rf - mc.st == j)) for j in range(rf)]:
                for k in cur:
                    cur[k] = np.where(mask, store[ident][k], cur[k])
            cur["z"] = np.where(a, cur["z"], F32(1.0))
            need = a & ~cur["known"]
            idents = [(("m", min(mc.it, nm - 1)), marching)] + [(("r", j), ~marching & (rf - mc.st == j)) for j in range(rf)]
            if need.any():
                assert not (new & need).any(), "a ray has two new probes in one run"
                q_new, new = np.where(need, q, q_new).astype(F32), new | need
                if fresh is not None:
                    for ident, mask in idents:
                        take = need & mask
                        for k in names:
                            if fresh[k] is not None:
                                store[ident][k] = np.where(take, fresh[k], store[ident][k])
                        store[ident]["known"] |= take
                    for k in names:
                        if fresh[k] is not None:
                            cur[k] = np.where(need, fresh[k], cur[k])
            thr, _ = R.thresholds_at(case, cur["z"].astype(F32))
            mc.update(cur["logit"], thr, cur["valid"], cur["key"] if case.keys else None)
            if fresh is None:
                mc.st = np.where(need, 0, mc.st)  # the collecting pass stops the ray at its new probe, whatever it would answer
            else:
                assert (mc.st[need] == 0).all(), "a new probe is not the ray's last"
        return mc, q_new, new

    for nm, rf in [(k, 0) for k in range(1, n + 1)] + [(n, r) for r in range(1, Rr + 1)]:
        got = _run(case, dev, n_march=nm, refine=rf, want=(True, True, False, True))
        _, q_new, new = replay(nm, rf)
        assert new.any() or nm > 1
        if new.any():
            q = np.where(new, q_new, got["d"].numpy()).astype(F32)  # the other rays ride along at their own final depth
            p32, ref = probe32(q), p64(q)
            l32 = got["l"].numpy()
            keep = new & ~ref["near"]
            assert (p32["valid"][keep] == ref["valid"][keep]).all()
            if case.keys:
                assert (p32["key"][keep] == ref["key"][keep]).all()
            on, off = keep & ref["valid"], keep & ~ref["valid"]
            assert (l32[off] == fill).all(), f"{case.name} ({nm}, {rf}): an invalid probe's logit is not fill"
            assert (l32[new & ~p32["valid"]] == fill).all()
            if on.any():
                ratio = np.abs(l32.astype(np.float64) - ref["logit"])[on] / ref["tol"][on]
                worst, checked = max(worst, float(ratio.max())), checked + int(on.sum())
                assert (ratio <= 1).all(), f"{case.name} ({nm}, {rf}): {int((ratio > 1).sum())} logits exceed the bound, worst err / bound {ratio.max():.3g}"
            fresh = {"logit": l32, "z": p32["z"], "valid": p32["valid"], "key": p32["key"]}
        else:
            fresh = None
        mc, _, _ = replay(nm, rf, fresh)
        _same(got["d"], mc.sd, f"{case.name} ({nm}, {rf}) depth")
        _same(got["l"], mc.logit.astype(F32), f"{case.name} ({nm}, {rf}) last logit")
        assert np.array_equal(got["f"].numpy(), mc.flags) and np.array_equal(got["h"].numpy(), mc.hit), f"{case.name} ({nm}, {rf}): flags or hit_step differ"
        if case.keys:
            assert np.array_equal(got["k"].numpy(), mc.key)
        d = got["d"].numpy()
        assert (d >= q_s[0]).all() and (d <= q_s[nm - 1]).all()
    print(f"{case.name}: worst err / bound {worst:.4f} over {checked} logits in {n + Rr} runs")
    assert checked > 0 or getattr(case, "camera", None) == "behind"


# ---- 3. list form == grid form, M = 1 == single key ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [VM.A, VM.B, VM.CASES[5], VM.KEYS_CASES[0], VM.KEYS_CASES[3]], ids=lambda c: c.name)
def test_list_form_at_pixel_centres_is_the_grid_form(case):
    inputs, m, dev = _setup(case)
    grid, listed = _run(case, dev), _run(case, dev, listed=True)
    for k in grid:
        assert (grid[k] is None and listed[k] is None) or torch.equal(_bits(grid[k]), _bits(listed[k])), k


def test_one_key_is_the_single_key_entry_point():
    case = next(c for c in VM.KEYS_CASES if c.M == 1)
    (feats, rays, cams, prior), m, dev = _setup(case)
    slot = case.slots[0]
    block = VK._Block(case)
    block.keys = False
    one = VS.Device(block, m, feats[slot], rays, VK.key_cams(cams, slot), None if prior is None else prior[slot])
    one.march_ptr = dev.march_ptr
    a, b = _run(case, dev), _run(block, one)
    for k in "dlfhp":
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert bool(((a["k"] == 0) | (a["k"] == VM.NONE)).all()) and bool((a["k"] == 0).any())


# ---- 4. / 5. world points, optional outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [VM.A, VM.B, VM.LISTED, VM.KEYS_CASES[0]], ids=lambda c: c.name)
def test_points_and_optional_outputs(case):
    """World points within the derived bound of ray_search_ref.points_reference at the kernel's own depth - and bitwise the exactly rounded
    expression; optional outputs passed as NULL change nothing else, and every output's guard words survive (checked by every read)."""
    inputs, m, dev = _setup(case)
    rays, cams = inputs[1], inputs[2]
    got = _run(case, dev)
    ref, tol = VS.points_reference(rays, got["d"], cams)
    _hold(got["p"], ref, tol, f"{case.name} world points")
    assert torch.equal(_bits(got["p"]), _bits(_points32(rays, got["d"].numpy(), cams)))
    back = torch.linalg.inv(cams[1].double())  # the live camera's z of the point is the depth
    zc = (got["p"].double() @ back[:, :3, :3].transpose(1, 2) + back[:, None, :3, 3])[..., 2]
    assert (zc - got["d"].double()).abs().max().item() < 1e-4
    for want in ((False, True, True, True), (True, False, True, False), (True, True, False, True), (False, False, False, False)):
        g2 = _run(case, dev, want=want)
        assert [g2[k] is None for k in "fhp"] == [not x for x in want[:3]] and (g2["k"] is None) == (not (want[3] and case.keys))
        for k in got:
            assert g2[k] is None or torch.equal(_bits(g2[k]), _bits(got[k])), (want, k)


# ---- 6. probes a ray never reaches read nothing -----------------------------------------------------------------------------------
def test_unreached_probes_read_nothing():
    """Case A with fill < 0 (most rays are done after one or two samples): every feature row and prior texel that only the shared samples
    AFTER a ray's first hit would touch is NaN, and every bit stays the same.  The poisoned set is a SUBSET of those rows and texels: the
    footprints are taken from the fp64 chain, whose floor / round can differ from the fp32 chain's next to an integer, so whatever lies
    within one texel of an evaluated probe's footprint is left alone."""
    case = VM.A_NEG
    inputs, m, dev = _setup(case)
    feat, rays, cams, prior = inputs
    w = R.weights64(m)
    mc, steps = VM.run_rule(case, _probe(case, inputs, m, dev))
    got = _run(case, dev)
    _check_against(case, got, mc, rays, cams, case.name)
    assert (mc.hit <= 1).mean() > 0.5
    p64 = VM.probe64(case, w, inputs)
    B, H, W = case.B, case.H, case.W
    bi = np.arange(B).reshape(B, 1) * np.ones(case.shape, np.int64)

    def texels(uv, mask, reach):
        """Texels (b, y, x) within ``reach`` of the bilinear corners (reach = 0: exactly the four) or of the nearest texel of the points uv[mask]."""
        hits = np.zeros((B, H, W), bool)
        x0, y0 = np.floor(uv[..., 0] - 0.5).astype(np.int64), np.floor(uv[..., 1] - 0.5).astype(np.int64)
        for dy in range(-reach, reach + 2):
            for dx in range(-reach, reach + 2):
                y, x = y0 + dy, x0 + dx
                ok = mask & (y >= 0) & (y < H) & (x >= 0) & (x < W)
                hits[bi[ok], y[ok], x[ok]] = True
        return hits

    touched_f, touched_p = np.zeros((B, H, W), bool), np.zeros((B, H, W), bool)
    for st in steps:  # every evaluated probe, valid or not, with a texel to spare on each side
        ch = p64(st["q"])
        touched_f |= texels(ch["uv"], st["active"], 1)
        touched_p |= texels(ch["prior_uv"], st["active"], 1)
    later_f, later_p = np.zeros((B, H, W), bool), np.zeros((B, H, W), bool)
    for s, q in enumerate(VM.samples(case)):
        ch = p64(np.full(case.shape, q, dtype=F32))
        after = (mc.hit != VM.NONE) & (s > mc.hit.astype(int)) & ch["valid"]
        later_f |= texels(ch["uv"], after, 0)
        later_p |= texels(ch["prior_uv"], after, 0)
    pf, pp = later_f & ~touched_f, later_p & ~touched_p
    print(f"{case.name}: {int(pf.sum())} feature rows and {int(pp.sum())} prior texels are reached only by probes after a first hit")
    assert pf.sum() > 8 and pp.sum() > 0
    feat2, prior2 = feat.clone(), prior.clone()
    feat2.permute(0, 2, 3, 1)[torch.from_numpy(pf)] = R.NAN
    prior2[:, 0][torch.from_numpy(pp)] = R.NAN
    dev2 = VM.device(case, m, (feat2, rays, cams, prior2))
    poisoned = _run(case, dev2)
    for k in got:
        assert poisoned[k] is None or torch.equal(_bits(poisoned[k]), _bits(got[k])), f"output {k} changed: an unreached probe was read"
    # the poison is in reach: with every row NaN the valid last probes turn NaN
    dev3 = VM.device(case, m, (torch.full_like(feat, R.NAN), rays, cams, prior))
    assert bool(torch.isnan(_run(case, dev3)["l"]).any())


def test_keys_read_nothing_from_a_key_no_evaluated_probe_selected():
    case = VM.KEYS_CASES[3]
    inputs, m, dev = _setup(case)
    feats, rays, cams, prior = inputs
    mc, steps = VM.run_rule(case, _probe(case, inputs, m, dev))
    got = _run(case, dev)
    _check_against(case, got, mc, rays, cams, case.name)
    for pos in range(case.M):
        slot = case.slots[pos]
        f2 = feats.clone()
        f2[slot] = R.NAN
        buf = VK.ring_buffer(case, f2)[0].cuda()
        keep = dev.prior
        if keep is not None:
            dev.prior = keep.clone()
            dev.prior[slot] = R.NAN
        try:
            g2 = _run(case, dev, fbuf=buf)
        finally:
            dev.prior = keep
        never = torch.from_numpy(~np.stack([s["active"] & (s["key"] == pos) for s in steps]).any(0))
        assert bool(never.any()) and bool((~never).any())
        for k in "dlfhk":
            assert torch.equal(_bits(got[k])[never], _bits(g2[k])[never]), f"{case.name}: a ray that never selected key {pos} read it ({k})"


# ---- 7. what bisection cannot -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [VM.A, VM.B], ids=lambda c: c.name)
def test_first_crossing_on_rays_that_cross_again(case):
    """The rays the fp64 simulation marks as in front again at some shared sample after their first hit, and as decided beyond both bounds at
    every probe they evaluate - |logit - thr| above the derived fp32 logit bound, and the probe not within PROJ_MARGIN of a validity or
    prior-texel boundary -: the kernel's hit_step is the simulation's and its depth lies inside [q_{s*-1}, q_{s*}].  The share of those rays
    on which the bisection of idh_binary_mlp_view_search_fwd over [lo, hi] lands outside that interval is recorded, not asserted."""
    inputs, m, dev = _setup(case)
    rays, sure, sim = VM.decided_recross(case, R.weights64(m), inputs)
    got = _run(case, dev)
    q_s, d, h = VM.samples(case), got["d"].numpy(), got["h"].numpy()
    assert rays.sum() >= VM.MIN_DECIDED_RECROSS * case.rays, (case.name, int(rays.sum()))  # (tests/test_view_march_cpu.py asserts it too)
    assert (h[rays] == sim.hit[rays]).all()
    s = sim.hit[rays].astype(int)
    assert ((d[rays] >= q_s[s - 1]) & (d[rays] <= q_s[s])).all()
    assert (d[sure] == sim.sd[sure]).all() and (got["f"].numpy()[sure] == sim.flags[sure]).all()  # and every ray decided beyond the bounds follows the simulation
    rc, bd, *_ = VS.run_view_search(_lib(), case, dev, want_flags=False, want_points=False)
    assert rc == VM.OK
    b = bd.read()[0].view(case.shape).numpy()
    outside = (b[rays] < q_s[s - 1]) | (b[rays] > q_s[s])
    print(f"{case.name}: {int(rays.sum())} of {case.rays} rays cross again and are decided beyond the bounds; the march returns the first crossing on all "
          f"of them, the {case.iters}-step bisection over [{case.lo}, {case.hi}] lands outside its bracket on {outside.mean():.2%}")


# ---- 9. the reference's own modules -------------------------------------------------------------------------------------------------
def test_march_reproduces_the_references_modules():
    """tests/golden/view_march.npz: hit_step and depth equal on every ray whose smallest |logit - thr| along its evaluated probes exceeds
    the logit tolerance of view_search.npz's test (scale-relative TOL)."""
    g = load_golden("view_march")
    case = VM.GOLDEN_CASE
    feat, cams = VS.golden_inputs()
    m = VM.golden_net()
    rays = VS.pixel_centres(case.B, case.h, case.w)
    assert np.array_equal(g["samples"], VM.samples(case))
    dev = VM.device(case, m, (feat, rays, cams, None))
    got = _run(case, dev)
    sure = torch.from_numpy(g["march_margin"]).view(case.shape) > TOL * float(g["logit_scale"])
    same_d = got["d"] == torch.from_numpy(g["march_depths"]).view(case.shape)
    same_h = got["h"] == torch.from_numpy(g["hit_step"]).view(case.shape)
    print(f"golden: {same_d.float().mean().item():.2%} of the depths and {same_h.float().mean().item():.2%} of the hit steps equal, "
          f"{sure.float().mean().item():.2%} of the rays qualify")
    assert sure.float().mean().item() > 0.5 and bool(same_d[sure].all()) and bool(same_h[sure].all())
    assert len(torch.unique(got["h"])) > 3


# ---- 8. the public API --------------------------------------------------------------------------------------------------------------
def _compose_public(query_view, B, size, th, q_s, refine):
    """What a caller had at the parent commit: one dense occlusion query per global step on rendered = q with the rule in torch between
    them.  ``query_view(rendered)`` -> the dictionary of HotPath.query_view (plus "view_key" for the ring)."""
    h, w = size
    sh = (B, 1, h, w)
    q_s = torch.as_tensor(q_s).cuda()
    n = q_s.numel()
    st = torch.full(sh, -1, dtype=torch.long, device="cuda")
    lo, hi, sd, logit = (torch.zeros(sh, device="cuda") for _ in range(4))
    flags = torch.zeros(sh, dtype=torch.uint8, device="cuda")
    hit, key = (torch.full(sh, 255, dtype=torch.uint8, device="cuda") for _ in range(2))
    if th is not None:
        bins = th.bins.cuda().float()
        tl = torch.log(th.thresholds.cuda().float() / (1 - th.thresholds.cuda().float()))
    calls = 0
    for it in range(n + refine):
        a = st != 0
        if not bool(a.any()):
            break
        marching = st < 0
        q = torch.where(marching, q_s[min(it, n - 1)], sd)
        v = query_view(q)
        calls += 1
        l, z = v["view_pred"], v["view_depth"]
        t = tl[(bins.view(1, 1, 1, 1, -1) < z.unsqueeze(-1)).sum(-1).clamp(max=bins.numel() - 1)] if th is not None else torch.zeros_like(q)
        behind = l < t
        nhi, nlo = torch.where(behind, q, hi), torch.where(behind, lo, q)
        bracket = marching & behind & (it > 0)
        nst = torch.where(marching, torch.where(behind, torch.full_like(st, refine if it > 0 else 0), torch.full_like(st, 0 if it == n - 1 else -1)), st - 1)
        nsd = torch.where(bracket | ~marching, (nhi + nlo) * 0.5, q)
        flags = torch.where(a, flags | (torch.where(behind, 1, 2) | torch.where(v["view_valid"], 0, 4)).to(torch.uint8), flags)
        hit = torch.where(a & marching & behind, torch.full_like(hit, it), hit)
        logit = torch.where(a, l, logit)
        if "view_key" in v:
            key = torch.where(a, v["view_key"], key)
        hi, lo, sd, st = (torch.where(a, x, y) for x, y in ((nhi, hi), (nlo, lo), (nsd, sd), (nst, st)))
    return {"view_march_depths": sd, "view_march_logits": logit, "view_march_flags": flags, "view_march_hit_step": hit, "view_march_key": key}, calls


def _equal_public(got, want, B, h, w):
    for k in ("view_march_depths", "view_march_logits", "view_march_flags", "view_march_hit_step") + (("view_march_key",) if "view_march_key" in got else ()):
        assert got[k].shape == (B, 1, h, w) and torch.equal(got[k], want[k]), k
    assert got["view_march_points"].shape == (B, 1, h, w, 3)


@pytest.mark.parametrize("thr", [False, True])
def test_query_view_first_hit_is_the_composition(thr):
    from implicit_depth_amd import mlp
    from implicit_depth_amd._lib import IdhError

    B, K, H, W, D = 2, 2, 16, 24, 16
    model, d, pyr, rd = _build(B, K, H, W, D, 1, use_prior=True)
    Hs, Ws, h, w = 2 * H, 2 * W, 15, 20
    iK, wTc, cTw, K0, pcTw, _ = (t.cuda() for t in V.cameras("moved", B, Hs, Ws, h, w))
    prior_pred = torch.sigmoid(syn.randn((B, 1, Hs, Ws), 8, "pp")).cuda()
    with pytest.raises(IdhError, match="no forward"):
        model.query_view_first_hit(iK, wTc, cTw, K0, size=(h, w))
    _fwd(model, d, pyr, rendered_depth=rd)
    th = _thresholder() if thr else None
    fill, n, refine = 4.5, 9, 5
    q_s = mlp.march_samples(n, 0.5, 8.0)
    for pi in (None, {"prior_prediction": prior_pred, "prior_cam_T_world": pcTw}):
        got = model.query_view_first_hit(iK, wTc, cTw, K0, size=(h, w), prior_inputs=pi, thresholder=th, fill=fill, samples=n, refine=refine,
                                         return_points=True)
        assert set(got) == {"view_march_depths", "view_march_logits", "view_march_flags", "view_march_hit_step", "view_march_points"}
        want, calls = _compose_public(lambda r: model.query_view(r, iK, wTc, cTw, K0, prior_inputs=pi, fill=fill), B, (h, w), th, q_s, refine)
        _equal_public(got, want, B, h, w)
        fl, hs = got["view_march_flags"], got["view_march_hit_step"]
        print(f"prior {'map' if pi else 'const'}, thresholder {thr}: {calls} calls composed; flags " + " ".join(f"{v}:{(fl == v).float().mean().item():.2f}" for v in range(1, 8)))
        assert bool(((hs == 255) == ((fl & 3) == 2)).all()) and bool(((hs == 0) == ((fl & 3) == 1)).all())
        # the samples as a tensor, and the list form at the pixel centres, give the same bits
        again = model.query_view_first_hit(iK, wTc, cTw, K0, size=(h, w), prior_inputs=pi, thresholder=th, fill=fill, samples=q_s.cuda(), refine=refine,
                                           return_points=True)
        lst = model.query_view_first_hit(iK, wTc, cTw, K0, rays=VS.pixel_centres(B, h, w).cuda(), prior_inputs=pi, thresholder=th, fill=fill, samples=n,
                                         refine=refine, return_points=True)
        for k in got:
            assert torch.equal(again[k], got[k]) and torch.equal(lst[k].reshape(-1), got[k].reshape(-1)), k
        assert lst["view_march_depths"].shape == (B, h * w) and lst["view_march_points"].shape == (B, h * w, 3)
        rays = (torch.rand((B, 45, 2), generator=torch.Generator().manual_seed(5)) * torch.tensor([w + 8.0, h + 8.0]) - 4.0).cuda()
        off = model.query_view_first_hit(iK, wTc, cTw, K0, rays=rays, prior_inputs=pi, thresholder=th, fill=fill, samples=n, refine=refine, return_points=True)
        ref, tol = S.points_reference(rays.cpu(), off["view_march_depths"].cpu(), iK.cpu(), wTc.cpu())
        _hold(off["view_march_points"], ref, tol, "query_view_first_hit world points at off-centre rays")
        assert model.query_view_first_hit(iK, wTc, cTw, K0, rays=rays, samples=n, refine=refine)["view_march_points"] is None
    inv = mlp.march_samples(7, 0.5, 8.0, "inverse")
    got = model.query_view_first_hit(iK, wTc, cTw, K0, size=(h, w), fill=-2.0, samples=7, spacing="inverse", refine=0, return_points=True)
    want, _ = _compose_public(lambda r: model.query_view(r, iK, wTc, cTw, K0, fill=-2.0), B, (h, w), None, inv, 0)
    _equal_public(got, want, B, h, w)
    with pytest.raises(IdhError, match="strictly increasing"):
        model.query_view_first_hit(iK, wTc, cTw, K0, size=(h, w), samples=torch.tensor([1.0, 1.0]).cuda())
    with pytest.raises(IdhError, match="batch size"):
        model.query_view_first_hit(iK[:1], wTc[:1], cTw[:1], K0[:1], size=(h, w))
    model.binary_mlp.mlp_math = "f16x3"
    with pytest.raises(IdhError, match="fp32 only"):
        model.query_view_first_hit(iK, wTc, cTw, K0, size=(h, w))


@pytest.mark.parametrize("use_prior", [False, True])
def test_query_view_first_hit_keys_is_the_composition(use_prior):
    from implicit_depth_amd import mlp

    B, K, H, W, D = 2, 2, 16, 24, 16
    model, d0, pyr0, rd = _build(B, K, H, W, D, 1, use_prior=use_prior)
    Hs, Ws, h, w = 2 * H, 2 * W, 15, 20
    case = VK.KeysCase(64, B, Hs, Ws, 1, h, w, None, "wide")
    iK, wTc, cTw_ring, K_ring, pcTw_ring, _ = (t.cuda() for t in VK.cameras(case))
    for s in range(3):  # three forwards on different inputs, each remembered with its own camera (and prior)
        d = {k: v.cuda() for k, v in syn.cost_volume_inputs(B, K, 16, H, W, seed=s, behind_view=K - 1).items()}
        _fwd(model, d, [t.cuda() for t in syn.encoder_pyramid(B, H * 4, W * 4, seed=s)], rendered_depth=rd)
        pi = None
        if use_prior:
            pi = {"prior_prediction": torch.sigmoid(syn.randn((B, 1, Hs, Ws), 8 + s, "pp")).cuda(), "prior_cam_T_world": pcTw_ring[s]}
        model.remember(cTw_ring[s], K_ring[s], prior_inputs=pi, capacity=4)
    th, fill, n, refine = _thresholder(), 4.5, 8, 4
    q_s = mlp.march_samples(n, 0.5, 8.0)
    for order in (None, [0, 2, 1], [1]):
        got = model.query_view_first_hit_keys(iK, wTc, size=(h, w), order=order, thresholder=th, fill=fill, samples=n, refine=refine, return_points=True)
        assert set(got) == {"view_march_depths", "view_march_logits", "view_march_flags", "view_march_hit_step", "view_march_points", "view_march_key"}
        want, _ = _compose_public(lambda r: model.query_view_keys(r, iK, wTc, order=order, fill=fill), B, (h, w), th, q_s, refine)
        _equal_public(got, want, B, h, w)
        lst = model.query_view_first_hit_keys(iK, wTc, rays=VS.pixel_centres(B, h, w).cuda(), order=order, thresholder=th, fill=fill, samples=n,
                                              refine=refine, return_points=True)
        for k in got:
            assert torch.equal(lst[k].reshape(-1), got[k].reshape(-1)), k
    one = model.query_view_first_hit_keys(iK, wTc, size=(h, w), order=[1], thresholder=th, fill=fill, samples=n, refine=refine)
    assert bool(((one["view_march_key"] == 0) | (one["view_march_key"] == 255)).all())


@pytest.mark.parametrize("use_prior", [False, True])
def test_streaming_first_hit_on_a_frame_between_keyframes(use_prior):
    """On a frame where step() returned None the session answers in the LIVE camera with the bits of the composition of its own
    occlusion_for_view calls (with use_prior: the carried prior, sampled per probe); raycast_first_hit at the pixel centres is
    first_hit_for_view."""
    from implicit_depth_amd import mlp
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import StreamingSession

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    session = StreamingSession(_model("mlp", 3, use_prior=use_prior), buffer_size=BUFFER)
    h, w = 30, 40
    invK = torch.linalg.inv(syn.intrinsics(w, h)).float()
    invK[:2, :3] *= 2.0  # a lens half as long as the keyframe's: the border of the live image looks past the keyframe's
    invK = invK.cuda()
    with pytest.raises(IdhError, match="no prediction"):
        session.first_hit_for_view(poses[0], invK, (h, w))
    with pytest.raises(IdhError, match="no prediction"):
        session.raycast_first_hit(VS.pixel_centres(1, h, w).cuda(), poses[0], invK)
    key, done = None, False
    n, refine, fill, th = 9, 4, 6.0, _thresholder()
    q_s = mlp.march_samples(n, 0.5, 8.0)
    for t in range(12):
        if not np.isfinite(poses[t]).all():
            break
        frame = _frame(t, poses)
        out, code = session.step(frame, world_T_cam=poses[t], dist_to_last_valid=dists[t])
        if out is not None:
            key = frame
            continue
        if key is None:
            continue
        got = session.first_hit_for_view(poses[t], invK, (h, w), thresholder=th, fill=fill, samples=n, refine=refine)
        want, calls = _compose_public(lambda r: session.occlusion_for_view(r, poses[t], invK, fill=fill), 1, (h, w), th, q_s, refine)
        _equal_public(got, want, 1, h, w)
        assert "view_march_key" not in got and bool(torch.isfinite(got["view_march_points"]).all())
        fl = got["view_march_flags"]
        print(f"frame {t}: {calls} calls composed; flags " + " ".join(f"{v}:{(fl == v).float().mean().item():.2f}" for v in range(1, 8)))
        live = torch.from_numpy(poses[t].astype(np.float32))[None]
        ref, tol = S.points_reference(VS.pixel_centres(1, h, w), got["view_march_depths"].view(1, -1).cpu(), invK[None].cpu(), live)
        _hold(got["view_march_points"].view(1, -1, 3), ref, tol, f"first_hit_for_view world points (frame {t})")
        cast = session.raycast_first_hit(VS.pixel_centres(1, h, w).cuda(), poses[t], invK, thresholder=th, fill=fill, samples=n, refine=refine)
        for k in got:
            assert torch.equal(cast[k].reshape(-1), got[k].reshape(-1)), k
        if use_prior:  # the prior path is taken: the constant -1 gives other logits
            assert session._prior is not None
            const = session.hot.query_view_first_hit(invK[None], live.cuda(), key["cam_T_world_b44"], key["K_s0_b44"], size=(h, w), thresholder=th,
                                                     fill=fill, samples=n, refine=refine)
            assert not torch.equal(const["view_march_logits"], got["view_march_logits"])
        done = True
        break
    assert done, "the sequence has no frame between keyframes after the first prediction"


def test_streaming_first_hit_asks_three_keyframes():
    """The pan of test_view_keys_gpu.py: on frame 6, where step() returned None, the session with query_keyframes = 3 answers
    first_hit_for_view / raycast_first_hit with the bits of the composition of its own occlusion_for_view calls, which ask the three
    remembered predictions nearest pose first."""
    from implicit_depth_amd import mlp
    from implicit_depth_amd.streaming import StreamingSession

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    multi = StreamingSession(_model("mlp", 3), buffer_size=BUFFER, query_keyframes=3)
    h, w, n, refine, fill = 30, 40, 9, 4, 6.0
    invK = torch.linalg.inv(syn.intrinsics(w, h)).float()
    invK[:2, :3] *= 2.0
    invK = invK.cuda()
    predicted = 0
    for t in range(7):
        out, code = multi.step(_frame(t, poses), world_T_cam=poses[t], dist_to_last_valid=dists[t])
        predicted += out is not None
    assert out is None and predicted >= 3
    live = poses[6]
    th = _thresholder()
    got = multi.first_hit_for_view(live, invK, (h, w), thresholder=th, fill=fill, samples=n, refine=refine)
    want, calls = _compose_public(lambda r: multi.occlusion_for_view(r, live, invK, fill=fill), 1, (h, w), th, mlp.march_samples(n, 0.5, 8.0), refine)
    _equal_public(got, want, 1, h, w)
    key = got["view_march_key"]
    print(f"{calls} calls composed; key shares " + " ".join(f"{(key == i).float().mean().item():.3f}" for i in range(3)) +
          f", none {(key == 255).float().mean().item():.3f}")
    assert len(torch.unique(key)) >= 3
    cast = multi.raycast_first_hit(VS.pixel_centres(1, h, w).cuda(), live, invK, thresholder=th, fill=fill, samples=n, refine=refine)
    for k in got:
        assert torch.equal(cast[k].reshape(-1), got[k].reshape(-1)), k
