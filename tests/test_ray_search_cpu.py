"""idh_binary_mlp_rays_search_fwd without a GPU: every refusal and its code (all return before the device is touched, so made-up
pointers do), and - on the fp64 simulation alone - that the case table of tests/ray_search_ref.py reaches what it was written for.
The same table is executed on the device by test_ray_search_gpu.py."""
import numpy as np
import pytest

import mlp_op_ref as R
import ray_query_ref as Q
import ray_search_ref as S

OK, EINVAL, EUNSUPPORTED = R.OK, R.EINVAL, R.EUNSUPPORTED
ENTRY = "idh_binary_mlp_rays_search_fwd"


def _lib():
    from implicit_depth_amd import _lib

    return _lib.lib()


P_ = lambda i: 0x100000 * (i + 1)  # 16-byte-aligned made-up addresses: nothing is dereferenced

# the argument list in the order of include/idh.h, with values the entry point accepts
ARGS = dict(feat=P_(1), feat_cs=64, Cf=64, B=2, H=5, W=7, rays=P_(2), prior=P_(3), has_prior=1, prior_const=-1.0, N=35, grid_w=14, grid_h=10,
            w1=P_(4), w2=P_(5), vecs=P_(6), iters=12, lo=0.5, hi=8.0, threshold=0.5, bins=P_(7), thr_logits=P_(8), n_bins=4, invK=P_(9),
            wTc=P_(10), depth=P_(11), logits=P_(12), flags=P_(13), points=P_(14), stream=None)
REQUIRED = ("feat", "rays", "w1", "w2", "vecs", "depth", "logits")
ALIGNED = ("feat", "rays", "prior", "bins", "thr_logits", "invK", "wTc", "depth", "logits", "points")


def _refusals():
    """(overrides of the valid arguments, expected code).  No row may describe a call that would launch."""
    rs = []
    add = lambda code=EINVAL, **kw: rs.append((kw, code))
    # the conditions of idh_binary_mlp_rays_fwd that apply
    for kw in ({"B": -1}, {"N": -1}, {"H": 0}, {"W": 0}, {"H": -5}, {"Cf": 0}, {"Cf": -4}, {"Cf": 62}, {"feat_cs": 60}, {"grid_w": 0}, {"grid_h": 0},
               {"grid_w": -14}):
        add(**kw)
    add(B=0, code=OK)
    add(N=0, code=OK)
    add(B=0, feat=None, depth=None, code=OK)  # nothing to do: the pointers are not looked at
    add(B=1 << 10, N=1 << 21, code=EUNSUPPORTED)  # B N = 2^31
    add(B=1 << 11, H=1 << 10, W=1 << 10, code=EUNSUPPORTED)  # B H W = 2^31
    for p in REQUIRED:
        add(**{p: None})
    for p in ALIGNED:
        add(**{p: ARGS[p] + 2})
    add(flags=P_(13) + 1, B=0, code=OK)  # bytes: any alignment
    add(feat_cs=65, feat=P_(1) + 4, B=0, code=OK)  # any row stride and any 4-byte-aligned base (dword loads)
    # the search's own
    add(iters=0)
    add(iters=-2)
    add(lo=8.0, hi=8.0)
    add(lo=8.0, hi=0.5)
    add(hi=float("nan"))
    for t in (0.0, 1.0, -0.1, 1.5, float("nan")):
        add(threshold=t, n_bins=0)
    add(threshold=7.0, B=0, code=OK)  # with a table the constant is not looked at
    add(n_bins=0, bins=None, thr_logits=None, B=0, code=OK)
    add(n_bins=-1)
    add(bins=None)
    add(thr_logits=None)
    add(invK=None)  # points without invK
    add(invK=None, wTc=None)
    add(invK=None, points=None, wTc=None, B=0, code=OK)
    add(flags=None, points=None, B=0, code=OK)  # both optional outputs
    add(prior=None, B=0, code=OK)  # prior_const
    # which rule wins: argument errors, then the empty call, then the pointers, then the sizes
    add(B=0, iters=0)
    add(B=0, threshold=0.0, n_bins=0)
    add(N=0, bins=None)
    add(N=0, invK=None)
    add(B=0, rays=None, depth=None, code=OK)
    add(N=0, B=1 << 11, H=1 << 10, W=1 << 10, code=OK)
    add(feat=None, B=1 << 10, N=1 << 21)
    add(points=P_(14) + 2, B=1 << 11, H=1 << 10, W=1 << 10)
    add(hi=0.5, lo=8.0, B=1 << 10, N=1 << 21)
    add(lo=0.0, B=0, code=OK)  # hi > lo is all this entry point asks of the bracket
    add(lo=-1.0, hi=float("inf"), B=0, code=OK)
    return rs


REFUSALS = _refusals()


@pytest.mark.parametrize("row", REFUSALS, ids=lambda r: ",".join(f"{k}={v}" for k, v in r[0].items()))
def test_refusals_and_their_codes(row):
    over, code = row
    args = dict(ARGS)
    assert set(over) <= set(args), over
    args.update(over)
    assert getattr(_lib(), ENTRY)(*args.values()) == code


def test_every_pointer_is_refused_in_turn():
    nulls = {next(iter(o)) for o, c in REFUSALS if len(o) == 1 and next(iter(o.values())) is None and c == EINVAL}
    assert set(REQUIRED) | {"bins", "thr_logits", "invK"} == nulls
    odd = {k for o, c in REFUSALS if len(o) == 1 and c == EINVAL for k, v in o.items() if isinstance(v, int) and k in ALIGNED and v & 3}
    assert odd == set(ALIGNED)


def test_the_symbol_is_declared_in_header_and_binding():
    import os

    from implicit_depth_amd import _lib

    assert ENTRY in _lib.declared_symbols()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "idh.h")).read()
    assert f"int {ENTRY}(" in hdr and hasattr(_lib.lib(), ENTRY)


# ---- the table reaches what it claims (fp64 simulation only) --------------------------------------------------------------------------
_SIM = {}


def _sim(case):
    if case.name not in _SIM:
        feat, rays, prior = S.case_inputs(case)
        _SIM[case.name] = S.simulate(case, R.weights64(S.search_net(case)), feat, rays, prior)
    return _SIM[case.name]


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_case_simulation(case):
    depth, flags, steps = _sim(case)
    assert np.isfinite(depth).all() and (depth >= np.float32(case.lo)).all() and (depth <= np.float32(case.hi)).all()
    assert set(np.unique(flags)) <= {1, 2, 3}
    share = {v: float((flags == v).mean()) for v in (1, 2, 3)}
    print(f"{case.name}: flags 1 / 2 / 3 = {share[1]:.2%} / {share[2]:.2%} / {share[3]:.2%}")
    if case.B * case.N > 1:  # both bounds move somewhere among the rays
        assert (flags & 1).any() and (flags & 2).any()
    if (case.lo, case.hi) == (1.0, 3.0):
        assert R.first_query(case) == np.float32(case.lo)  # the reference's (hi - lo) / 2 start equals lo here
    if case.thr == "edge":
        assert (steps[0]["q"] == np.float32(3.75)).all() and (steps[0]["idx"] == 2).all()  # 3.75 itself is not "strictly below"
    if case.thr in ("clamp", "one"):
        assert any((s["idx"] == len(case.table[0])).any() for s in steps)  # a query beyond the last edge: the count is clamped
    if case.nonfinite:
        _, rays, _ = S.case_inputs(case)
        bad = ~np.isfinite(rays.numpy()).all(-1)
        assert bad.sum() == 2 and np.isnan(rays[0, 5, 0].item()) and (rays[case.B - 1, 7] == float("inf")).all()
        assert (Q.sample64(S.case_inputs(case)[0], S.finite_rays(rays), case.grid).permute(0, 2, 1)[bad] == 0).all()  # f = 0


def test_table_as_a_whole():
    assert [(c.cf, c.B, c.H, c.W, c.N) for c in S.CASES] == [(4, 1, 5, 7, 1), (20, 3, 5, 7, 15), (64, 1, 12, 16, 16), (64, 3, 12, 16, 37), (68, 3, 5, 7, 17),
                                                             (256, 1, 12, 16, 37), (64, 3, 5, 7, 16411)]
    assert {c.layout for c in S.CASES} == set(Q.LAYOUTS) and {c.thr for c in S.CASES} == {0.5, 0.3, "edge", "clamp", "one"}
    assert {("none" if c.prior is None else "tensor" if c.prior == "tensor" else "const") for c in S.CASES} == {"none", "tensor", "const"}
    assert sum(c.nonfinite for c in S.CASES) == 1
    big = S.CASES[-1]
    assert (big.B * big.N + 15) // 16 > Q.LAUNCHED_WAVES  # a second round of the persistent loop
    assert any(c.cf > 64 for c in S.CASES) and any(c.cf % 16 for c in S.CASES)  # W1f from global memory; a partial channel block
    seen = set()
    bracketed = 0
    for c in S.CASES:
        flags = _sim(c)[1]
        seen |= set(np.unique(flags).tolist())
        bracketed += bool((flags == 3).any())
    assert seen == {1, 2, 3}  # rays that run into lo, rays that run into hi, rays that bracket the surface
    print(f"{bracketed} of {len(S.CASES)} cases have rays that bracket the surface")
    # a ray that brackets the surface converges onto the decision boundary, so its late steps sit close to the threshold: the GPU test is
    # teacher forcing, which excludes no ray
    for c in S.CASES:
        late = np.minimum.reduce([s["margin"] for s in _sim(c)[2][6:]]) < 1e-2
        print(f"{c.name}: {late.mean():.1%} of the rays have a step after the sixth within 1e-2 of their threshold")
