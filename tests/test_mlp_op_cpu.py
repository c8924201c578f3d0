"""The nine C entry points of csrc/mlp.hip without a GPU: every refusal and its code (all of them return before the device is
touched, so made-up pointers do), the two size queries, and - on the fp64 reference alone - that the case tables of
tests/mlp_op_ref.py reach what they were written for and that the derived logit bound tells a wrong kernel from a right one.
The same tables are executed on the device by test_mlp_op_gpu.py."""
import numpy as np
import pytest
import torch

import mlp_op_ref as R
from oracle import networks as onet

OK, EINVAL, EUNSUPPORTED = R.OK, R.EINVAL, R.EUNSUPPORTED


def _lib():
    from implicit_depth_amd import _lib

    return _lib.lib()


P_ = lambda i: 0x100000 * (i + 1)  # 16-byte-aligned made-up addresses: nothing is dereferenced

# argument lists in the order of include/idh.h, with values every entry point accepts
LOGIT_ARGS = dict(feat=P_(1), feat_cs=64, Cf=64, depth=P_(2), prior=P_(3), has_prior=1, prior_const=-1.0, w1=P_(4), w2=P_(5), vecs=P_(6),
                  B=2, P=3, HW=35, out=P_(7), stream=None)
STRIDED_ARGS = dict(feat=P_(1), bs=66 * 35, ps=1, chs=35, Cf=64, depth=P_(2), prior=P_(3), has_prior=1, prior_const=-1.0, w1=P_(4), w2=P_(5),
                    vecs=P_(6), B=2, P=3, HW=35, out=P_(7), stream=None)
SEARCH_HEAD = dict(feat=P_(1), feat_cs=64, Cf=64, prior=P_(3), has_prior=1, prior_const=-1.0, w1=P_(4), w2=P_(5), vecs=P_(6), B=2, HW=35,
                   iters=12, lo=0.5, hi=8.0)
SEARCH_TAIL = dict(sd=P_(8), logits=P_(9), stream=None)
ENTRIES = {
    "idh_binary_mlp_fwd": LOGIT_ARGS,
    "idh_binary_mlp_f16x3_fwd": LOGIT_ARGS,
    "idh_binary_mlp_strided_fwd": STRIDED_ARGS,
    "idh_binary_mlp_search_fwd": {**SEARCH_HEAD, "threshold": 0.5, **SEARCH_TAIL},
    "idh_binary_mlp_search_thr_fwd": {**SEARCH_HEAD, "bins": P_(10), "thr_logits": P_(11), "n_bins": 4, **SEARCH_TAIL},
    "idh_binary_mlp_search_f16x3_fwd": {**SEARCH_HEAD, "threshold": 0.5, "bins": P_(10), "thr_logits": P_(11), "n_bins": 4, **SEARCH_TAIL},
    "idh_sample_prior_fwd": dict(depth=P_(1), prior=P_(2), Q=1, cur=P_(3), pcw=P_(4), K=P_(5), invK=P_(6), B=2, P=3, H=5, W=7, out=P_(7), stream=None),
    "idh_pack_mlp_weight": dict(w=P_(1), dst=P_(2), ld=66, col0=1, n_in=64, stream=None),
    "idh_pack_mlp_weight_f16": dict(w=P_(1), dst=P_(2), ld=66, col0=1, n_in=64, stream=None),
}
LOGIT = ("idh_binary_mlp_fwd", "idh_binary_mlp_f16x3_fwd", "idh_binary_mlp_strided_fwd")
SEARCH = ("idh_binary_mlp_search_fwd", "idh_binary_mlp_search_thr_fwd", "idh_binary_mlp_search_f16x3_fwd")
ROWS = ("idh_binary_mlp_fwd", "idh_binary_mlp_f16x3_fwd") + SEARCH  # the row-based entry points
ALIGNED16 = ROWS[1:]  # the four that read rows with dwordx4 loads only
PACKERS = ("idh_pack_mlp_weight", "idh_pack_mlp_weight_f16")
POINTERS = {
    "idh_binary_mlp_fwd": ("feat", "depth", "w1", "w2", "vecs", "out"),
    "idh_binary_mlp_f16x3_fwd": ("feat", "depth", "w1", "w2", "vecs", "out"),
    "idh_binary_mlp_strided_fwd": ("feat", "depth", "w1", "w2", "vecs", "out"),
    "idh_binary_mlp_search_fwd": ("feat", "w1", "w2", "vecs", "sd", "logits"),
    "idh_binary_mlp_search_thr_fwd": ("feat", "w1", "w2", "vecs", "sd", "logits", "bins", "thr_logits"),
    "idh_binary_mlp_search_f16x3_fwd": ("feat", "w1", "w2", "vecs", "sd", "logits", "bins", "thr_logits"),
    "idh_sample_prior_fwd": ("depth", "prior", "cur", "pcw", "K", "invK", "out"),
    "idh_pack_mlp_weight": ("w", "dst"),
    "idh_pack_mlp_weight_f16": ("w", "dst"),
}


def _refusals():
    """(entry point, overrides of its valid arguments, expected code).  No row may describe a call that would launch."""
    rs = []
    add = lambda e, code=EINVAL, **kw: rs.append((e, kw, code))
    for e in LOGIT + SEARCH:
        add(e, B=-1)
        add(e, HW=0)
        add(e, HW=-3)
        add(e, Cf=0)
        add(e, Cf=-4)
        add(e, Cf=62)  # Cf % 4 != 0
        add(e, B=0, code=OK)
        add(e, B=1 << 10, HW=1 << 21, code=EUNSUPPORTED)  # B HW = 2^31
        add(e, feat=P_(1) + 2)  # base not 4-byte aligned
        for p in POINTERS[e]:
            add(e, **{p: None})
    for e in LOGIT:
        add(e, P=-1)
        add(e, P=0, code=OK)
        add(e, P=0, B=0, code=OK)
    for e in ROWS:
        add(e, feat_cs=60)  # feat_cs < Cf
    add("idh_binary_mlp_fwd", feat_cs=65, B=0, code=OK)  # any row stride ...
    add("idh_binary_mlp_fwd", feat=P_(1) + 4, B=0, code=OK)  # ... and any 4-byte-aligned base (dword loads)
    for e in ALIGNED16:
        add(e, feat_cs=66)  # feat_cs % 4 != 0
        add(e, feat_cs=66, B=0)  # (a shape error: refused before the B == 0 shortcut)
        for off in (4, 8, 12):  # ABI 109: the base must be 16-byte aligned
            add(e, feat=P_(1) + off)
    add("idh_binary_mlp_strided_fwd", ps=0)
    add("idh_binary_mlp_strided_fwd", ps=-1)
    add("idh_binary_mlp_strided_fwd", chs=0)
    add("idh_binary_mlp_strided_fwd", chs=-35)
    add("idh_binary_mlp_strided_fwd", bs=-1)
    add("idh_binary_mlp_strided_fwd", bs=0, B=0, code=OK)  # a zero batch stride (a broadcast frame) is a valid shape
    for e in SEARCH:
        add(e, iters=0)
        add(e, iters=-2)
        add(e, lo=8.0, hi=8.0)
        add(e, lo=8.0, hi=0.5)
        add(e, hi=float("nan"))
    for e, extra in (("idh_binary_mlp_search_fwd", {}), ("idh_binary_mlp_search_f16x3_fwd", {"n_bins": 0})):
        for t in (0.0, 1.0, -0.1, 1.5, float("nan")):
            add(e, threshold=t, **extra)
    add("idh_binary_mlp_search_f16x3_fwd", threshold=7.0, B=0, code=OK)  # with a table the constant is not looked at
    add("idh_binary_mlp_search_f16x3_fwd", n_bins=0, bins=None, thr_logits=None, B=0, code=OK)
    add("idh_binary_mlp_search_thr_fwd", n_bins=0)
    add("idh_binary_mlp_search_thr_fwd", n_bins=-1)
    add("idh_binary_mlp_search_f16x3_fwd", n_bins=-1)
    e = "idh_sample_prior_fwd"
    for kw in ({"Q": 0}, {"Q": -1}, {"P": 0}, {"P": -1}, {"B": -1}, {"H": 0}, {"W": 0}, {"B": 65536}):
        add(e, **kw)
    add(e, B=0, code=OK)
    for p in POINTERS[e]:
        add(e, **{p: None})
    for e in PACKERS:
        add(e, ld=64)  # col0 + n_in > ld
        add(e, n_in=0)
        add(e, n_in=-16)
        add(e, col0=-1)
        for p in POINTERS[e]:
            add(e, **{p: None})
    return rs


REFUSALS = _refusals()


@pytest.mark.parametrize("row", REFUSALS, ids=lambda r: f"{r[0][4:]}:{','.join(f'{k}={v}' for k, v in r[1].items())}")
def test_refusals_and_their_codes(row):
    entry, over, code = row
    args = dict(ENTRIES[entry])
    assert set(over) <= set(args), over
    args.update(over)
    assert getattr(_lib(), entry)(*args.values()) == code


def test_every_entry_point_has_refusals():
    seen = {r[0] for r in REFUSALS}
    assert seen == set(ENTRIES) and len(ENTRIES) == 9
    for e in ENTRIES:  # each null pointer in turn
        assert {next(iter(r[1])) for r in REFUSALS if r[0] == e and len(r[1]) == 1 and next(iter(r[1].values())) is None} == set(POINTERS[e])


@pytest.mark.parametrize("n_in", [-1, 0, 1, 16, 17, 64, 65, 128])
def test_size_queries(n_in):
    L = _lib()
    assert L.idh_packed_mlp_weight_floats(n_in) == (0 if n_in <= 0 else ((n_in + 15) // 16) * 8 * 64 * 4)
    assert L.idh_packed_mlp_weight_f16_bytes(n_in) == (0 if n_in <= 0 else ((n_in + 31) // 32) * 8 * 2 * 64 * 16 + 128 * 4)


# ---- the tables reach what they claim (fp64 reference only) ------------------------------------------------------------------
def test_logit_table_covers_every_value_per_entry_point():
    for entry in ("fp32", "f16x3", "strided"):
        cs = [c for c in R.LOGIT_CASES if c.entry == entry]
        assert {c.cf for c in cs} == {4, 20, 48, 64, 68, 128, 256}
        assert {1, 15, 16, 17} <= {c.M for c in cs if c.B == 1}
        assert any(c.B == 3 and c.HW == 21 for c in cs)
        assert {c.P for c in cs} == {1, 3}
        assert {c.prior for c in cs} == {None, "tensor", -1.0, 0.37}
        big = [c for c in cs if c.large]
        waves = 8 if entry == "f16x3" else 12
        assert len(big) == 1 and big[0].P == 1 and big[0].cf == 64 and big[0].B == 2 and big[0].M > 256 * waves * 16
        layouts = {"fp32": {"dense", "wide", "row65", "row66", "base1"}, "f16x3": {"dense", "wide"}, "strided": {"nchw", "frames2", "nhwc"}}[entry]
        assert {c.layout for c in cs} == layouts
    for c in R.LOGIT_CASES:
        if c.entry != "strided":
            cs_, off = R.row_layout(c)
            assert cs_ >= c.cf and (c.entry == "fp32" or (cs_ % 4 == 0 and off % 4 == 0))
    # the dword path taken because of the base alone: a stride that is a multiple of 4 on a base that is not 16-byte aligned
    assert any(R.row_layout(c) == (c.cf + 4, 1) for c in R.LOGIT_CASES if c.layout == "base1")


@pytest.mark.parametrize("case", [c for c in R.LOGIT_CASES if not c.large], ids=lambda c: c.name)
def test_logit_case_inputs(case):
    feat, depth, prior = R.logit_inputs(case)
    assert (depth == 80.0).any() and (case.M * case.P == 1 or (depth == 0.0).any())
    m = R.make_net(case.cf, case.has_prior, R._seed(case.name))
    w = R.weights64(m)
    p64 = R.prior64(case, prior, depth.shape)
    ref = R.reference_logits(w, feat, depth, p64)
    mine, tol = R.logit_bound(w, feat, depth, p64, f16=case.entry == "f16x3")
    assert (mine - ref).abs().max().item() < 1e-11  # the layer-by-layer restatement the bound is built on is the oracle's network
    assert (tol > 0).all() and tol.max().item() < 0.1  # (worst-case propagation through three layers; the widest belong to the depth-80 pixels)
    if case.P > 1:  # planes whose logits differ
        assert ((ref[:, 0] - ref[:, 1]).abs() > tol[:, 0] + tol[:, 1]).float().mean().item() > 0.5
    # the hostile buffer holds the features where the entry point will look for them, NaN elsewhere
    buf, off, fargs = R.feature_buffer(case, feat)
    assert int((~buf.isnan()).sum()) == feat.numel()
    bs, ps, chs = fargs if len(fargs) == 3 else (case.HW * fargs[0], fargs[0], 1)
    b, pix, ch = case.B - 1, case.HW - 1, case.cf - 1
    assert buf[off + b * bs + pix * ps + ch * chs] == feat[b, ch, pix] and buf[off] == feat[0, 0, 0]
    assert off + b * bs + pix * ps + ch * chs < buf.numel()


def _perturbed(case, kind):
    """fp64 logits of a subtly wrong kernel, or None when the case cannot see the defect."""
    feat, depth, prior = R.logit_inputs(case)
    m = R.make_net(case.cf, case.has_prior, R._seed(case.name))
    w = R.weights64(m)
    p64 = R.prior64(case, prior, depth.shape)
    f16 = case.entry == "f16x3"
    ref, tol = R.logit_bound(w, feat, depth, p64, f16)
    if kind == "drop-last-channel":
        f2 = feat.clone()
        f2[:, -1] = 0
        bad = R.logit_bound(w, f2, depth, p64, f16)[0]
    elif kind == "prior-plane-0":
        if case.prior != "tensor" or case.P == 1:
            return None
        bad = R.logit_bound(w, feat, depth, p64[:, :1].expand_as(p64), f16)[0]
    elif kind == "swap-w3":
        w2 = dict(w)
        w2["mlps.s0.4.weight"] = w["mlps.s0.4.weight"].clone()
        w2["mlps.s0.4.weight"][0, [0, 1]] = w["mlps.s0.4.weight"][0, [1, 0]]
        bad = R.logit_bound(w2, feat, depth, p64, f16)[0]
    elif kind == "relu":
        bad = R.logit_bound(w, feat, depth, p64, f16, elu=torch.relu)[0]
    elif kind == "depth-wrong-plane":
        if case.P == 1:
            return None
        bad = R.logit_bound(w, feat, depth.roll(1, 1), p64, f16)[0]
    return ((bad - ref).abs() > tol).float().mean().item()


@pytest.mark.parametrize("kind", ["drop-last-channel", "prior-plane-0", "swap-w3", "relu", "depth-wrong-plane"])
def test_the_bound_discriminates(kind):
    """Each defect, applied to the fp64 reference, exceeds the elementwise bound on at least a tenth of the pixels of every case
    of at least 15 rows that can see it (a one-row case has no tenth)."""
    shares = {c.name: _perturbed(c, kind) for c in R.LOGIT_CASES if not c.large and c.M >= 15}
    shares = {k: v for k, v in shares.items() if v is not None}
    print(kind, {k: round(v, 3) for k, v in shares.items()})
    assert len(shares) >= 6
    assert min(shares.values()) >= 0.1, min(shares, key=shares.get)


@pytest.mark.parametrize("case", R.SEARCH_CASES, ids=lambda c: c.name)
def test_search_case_inputs(case):
    feat, prior = R.search_inputs(case)
    steps = R.simulate_search(case, R.weights64(R.search_net(case)), feat, prior)
    moved_hi = np.zeros(steps[0]["vis"].shape, bool)
    moved_lo = moved_hi.copy()
    for s in steps:
        moved_hi |= s["vis"]
        moved_lo |= ~s["vis"]
    assert moved_hi.any() and moved_lo.any()  # both bounds move somewhere in the image
    assert moved_hi.mean() > 0.05 and moved_lo.mean() > 0.05
    if (case.lo, case.hi) == (1.0, 3.0):
        assert R.first_query(case) == np.float32(case.lo)  # the reference's (hi - lo) / 2 start equals lo here
    if case.table:
        bins = np.asarray(case.table[0], dtype=np.float32)
        on_edge = any(np.isin(s["q"], bins).any() for s in steps)
        past = any((s["idx"] == len(bins)).any() for s in steps)
        used = set(np.unique(np.concatenate([np.minimum(s["idx"], len(bins) - 1).ravel() for s in steps])).tolist())
        if case.thr == "edge":
            assert on_edge and (steps[0]["q"] == np.float32(3.75)).all() and (steps[0]["idx"] == 2).all()  # 3.75 itself is not "strictly below"
            assert len(used) >= 4
        if case.thr in ("clamp", "one"):
            assert past  # a query beyond the last edge: the count reaches n_bins
        if case.thr == "clamp":
            assert len(used) == 3


def test_search_table_covers_every_combination():
    combos = {(c.entry, c.table is not None, "none" if c.prior is None else "tensor" if c.prior == "tensor" else "const") for c in R.SEARCH_CASES}
    assert len(combos) == 12
    assert {(c.lo, c.hi) for c in R.SEARCH_CASES} == {(0.5, 8.0), (1.0, 3.0)}
    assert {c.thr for c in R.SEARCH_CASES} == {0.5, 0.3, "edge", "clamp", "one"} and {c.cf for c in R.SEARCH_CASES} == {64, 20}
    assert all(R.row_layout(c)[0] % 4 == 0 and R.row_layout(c)[1] % 4 == 0 for c in R.SEARCH_CASES)  # 16-byte-aligned rows (ABI 109)
    assert R.const_thr_logit(0.5) == 0.0


@pytest.mark.parametrize("case", R.PRIOR_CASES, ids=lambda c: c.name)
def test_sample_prior_case_inputs(case):
    args = R.prior_inputs(case)
    depth, prior = args[:2]
    ref = R.prior_reference(case, *args)
    skip = R.prior_skip_mask(case, depth, *args[2:])
    share = skip.float().mean().item()
    print(f"{case.name}: skipped share {share:.4%}")
    assert (ref[depth <= 0] == -1).all() and (depth <= 0).any() == (case.kind != "tie")
    if case.kind == "general":
        assert share <= 0.01
        assert case.B == 3 and (args[4][0] != args[4][1]).any() and (args[2][1] != args[2][2]).any()  # per-frame intrinsics and poses
        # the last frame's previous camera looks the other way: 0 where the depth is positive, -1 where it is not
        last = ref[-1]
        assert ((last == 0) | (last == -1)).all() and ((last == 0) == (depth[-1] > 0)).all()
        # the other frames really sample: most valid pixels land inside the previous image
        inside = (ref[:-1] > 0).float().mean().item()
        assert inside > 0.3, inside
        if case.Q > 1:  # plane p reads channel min(p, Q - 1): values in [q, q + 1)
            for p in range(case.P):
                v = ref[:-1, p][ref[:-1, p] > 0]
                assert len(v) and (v.floor() == min(p, case.Q - 1)).all()
    else:
        assert share == 0.0  # nothing is skipped in the exact cases
    if case.kind == "tie":
        H, W = case.H, case.W
        want = torch.zeros(H, W, dtype=torch.float64)
        for y in range(H):
            for x in range(W):
                xs = x + 2 + (x % 2)  # x + 2.5 rounds half to even
                if xs < W and y + 1 < H:
                    want[y, x] = prior[0, 0, y + 1, xs]
        assert torch.equal(ref[0, 0], want)
        away = torch.zeros_like(want)  # a kernel rounding half away from zero: x + 3 everywhere
        for y in range(H - 1):
            for x in range(W - 3):
                away[y, x] = prior[0, 0, y + 1, x + 3]
        assert (away != want).float().mean().item() > 0.3
    if case.kind == "identity":
        p_of = [min(p, case.Q - 1) for p in range(case.P)]
        assert torch.equal(torch.where(depth > 0, prior[:, p_of], torch.full_like(depth, -1.0)).double(), ref)


def test_pack_reference_layout():
    """The numpy statement of the fragment order against the formula in idh.h, on a matrix that names its own coordinates."""
    w = (torch.arange(128).view(128, 1) * 1000 + torch.arange(23).view(1, 23)).float()
    d = R.packed_fragment_order(w, 1, 20)
    assert d.shape == (2, 8, 64, 4)
    assert d[1, 3, 37, 2] == 0  # k = 16 + 8 + 2 = 26 >= 20
    assert d[1, 3, 5, 2] == (48 + 5) * 1000 + 1 + 18 and d[0, 7, 63, 3] == 127 * 1000 + 1 + 15
    assert {(n, c0) for n, c0, ld in R.PACK_CASES} == {(n, c) for n in (4, 20, 64, 65, 128) for c in (0, 1)} and all(ld > c0 + n for n, c0, ld in R.PACK_CASES)
    assert {n for n, _, _ in R.PACK_F16_CASES} == {20, 128}
