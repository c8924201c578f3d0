"""Every C entry point of csrc/mlp.hip, called directly and compared with fp64 (tables, builders, references and bounds in
tests/mlp_op_ref.py; test_mlp_op_cpu.py shows without a GPU that the tables reach what they claim and pins the refusals).

Logits: the derived elementwise bound of mlp_op_ref.logit_bound.  Searches: teacher forcing over iters = 1 .. 12 - every logit
against the fp64 MLP at the kernel's own previous query, every query bitwise against the fp32 replay of the rule on the kernel's
own logits.  sample_prior: exact equality with the fp64 oracle outside a derived band around the rounding boundaries; exact
everywhere in the tie and identity cases.  Packers: bitwise / within the split's truncation bound.  Every launch writes into a
slice of a prefilled buffer whose surroundings must come back untouched, and runs twice with bitwise equal results."""
import numpy as np
import pytest
import torch

import mlp_op_ref as R

pytestmark = pytest.mark.gpu


def _lib():
    from implicit_depth_amd import _lib

    return _lib.lib()


def _bits(t):
    return t.view(torch.int32)


def _twice(run):
    """Run twice into fresh outputs: both IDH_OK, guard words untouched, results bitwise equal.  Returns the first run's outputs (CPU fp32)."""
    res = []
    for _ in range(2):
        rc, *outs = run()
        assert rc == R.OK
        vals = []
        for o in outs:
            v, clean = o.read()
            assert clean, "a store landed outside the output"
            vals.append(v)
        res.append(vals)
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b)), "two launches of the same call differ in bits"
    return res[0]


def _assert_within(name, got, ref, tol):
    err = (got.double() - ref).abs()
    ok = err <= tol  # (a NaN - an element never written, or a NaN that leaked in from the padding - compares false)
    worst = (err / tol).nan_to_num(nan=float("inf")).max().item()
    print(f"{name}: max err {err.nan_to_num(nan=float('inf')).max().item():.3e}, max err / bound {worst:.4f}")
    assert ok.all(), f"{name}: {int((~ok).sum())} of {ok.numel()} elements exceed the bound, worst err / bound {worst:.3g}, first at {tuple((~ok).nonzero()[0].tolist())}"
    return worst


@pytest.mark.parametrize("case", R.LOGIT_CASES, ids=lambda c: c.name)
def test_logits_match_fp64(case):
    L = _lib()
    feat, depth, prior = R.logit_inputs(case)
    m = R.make_net(case.cf, case.has_prior, R._seed(case.name))
    dev = R.device_case(case, m, feat, depth, prior)
    (got,) = _twice(lambda: R.run_logits(L, case, dev))
    ref, tol = R.logit_bound(R.weights64(m), feat, depth, R.prior64(case, prior, depth.shape), f16=case.entry == "f16x3")
    _assert_within(case.name, got.view(case.B, case.P, case.HW), ref, tol)
    if case.layout == "nhwc":  # NHWC rows expressed as strides: the same bits as idh_binary_mlp_fwd on the same memory
        rc, out = R.run_logits(L, case, dev, entry="fp32")
        assert rc == R.OK
        assert torch.equal(_bits(out.read()[0]), _bits(got))


@pytest.mark.parametrize("case", R.SEARCH_CASES, ids=lambda c: c.name)
def test_search_by_teacher_forcing(case):
    L = _lib()
    feat, prior = R.search_inputs(case)
    m = R.search_net(case)
    w = R.weights64(m)
    dev = R.device_case(case, m, feat, None, prior)
    if case.table:
        dev["bins"], dev["thr_logits"] = (t.cuda() for t in R.table_tensors(case))
    shape = (case.B, 1, case.HW)
    p64 = R.prior64(case, prior, shape)
    lo = np.full(shape, case.lo, dtype=np.float32)
    hi = np.full(shape, case.hi, dtype=np.float32)
    q = np.full(shape, R.first_query(case), dtype=np.float32)
    skipped = np.zeros(shape, bool)
    may_skip = case.table is None and case.thr != 0.5  # the host's logf may differ from numpy's by an ulp; logit(0.5) is exactly 0
    worst, moved_hi, moved_lo = 0.0, False, False
    for n in range(1, R.SEARCH_ITERS + 1):
        q_n, l_n = _twice(lambda: R.run_search(L, case, dev, n))
        q_n, l_n = q_n.view(shape).numpy(), l_n.view(shape)
        # (a) the logit of the evaluation at the kernel's own previous query
        ref, tol = R.logit_bound(w, feat, torch.from_numpy(q), p64, f16=case.entry == "f16x3")
        worst = max(worst, _assert_within(f"{case.name} step {n}", l_n, ref, tol))
        # (b) the next query: the fp32 rule replayed on the kernel's own logit
        thr, _ = R.thresholds_at(case, q)
        l32 = l_n.numpy()
        lo_v, hi_v, q_v = R.search_step(case, lo, hi, q, l32, thr)  # as decided by logit < thr
        if may_skip:
            knife = np.abs(l32 - thr) <= 2 * np.spacing(np.abs(thr))
            other = knife & (q_n.view(np.int32) != q_v.view(np.int32))
            assert (q_n.view(np.int32)[other] == _other_query(lo, hi, q, l32, thr).view(np.int32)[other]).all()
            skipped |= other
            took_other = other
        else:
            took_other = np.zeros(shape, bool)
        expect = np.where(took_other, _other_query(lo, hi, q, l32, thr), q_v).astype(np.float32)
        bad = q_n.view(np.int32) != expect.view(np.int32)
        assert not bad.any(), f"{case.name} step {n}: {int(bad.sum())} queries differ from the replay, first at {tuple(np.argwhere(bad)[0])}"
        vis = (l32 < thr) ^ took_other
        moved_hi, moved_lo = moved_hi or bool(vis.any()), moved_lo or bool((~vis).any())
        hi = np.where(vis, q, hi).astype(np.float32)
        lo = np.where(vis, lo, q).astype(np.float32)
        q = q_n.copy()
    assert (q >= np.float32(case.lo)).all() and (q <= np.float32(case.hi)).all()  # (c)
    assert moved_hi and moved_lo
    assert skipped.mean() <= 1e-3, skipped.mean()
    print(f"{case.name}: worst err / bound over {R.SEARCH_ITERS} steps {worst:.4f}, skipped {int(skipped.sum())} pixels")


def _other_query(lo, hi, q, logit, thr):
    """The query the opposite decision leads to."""
    vis = ~(logit < thr)
    hi2 = np.where(vis, q, hi).astype(np.float32)
    lo2 = np.where(vis, lo, q).astype(np.float32)
    return ((hi2 + lo2) * np.float32(0.5)).astype(np.float32)


@pytest.mark.parametrize("case", R.PRIOR_CASES, ids=lambda c: c.name)
def test_sample_prior_matches_fp64(case):
    L = _lib()
    args = R.prior_inputs(case)
    dev = tuple(a.contiguous().cuda() for a in args)
    (got,) = _twice(lambda: R.run_sample_prior(L, case, dev))
    got = got.view(case.B, case.P, case.H, case.W)
    ref = R.prior_reference(case, *args)
    skip = R.prior_skip_mask(case, args[0], *args[2:])
    share = skip.float().mean().item()
    wrong = (got.double() != ref) & ~skip  # copies of prior elements, 0 or -1: exact
    print(f"{case.name}: skipped {share:.4%}, wrong outside the band {int(wrong.sum())}, wrong inside {int(((got.double() != ref) & skip).sum())}")
    assert share <= (0.01 if case.kind == "general" else 0.0)
    assert not wrong.any(), f"{case.name}: {int(wrong.sum())} pixels differ, first at {tuple(wrong.nonzero()[0].tolist())}"


@pytest.mark.parametrize("n_in,col0,ld", R.PACK_CASES)
def test_pack_mlp_weight_is_the_fragment_order(n_in, col0, ld):
    from implicit_depth_amd import _lib

    L = _lib.lib()
    w = R.pack_source(n_in, col0, ld, seed=n_in * 2 + col0)
    wd = w.cuda()
    n = L.idh_packed_mlp_weight_floats(n_in)

    def run():
        out = R.Out(n)
        rc = L.idh_pack_mlp_weight(wd.data_ptr(), out.ptr, ld, col0, n_in, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, out

    (got,) = _twice(run)
    want = torch.from_numpy(R.packed_fragment_order(w, col0, n_in)).reshape(-1)
    assert got.numel() == want.numel() and torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("n_in,col0,ld", R.PACK_F16_CASES)
def test_pack_mlp_weight_f16_pieces_and_scales(n_in, col0, ld):
    """(hi + lo) * scale reproduces W within the split's truncation: hi = f16(v), lo = f16(v - hi) of v = W / scale miss v by at most
    2^-22 |v| (two half-ulp roundings of 11-bit significands; 2^-24, an f16 subnormal step, where a piece is subnormal).  The scales
    are 2^(e - 14) with 2^e <= max |row| < 2^(e + 1), so |v| < 2^15 fits f16."""
    from implicit_depth_amd import _lib

    L = _lib.lib()
    w = R.pack_source(n_in, col0, ld, seed=100 + n_in)
    wd = w.cuda()
    nbytes = L.idh_packed_mlp_weight_f16_bytes(n_in)

    def run():
        out = R.Out(nbytes // 4)
        rc = L.idh_pack_mlp_weight_f16(wd.data_ptr(), out.ptr, ld, col0, n_in, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, out

    (got,) = _twice(run)
    hi, lo, scales = R.decode_f16_pack(got.numpy().tobytes(), n_in)
    W = w[:, col0: col0 + n_in].double().numpy()
    mant, exp = np.frexp(scales.astype(np.float64))
    assert (mant == 0.5).all()  # exact powers of two
    rowmax = np.abs(W).max(1)
    assert (np.floor(np.log2(rowmax)) - 14 == exp - 1).all()
    s = scales.astype(np.float64)[:, None]
    assert (hi[:, n_in:] == 0).all() and (lo[:, n_in:] == 0).all()  # zero padding up to the 32-wide K block
    err = np.abs((hi[:, :n_in] + lo[:, :n_in]) * s - W)
    tol = 2.0 ** -22 * np.abs(W) + 2.0 ** -24 * s
    print(f"f16 pack n_in={n_in}: max err / bound {(err / tol).max():.4f}")
    assert (err <= tol).all()
    assert (np.abs(lo[:, :n_in]) <= 2.0 ** -11 * np.abs(hi[:, :n_in]) + 2.0 ** -24).all()  # lo really is the remainder of hi
