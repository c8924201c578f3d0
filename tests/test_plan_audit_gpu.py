"""The plan hazard audit (tests/plan_audit.py) on the device.

(a) ``footprints`` against the kernels, one op per launch, over every spec of conv_op_ref.CASES and op_kind_ref.CASES: with every float of
    every input allocation outside the predicted reads overwritten by a NaN pattern the op's outputs keep every bit, and the floats of the
    output-side allocations (the wider output buffer, split-K / InstanceNorm workspaces, the head's exp output) that no longer hold the
    prefill pattern are exactly the predicted writes.  No tolerance.  An audit that passed because ``footprints`` forgot a read or a write
    fails here.
(b) the plans ``nhwc.Plan`` builds for the shipped hot paths (bench.py's workload at batch 1 / 4 / 32, the DepthModel path, every buffer
    recycled) have no order or concurrency hazard.
(c) the plans csrc/networks.hip builds on real memory (idh_basic_block_fwd, idh_cvencoder_fwd, idh_unetpp_fwd, idh_model_fwd), seen through
    idh_debug_set_plan_observer, have none either, and every footprint lies inside the workspace, the blob or a tensor the caller declared.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import conv_op_ref as R
import op_kind_ref as K
import plan_audit as A

pytestmark = pytest.mark.gpu

POISON = 0x7FC0DEAD  # a quiet NaN that is neither the prefill pattern nor a NaN the cases build themselves


def _run(op):
    from implicit_depth_amd import _lib, nhwc

    arr, p = R.op_array(nhwc, [op])
    _lib.check(_lib.lib().idh_run_ops(p, 1, _lib.stream_ptr()), "idh_run_ops")
    torch.cuda.synchronize()


def _bits(t):
    return t.reshape(-1).view(torch.int32)


def _check_footprints(op, dev, outputs, split=None, footprints=A.footprints):
    """dev: name -> device tensor (4-byte elements) of every allocation of the case; ``outputs``: the names on the output side."""
    allocs = {n: t for n, t in dev.items() if t._base is None}  # (views of another entry, e.g. the statistics inside their workspace, ride with it)
    assert all(t.is_contiguous() and t.element_size() == 4 for t in allocs.values())
    reads, writes = footprints(op, split)
    masks = {n: np.zeros(t.numel(), dtype=bool) for n, t in allocs.items()}

    def mark(f, side):
        for n, t in allocs.items():
            base = t.data_ptr() // 4
            if base <= f.lo < base + t.numel():
                assert f.hi <= base + t.numel(), f"{f!r} runs past the end of {n}"
                assert (n in outputs) == (side == "write"), f"{f!r} is a {side} of {n}"
                masks[n][f.indices(base)] = True
                return
        raise AssertionError(f"{f!r} lies in no allocation of the case")

    for f in reads:
        mark(f, "read")
    for f in writes:
        mark(f, "write")
    for n in outputs:
        _bits(allocs[n]).fill_(R.PREFILL)
    _run(op)
    first = {n: _bits(allocs[n]).clone() for n in outputs}
    for n, t in allocs.items():
        if n in outputs:
            _bits(t).fill_(R.PREFILL)
        else:
            _bits(t)[torch.from_numpy(~masks[n]).to(t.device)] = POISON
    _run(op)
    poisoned = sum(int((~masks[n]).sum()) for n in allocs if n not in outputs)
    for n in outputs:
        got = _bits(allocs[n])
        assert torch.equal(got, first[n]), f"{n} changed when the floats outside the predicted reads became NaN"
        written = (got != R.PREFILL).cpu().numpy()
        extra, missing = int((written & ~masks[n]).sum()), int((~written & masks[n]).sum())
        assert extra == 0 and missing == 0, f"{n}: {extra} floats written outside the predicted footprint, {missing} predicted floats not written"
    return poisoned


CONV = {s.name: s for s in R.CASES}
KIND = {s.name: s for s in K.CASES}


@pytest.mark.parametrize("name", list(CONV))
def test_conv_footprints_match_the_kernel(name):
    from implicit_depth_amd import _lib, nhwc

    spec = CONV[name]
    t0 = time.time()
    c = R.make_conv_case(spec, "cuda")
    rc, variant = R.variant_of(_lib.lib(), nhwc, c.op)
    assert rc == 0 and variant == spec.variant
    poisoned = _check_footprints(c.op, c.dev, {"out", "ws"} & set(c.dev), split=variant[4])
    print(f"{name}: {poisoned} input floats poisoned, {time.time() - t0:.2f} s")


@pytest.mark.parametrize("name", list(KIND))
def test_op_kind_footprints_match_the_kernel(name):
    spec = KIND[name]
    t0 = time.time()
    c = K.make_case(spec, "cuda")
    poisoned = _check_footprints(c.op, c.dev, {"out", "exp", "ws"} & set(c.dev))
    print(f"{name}: {poisoned} input floats poisoned, {time.time() - t0:.2f} s")


def _forget(what, side):
    def fp(op, split):
        reads, writes = A.footprints(op, split)
        drop = lambda fs: [f for f in fs if f.what != what]
        return (drop(reads), writes) if side == "read" else (reads, drop(writes))
    return fp


def _short_out(op, split):  # the output four channels short
    reads, writes = A.footprints(op, split)
    return reads, [A.strided(op.out, op.N * op.Ho * op.Wo, op.out_cs, 0, op.Cout - 4, "out")] + writes[1:]


def _no_padding(op, split):  # source 0 read over [0, Cin) instead of whole 16-channel blocks
    reads, writes = A.footprints(op, split)
    s = op.src[0]
    return [A.strided(s.in_, op.N * s.H * s.W, s.cs, 0, s.Cin, "src[0].in")] + reads[1:], writes


@pytest.mark.parametrize("fault,message", [
    (_forget("res", "read"), "changed when"), (_forget("bias", "read"), "changed when"), (_forget("src[1].in", "read"), "changed when"),
    (_forget("ws", "write"), "ws: [0-9]+ floats written outside"), (_short_out, "out: 1368 floats written outside"),
])
def test_a_wrong_footprint_fails_the_check(fault, message):
    """The check of (a) is no formality: without the residual, the bias or the second source among the reads, without the split-K workspace
    among the writes, or with an output four channels short (4 x M, M = 2 x 9 x 19 = 342), the case lds9-n0-proj1x1-split2 fails."""
    spec = CONV["lds9-n0-proj1x1-split2"]
    assert spec.res and spec.bias and spec.S == 2
    c = R.make_conv_case(spec, "cuda")
    with pytest.raises(AssertionError, match=message):
        _check_footprints(c.op, c.dev, {"out", "ws"}, split=spec.S, footprints=fault)


def test_a_forgotten_padding_read_fails_the_check():
    """... and so does a conv read that stops at Cin = 40 instead of the 16-channel block's end (48): the kernels do read the padding."""
    for name in ("lds9-n0-c64", "direct-4x4-3x3"):  # 16-channel chunks / K steps: 40 -> 48, 24 -> 32
        c = R.make_conv_case(CONV[name], "cuda")
        assert c.op.src[0].Cin % 16
        with pytest.raises(AssertionError, match="changed when"):
            _check_footprints(c.op, c.dev, {"out"}, footprints=_no_padding)


# ----------------------------------------------------------------------------------------------------------------------------------------
# (b) nhwc.Plan
# ----------------------------------------------------------------------------------------------------------------------------------------
def _audit_python_plan(model, label, want_recycled):
    assert len(model._plans) == 1
    ent = next(iter(model._plans.values()))
    p = ent["plan"]
    pos = p._pos  # build index -> position after schedule_segments
    order = [0] * len(pos)
    for build, at in enumerate(pos):
        order[at] = build
    ops = list(p._array())  # (the array the pass replays: source and output pointers patched in)
    found = A.audit(ops, order, ent["n_head_ops"])
    print(f"{label}: {found.summary()}; recycled {p.recycled}")
    assert not found, [repr(f) for f in found[:8]]
    assert found.conservative == 0 and found.decided > 0
    if want_recycled:
        assert p.recycled >= 1
    return found


@pytest.mark.parametrize("batch", [1, 4, 32])
def test_bench_hot_path_plan_is_clean(batch):
    import bench

    t0 = time.time()
    w = bench.HotPathWorkload(bench.parse(["--batch", str(batch)]), torch.device("cuda"), 0)
    w.step()
    torch.cuda.synchronize()
    found = _audit_python_plan(w.model, f"bench hot_path batch {batch}", want_recycled=batch == 32)
    assert found.ops > 100 and found.largest_group >= 2
    print(f"{time.time() - t0:.2f} s")


def _pipeline(B, K_, H, W, D, P, depth_model):
    from test_pipeline_gpu import _build

    model, inp, pyr, rd = _build(B, K_, H, W, D, P, depth_model=depth_model)
    model.cuda()
    d = {k: v.cuda() for k, v in inp.items()}
    model(d["cur_feats"], d["src_feats"], [t.cuda() for t in pyr], d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"],
          rendered_depth=None if depth_model else rd.cuda())
    torch.cuda.synchronize()
    return model


@pytest.mark.parametrize("B", [1, 4])
def test_depth_model_hot_path_plan_is_clean(B):
    """DepthDecoderPP with its four 1x1 heads (log-depth + exp outputs) at the shipped size: 96 x 128 matching map, 64 planes."""
    found = _audit_python_plan(_pipeline(B, 7, 96, 128, 64, 2, True), f"DepthModel hot path B={B}", want_recycled=False)
    assert found.ops > 100 and found.largest_group >= 2


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("depth_model", [False, True])
def test_plan_with_every_buffer_recycled_is_clean(B, depth_model):
    """nhwc.REUSE_MIN_BYTES = 0, as test_pipeline_gpu.py::test_buffer_reuse_aliasing_is_bit_identical sets up: every released buffer is taken over."""
    from implicit_depth_amd import nhwc

    old = (nhwc.BUFFER_REUSE, nhwc.REUSE_MIN_BYTES)
    try:
        nhwc.BUFFER_REUSE, nhwc.REUSE_MIN_BYTES = True, 0
        model = _pipeline(B, 2, 24, 32, 16, 2, depth_model)
    finally:
        nhwc.BUFFER_REUSE, nhwc.REUSE_MIN_BYTES = old
    _audit_python_plan(model, f"every buffer recycled, B={B}, depth_model={depth_model}", want_recycled=True)
    assert next(iter(model._plans.values()))["plan"].recycled >= 8


# ----------------------------------------------------------------------------------------------------------------------------------------
# (c) csrc/networks.hip on real memory
# ----------------------------------------------------------------------------------------------------------------------------------------
def _declared(t, N):
    """(address, floats) an idh_tensor (net_abi.Tensor) of N images declares."""
    from implicit_depth_amd import net_abi as na

    if t.layout == na.LAYOUT_NCHW:
        return (t.ptr, N * t.C * t.H * t.W)
    # (include/idh_net.h: a channel count that is no multiple of 16 is a whole zero-padded buffer, cs == ceil16(C): the padding is the caller's too)
    return (t.ptr, (N * t.H * t.W - 1) * t.cs + (A.ceil16(t.C) if t.cs == A.ceil16(t.C) else t.C))


def _check_observed(plans, label, sz, ws, blob, externals):
    assert len(plans) == 1, label
    p = plans[0]
    assert p.ws == (ws.data_ptr(), sz.workspace_floats) and p.blob == (blob.data_ptr(), sz.weight_floats) and len(p.ops) == sz.ops, label
    found = p.audit(externals)
    print(f"{label}: {found.summary()}")
    assert not found, [repr(f) for f in found[:8]]
    assert found.conservative == 0
    return found


def test_basic_block_fwd_plans_are_clean():
    from implicit_depth_amd import _lib
    from implicit_depth_amd import net_abi as na
    from implicit_depth_amd.layers import BasicBlock
    from test_net_abi_gpu import _alloc

    import implicit_depth_amd.synthetic as syn

    L = _lib.lib()
    for cin, cout, stride in ((24, 24, 1), (24, 40, 1), (24, 40, 2)):
        for layout in ("nchw", "nhwc"):
            bb = BasicBlock(cin, cout, stride).cuda()
            syn.fill_state_dict(bb, seed=10)
            N, H, W = 2, 12, 20
            Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
            keep = []
            blk = na.block_params(bb, keep)
            if layout == "nchw":
                x, out = torch.randn(N, cin, H, W, device="cuda"), torch.empty(N, cout, Ho, Wo, device="cuda")
                tx, to = na.nchw(x), na.nchw(out)
            else:  # a zero-padded 32-channel input, the output a channel slice of a wider buffer
                x, out = torch.zeros(N, H, W, 32, device="cuda"), torch.empty(N, Ho, Wo, cout + 16, device="cuda")
                tx, to = na.nhwc(x, cin), na.Tensor(out.data_ptr() + 4 * 16, na.LAYOUT_NHWC, cout, Ho, Wo, cout + 16)
            sz = na.NetSizes()
            _lib.check(L.idh_basic_block_sizes(C.byref(blk), N, C.byref(tx), C.byref(to), C.byref(sz)), "sizes")
            blob, ws = _alloc(sz)
            _lib.check(L.idh_basic_block_pack(C.byref(blk), N, C.byref(tx), C.byref(to), blob.data_ptr(), _lib.stream_ptr()), "pack")
            with A.observe() as plans:
                _lib.check(L.idh_basic_block_fwd(C.byref(blk), blob.data_ptr(), N, C.byref(tx), C.byref(to), ws.data_ptr(), sz.workspace_floats,
                                                 _lib.stream_ptr()), "fwd")
            torch.cuda.synchronize()
            _check_observed(plans, f"idh_basic_block_fwd {cin}>{cout}/{stride} {layout}", sz, ws, blob, [_declared(tx, N), _declared(to, N)])


@pytest.mark.parametrize("out_layout", ["nhwc", "nchw"])
def test_cvencoder_fwd_plan_is_clean(out_layout):
    from implicit_depth_amd import _lib
    from implicit_depth_amd import net_abi as na
    from test_net_abi_gpu import _alloc, _small_nets

    L = _lib.lib()
    net, pyr, cvol, cve = _small_nets()
    cve.cuda()
    N, D, H, W = cvol.shape
    keep = []
    blocks = na.cvencoder_blocks(cve, keep)
    cost_t = cvol.cuda().permute(0, 2, 3, 1).contiguous() if out_layout == "nhwc" else cvol.cuda().contiguous()
    cost = na.nhwc(cost_t) if out_layout == "nhwc" else na.nchw(cost_t)
    img = [p.cuda() for p in pyr[1:]]
    imgs = na.tensors([na.nchw(t) for t in img])
    shape = (lambda i, c: (N, H >> i, W >> i, c)) if out_layout == "nhwc" else (lambda i, c: (N, c, H >> i, W >> i))
    outs_t = [torch.empty(shape(i, c), device="cuda") for i, c in enumerate(cve.num_ch_enc)]
    outs = na.tensors([(na.nhwc if out_layout == "nhwc" else na.nchw)(t) for t in outs_t])
    sz = na.NetSizes()
    _lib.check(L.idh_cvencoder_sizes(blocks, 4, N, C.byref(cost), imgs, outs, C.byref(sz)), "sizes")
    blob, ws = _alloc(sz)
    _lib.check(L.idh_cvencoder_pack(blocks, 4, N, C.byref(cost), imgs, outs, blob.data_ptr(), _lib.stream_ptr()), "pack")
    with A.observe() as plans:
        _lib.check(L.idh_cvencoder_fwd(blocks, 4, blob.data_ptr(), N, C.byref(cost), imgs, outs, ws.data_ptr(), sz.workspace_floats, _lib.stream_ptr()), "fwd")
    torch.cuda.synchronize()
    ext = [_declared(cost, N)] + [_declared(imgs[i], N) for i in range(4)] + [_declared(outs[i], N) for i in range(4)]
    _check_observed(plans, f"idh_cvencoder_fwd {out_layout}", sz, ws, blob, ext)


@pytest.mark.parametrize("which", ["bd", "depth"])
def test_unetpp_fwd_plan_is_clean(which):
    from implicit_depth_amd import _lib
    from implicit_depth_amd import net_abi as na
    from test_net_abi_gpu import _alloc, _small_nets

    import implicit_depth_amd.synthetic as syn

    L = _lib.lib()
    net, pyr, cvol, cve = _small_nets()
    dec = (net.BDDecoderPP if which == "bd" else net.DepthDecoderPP)([24, 64, 128, 256, 384]).cuda()
    syn.fill_state_dict(dec, seed=13)
    N, H0, W0 = 1, pyr[0].shape[2], pyr[0].shape[3]
    keep = []
    blocks, heads = na.unetpp_blocks(dec, keep)
    f0 = pyr[0].cuda().contiguous()  # level 0 as the reference hands it: NCHW, imported by the library
    nh = [torch.randn(N, H0 >> (i + 1), W0 >> (i + 1), c, device="cuda") for i, c in enumerate([64, 128, 256, 384])]
    feats = na.tensors([na.nchw(f0)] + [na.nhwc(t) for t in nh])
    fo_t = [torch.empty(N, H0 >> i, W0 >> i, c, device="cuda") for i, c in enumerate([64, 64, 128, 256])]
    fouts = na.tensors([na.nhwc(t) for t in fo_t])
    ld = dp = None
    if heads is not None:
        ld = [torch.empty(N, 1, H0 >> i, W0 >> i, device="cuda") for i in range(4)]
        dp = [torch.empty(N, 1, H0 >> i, W0 >> i, device="cuda") for i in range(4)]
    sz = na.NetSizes()
    _lib.check(L.idh_unetpp_sizes(blocks, na.UNETPP_BLOCKS, heads, N, feats, fouts, C.byref(sz)), "sizes")
    blob, ws = _alloc(sz)
    _lib.check(L.idh_unetpp_pack(blocks, na.UNETPP_BLOCKS, heads, N, feats, fouts, blob.data_ptr(), _lib.stream_ptr()), "pack")
    with A.observe() as plans:
        _lib.check(L.idh_unetpp_fwd(blocks, na.UNETPP_BLOCKS, heads, blob.data_ptr(), N, feats, fouts, na.ptr_array(ld), na.ptr_array(dp), ws.data_ptr(),
                                    sz.workspace_floats, _lib.stream_ptr()), "fwd")
    torch.cuda.synchronize()
    ext = [_declared(feats[i], N) for i in range(5)] + [_declared(fouts[i], N) for i in range(4)]
    ext += [(t.data_ptr(), t.numel()) for t in (ld or []) + (dp or [])]
    found = _check_observed(plans, f"idh_unetpp_fwd {which}", sz, ws, blob, ext)
    assert found.ops > 100 and found.largest_group >= 2


def test_model_fwd_plan_is_clean():
    """One idh_model_fwd at B = 2 (DepthModel, the matching-encoder head inside the call): the size query it starts with and the plan it runs."""
    import implicit_depth_amd.synthetic as syn
    from test_model_abi_gpu import _setup

    B, K_, img_h, img_w = 2, 7, 64, 128
    hp, ent, cur, args = _setup(K_, "mlp", "depth", False, B, img_h, img_w, with_head=True)
    l1 = syn.layer1_maps(B, K_, img_h // 4, img_w // 4, seed=9).cuda()
    args["matching_cur_feats"] = args["matching_src_feats"] = None
    plan = ent.prepare(B, K_, 16, img_h // 4, img_w // 4, 0, device="cuda", matching_input=1)
    d, blob, s, ws = plan
    with A.observe() as plans:
        out = ent(**args, matching_layer1=l1, plan=plan)
    torch.cuda.synchronize()
    assert len(plans) == 2, "the layout query, then the pass"
    sized, run = plans
    assert run.ws[0] == ws.data_ptr() and run.blob[0] == blob.data_ptr() and sized.ws[0] != run.ws[0]
    assert (run.ws[1], run.blob[1]) == (sized.ws[1], sized.blob[1]) and run.ws[1] <= s.workspace_floats and run.blob[1] <= s.weight_floats
    ext = [(t.data_ptr(), t.numel()) for t in list(args["cur_feats"]) + [l1] + [v for v in out.values() if torch.is_tensor(v)]]
    for label, p, e in (("idh_model_fwd, layout query", sized, None), ("idh_model_fwd, pass", run, ext)):
        found = p.audit(e)
        print(f"{label}: {found.summary()}")
        assert not found and found.conservative == 0, [repr(f) for f in found[:8]]
        assert found.ops > 100 and found.largest_group >= 2 and p.n_first > 0
