"""The plan hazard audit (tests/plan_audit.py), host side: it finds every seeded fault - a region a plan builder forgot to hand to
idh_schedule_ops - as exactly the hazard that region stood for, it stays quiet on complete plans, and every plan the C++ builder
(csrc/networks.hip) schedules for the shipped configurations is free of hazards and stays inside its workspace and weight blob.

The seeded lists are hand-built descriptors on made-up addresses, scheduled by the library's own idh_schedule_ops."""
import ctypes as C

import pytest

import op_kind_ref as KR
import plan_audit as A
from test_model_abi_cpu import CONFIGS, _entry

H, W = 8, 16  # every map of the seeded lists (half-size maps: 4 x 8)


class Mini:
    """An op list on made-up memory with the regions a plan builder would record: ``add(op, reads, writes)``, regions as (buffer, c0, c1)."""

    def __init__(self):
        self.next = 1 << 32
        self.plan = []

    def alloc(self, floats):
        a = self.next
        self.next += (4 * floats + 255) & ~255
        return a

    def buffer(self, cs, h=H, w=W):
        return self.alloc(h * w * cs)

    def add(self, op, reads, writes):
        self.plan.append((op, list(reads), list(writes)))
        return len(self.plan) - 1

    def conv(self, x, cin, x_cs, out, cout, out_cs, tile_m=9, tile_n=0, res=None, res_cs=0, up=None, norm=None, split_k=1, ws=None):
        """3x3 stride-1 conv of view x (address of its channel 0) into view out; up = (address, cs, C) of a half-size map behind cin channels."""
        from implicit_depth_amd import nhwc

        o = nhwc.Op()
        o.kind, o.N, o.Ho, o.Wo, o.Cout, o.tile_m, o.tile_n, o.split_k = nhwc.OP_CONV, 1, H, W, cout, tile_m, tile_n, split_k
        s = o.src[0]
        s.in_, s.cs, s.H, s.W, s.Cin, s.ks, s.stride = x, x_cs, H, W, cin + (up[2] if up else 0), 3, 1
        s.w = self.alloc(9 * A.ceil16(s.Cin) * A.ceil16(cout))
        if up:
            s.up_in[0], s.up_cs[0], s.up_c0, s.up_C = up[0], up[1], cin, up[2]
        if norm:
            s.norm, s.norm_act, s.norm_slope = norm, 1, 0.2
        o.bias = self.alloc(cout)
        if res:
            o.res, o.res_cs = res, res_cs
        o.out, o.out_cs = out, out_cs
        if ws:
            o.ws = ws
        return o

    def instnorm(self, x, c, cs):
        from implicit_depth_amd import nhwc

        o = nhwc.Op()
        o.kind, o.N = nhwc.OP_INSTNORM, 1
        s = o.src[0]
        s.in_, s.cs, s.H, s.W, s.Cin = x, cs, H, W, c
        o.ws = self.alloc(2 * 2 * c)  # one chunk: partials, then mean / rstd
        return o, o.ws + 4 * 2 * c

    def export(self, x, c, cs, out):
        from implicit_depth_amd import nhwc

        o = nhwc.Op()
        o.kind, o.N, o.out = nhwc.OP_EXPORT, 1, out
        s = o.src[0]
        s.in_, s.cs, s.H, s.W, s.Cin = x, cs, H, W, c
        return o

    def schedule(self, n_first=0, leave_out=None, replace=None):
        """Scheduled ops + order; leave_out = (op, "reads" / "writes", index): that region never reaches the scheduler; replace =
        (op, "reads" / "writes", index, region): it does, in this (wrong) form."""
        from implicit_depth_amd import _lib, nhwc

        n = len(self.plan)
        ops = (nhwc.Op * n)(*[p[0] for p in self.plan])
        regions, offs = [], [0]
        for k, (_, reads, writes) in enumerate(self.plan):
            for name, rs in (("reads", reads), ("writes", writes)):
                for j, r in enumerate(rs):
                    if leave_out == (k, name, j):
                        continue
                    if replace is not None and replace[:3] == (k, name, j):
                        r = replace[3]
                    regions += list(r)
                offs.append(len(regions) // 3)
        order = (C.c_int32 * n)()
        rc = _lib.lib().idh_schedule_ops(ops, n, n_first, (C.c_uint64 * (len(regions) + 1))(*regions), (C.c_int32 * len(offs))(*offs),
                                         nhwc.SCHED_MERGE_LEVELS | nhwc.SCHED_WINO_GROUP, order, None)
        assert rc == 0
        return list(ops), list(order)


def _residual():
    m = Mini()
    a, b, x, y = m.buffer(64), m.buffer(64), m.buffer(64), m.buffer(64)
    m.add(m.conv(a, 64, 64, x, 64, 64), [(a, 0, 64)], [(x, 0, 64)])
    m.add(m.conv(b, 64, 64, y, 64, 64, res=x, res_cs=64), [(x, 0, 64), (b, 0, 64)], [(y, 0, 64)])
    return m, 0, dict(leave_out=(1, "reads", 0)), {("concurrency", "RAW", 0, "out", 1, "res")}


def _up_in():
    m = Mini()
    a, low, x, y = m.buffer(64, H // 2, W // 2), m.buffer(32, H // 2, W // 2), m.buffer(16), m.buffer(64)
    o = m.conv(a, 64, 64, low, 32, 32)
    o.Ho, o.Wo, o.src[0].H, o.src[0].W = H // 2, W // 2, H // 2, W // 2
    m.add(o, [(a, 0, 64)], [(low, 0, 32)])
    m.add(m.conv(x, 16, 16, y, 64, 64, up=(low, 32, 32)), [(x, 0, 16), (low, 0, 32)], [(y, 0, 64)])
    return m, 0, dict(leave_out=(1, "reads", 1)), {("concurrency", "RAW", 0, "out", 1, "src[0].up_in[0]")}


def _norm_stats():
    m = Mini()
    a, h, y = m.buffer(64), m.buffer(32), m.buffer(16)
    m.add(m.conv(a, 64, 64, h, 32, 32), [(a, 0, 64)], [(h, 0, 32)])
    st, stats = m.instnorm(h, 32, 32)
    m.add(st, [(h, 0, 32)], [(stats, 0, 1)])
    # the conv (4-row tiles, 16 channels: a grouped rank) sorts in front of the statistics pass of its level unless it waits for it
    m.add(m.conv(h, 32, 32, y, 16, 16, tile_n=1, norm=stats), [(stats, 0, 1), (h, 0, 32)], [(y, 0, 16)])
    return m, 0, dict(leave_out=(2, "reads", 0)), {("order", "RAW", 1, "ws", 2, "src[0].norm")}


def _pad16():
    m = Mini()
    a, b, x, y = m.buffer(64), m.buffer(64), m.buffer(16), m.buffer(64)
    m.add(m.conv(a, 64, 64, x, 12, 16), [(a, 0, 64)], [(x, 0, 12)])
    m.add(m.conv(x, 12, 16, y, 64, 64), [(x, 0, 16)], [(y, 0, 64)])  # reads the whole 16-channel block
    m.add(m.conv(b, 64, 64, x + 4 * 12, 4, 16), [(b, 0, 64)], [(x, 12, 16)])  # a later writer of the padding channels
    return m, 0, dict(replace=(1, "reads", 0, (x, 0, 12))), {("order", "WAR", 1, "src[0].in", 2, "out")}


def _split_ws(shared=True):
    m = Mini()
    a, b, x, y = m.buffer(64), m.buffer(64), m.buffer(64), m.buffer(64)
    ws = [m.alloc(2 * H * W * 64) for _ in range(2)]
    m.add(m.conv(a, 64, 64, x, 64, 64, split_k=2, ws=ws[0]), [(a, 0, 64)], [(x, 0, 64)])
    m.add(m.conv(b, 64, 64, y, 64, 64, split_k=2, ws=ws[0 if shared else 1]), [(b, 0, 64)], [(y, 0, 64)])
    return m, 0, {}, {("concurrency", "WAW", 0, "ws", 1, "ws")}


def _recycled():
    m = Mini()
    a, t, u, v = m.buffer(64), m.buffer(64), m.buffer(64), m.buffer(64)
    m.add(m.conv(a, 64, 64, t, 64, 64), [(a, 0, 64)], [(t, 0, 64)])  # segment 0 fills t
    m.add(m.conv(t, 64, 64, u, 64, 64), [(t, 0, 64)], [(u, 0, 64)])  # its last reader
    m.add(m.conv(v, 64, 64, t, 64, 64), [(v, 0, 64)], [(t, 0, 64)])  # t recycled: the new writer
    return m, 1, dict(leave_out=(2, "writes", 0)), {("concurrency", "WAR", 1, "src[0].in", 2, "out")}


def _exports():
    m = Mini()
    a, x, y, d = m.buffer(64), m.buffer(64), m.buffer(64), m.alloc(64 * H * W)
    m.add(m.conv(a, 64, 64, x, 64, 64), [(a, 0, 64)], [(x, 0, 64)])
    m.add(m.export(x, 64, 64, d), [(x, 0, 64)], [(d, 0, 1)])
    m.add(m.export(y, 64, 64, d), [(y, 0, 64)], [(d, 0, 1)])
    return m, 0, dict(leave_out=(2, "writes", 0)), {("order", "WAW", 1, "out", 2, "out")}


SEEDED = {"residual": _residual, "up_in": _up_in, "norm_stats": _norm_stats, "pad16": _pad16, "split_ws": _split_ws, "recycled": _recycled,
          "exports": _exports}


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_audit_finds_the_seeded_fault(name):
    m, n_first, fault, expected = SEEDED[name]()
    ops, order = m.schedule(n_first, **fault)
    found = A.audit(ops, order, n_first)
    assert {f.key() for f in found} == expected and len(found) == len(expected), [repr(f) for f in found]
    assert found.conservative == 0
    f = found[0]
    assert {f.a["build"], f.b["build"]} == {order[f.a["pos"]], order[f.b["pos"]]} and repr(f.fa) in repr(f) and repr(f.fb) in repr(f)


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_audit_is_quiet_on_the_complete_plan(name):
    m, n_first, _, _ = SEEDED[name](False) if name == "split_ws" else SEEDED[name]()
    ops, order = m.schedule(n_first)
    found = A.audit(ops, order, n_first)
    assert not found, [repr(f) for f in found]
    assert found.pairs == len(ops) * (len(ops) - 1) // 2 and found.conservative == 0


def test_channel_slices_of_one_buffer_are_disjoint():
    """Two group mates writing slices [0, 64) and [64, 128) of one wide buffer, and a mate reading [0, 64) of a buffer while another writes
    its [64, 128): same address range, no float in common."""
    m = Mini()
    a, b, wide, cat, y = m.buffer(64), m.buffer(64), m.buffer(128), m.buffer(128), m.buffer(64)
    m.add(m.conv(a, 64, 64, wide, 64, 128), [(a, 0, 64)], [(wide, 0, 64)])
    m.add(m.conv(b, 64, 64, wide + 4 * 64, 64, 128), [(b, 0, 64)], [(wide, 64, 128)])
    m.add(m.conv(cat, 64, 128, y, 64, 64), [(cat, 0, 64)], [(y, 0, 64)])
    m.add(m.conv(a, 64, 64, cat + 4 * 64, 64, 128), [(a, 0, 64)], [(cat, 64, 128)])
    ops, order = m.schedule()
    assert len({op.group for op in ops}) == 1 and ops[0].group != 0, "one launch group"
    found = A.audit(ops, order, 0)
    assert not found and found.groups == 1 and found.largest_group == 4 and found.decided >= 2 and found.conservative == 0, found.summary()
    # ... and the same slices one channel wider do meet
    wr = lambda op: A.footprints(op)[1][0]
    f0, f1 = wr(ops[order.index(0)]), wr(ops[order.index(1)])
    assert not A.conflict(f0, f1)
    wider = A.Footprint(f0.base, f0.pixels, f0.cs, 0, 65, "out")
    assert A.conflict(wider, f1) and A.conflict(f1, wider)


def test_conflict_is_exact():
    """Against brute force over small strided sets, pixel counts and offsets (the window may wrap past the stride: a view at c0 > 0)."""
    import itertools

    import numpy as np

    def floats(f):
        return set(f.indices(0).tolist())

    rng = np.random.default_rng(0)
    n = 0
    for cs, pa, pb in itertools.product((4, 7), (1, 3), (1, 2, 4)):
        for _ in range(60):
            a_lo, b_lo = int(rng.integers(0, cs)), int(rng.integers(0, cs))
            a = A.Footprint(100, pa, cs, a_lo, a_lo + int(rng.integers(1, cs)), "a")
            b = A.Footprint(100 + int(rng.integers(-2 * cs, 3 * cs)), pb, cs, b_lo, b_lo + int(rng.integers(1, cs)), "b")
            assert A.conflict(a, b) == bool(floats(a) & floats(b)) == A.conflict(b, a), (a, b)
            n += 1
    assert n == 720
    d = A.dense(400, 10, "d")
    assert A.conflict(d, A.dense(436, 1, "e")) and not A.conflict(d, A.dense(440, 1, "e"))
    cnt = [0]
    assert A.conflict(A.Footprint(0, 4, 8, 0, 4, "a"), A.Footprint(0, 4, 16, 8, 12, "b"), cnt) and cnt == [1], "different strides: conservative, and counted"


def test_every_accepted_kind_has_a_footprint():
    """idh_run_ops accepts the kinds of the two tables + IDH_OP_STEM; footprints() knows each (the stem's strided batch view on the host)."""
    from implicit_depth_amd import _lib, nhwc

    kinds = {A.OP_CONV} | {KR.KINDS[s.kind][0] for s in KR.CASES}
    assert kinds | {A.OP_STEM} == set(A.KIND_NAMES) == set(KR.declared_kinds().values()) - {5}
    op = nhwc.Op()
    op.kind, op.N, op.Ho, op.Wo, op.out_cs, op.out = A.OP_STEM, 6, 4, 6, 64, 1 << 30
    s = op.src[0]
    s.in_, s.w, s.H, s.W, s.up_C, s.up_cs[0], s.up_cs[1] = 1 << 20, 1 << 28, 16, 24, 3, 2 * 3 * 16 * 24, 10 * 3 * 16 * 24
    reads, writes = A.footprints(op)
    img = 3 * 16 * 24
    assert [(f.lo - (1 << 18), f.count) for f in reads[:-1]] == [(g * 10 * img + k * 2 * img, img) for g in range(2) for k in range(3)]
    assert reads[-1].role == A.WEIGHT and reads[-1].count == _lib.lib().idh_stem_weight_floats()
    assert len(writes) == 1 and writes[0].count == 6 * 4 * 6 * 64
    s.up_C = s.up_cs[0] = s.up_cs[1] = 0  # one group of N dense images
    assert [(f.lo, f.count) for f in A.footprints(op)[0][:-1]] == [(1 << 18, 6 * img)]


# ----------------------------------------------------------------------------------------------------------------------------------------
# the C++ builder's plans
# ----------------------------------------------------------------------------------------------------------------------------------------
def _rewritten(plan):
    """Writes to an output view some earlier op wrote already: only an activation buffer that aliases an earlier, dead one gets any."""
    outs = [op.out for op in plan.ops if op.kind != 4]  # (exports write the caller's tensors)
    return len(outs) - len(set(outs))


def _check(plan, label):
    found = plan.audit()
    print(f"{label}: {found.summary()}")
    assert not found, [repr(f) for f in found[:8]]
    assert found.conservative == 0
    return found


# plan_key of every configuration of test_sizes_cover_shipped_configs before the made-up addresses of the size query moved (it hashes no pointer)
PLAN_KEYS = {
    ("mlp", "bd", False): (9420045795984967724, 18218469603498083352, 6508761130980094407),
    ("mlp", "bd", True): (1730167218501153122, 13935085555932181420, 9563024981266388328),
    ("mlp", "depth", False): (2602241845753211618, 8886086688253491631, 18160384492185746315),
    ("dot", "depth", False): (17499591246687303249, 9042646735167799886, 4012616310564595097),
    ("dot", "bd", False): (5227985214023449100, 10541169052799502865, 11373118092932410724),
}


@pytest.mark.parametrize("volume,decoder,use_prior", CONFIGS)
def test_model_plans_are_clean(volume, decoder, use_prior):
    from implicit_depth_amd import model_abi as m

    e = _entry(volume, decoder, use_prior, with_head=True)
    pm = m.PRIOR_INPUTS if use_prior else m.PRIOR_NONE
    for bi, B in enumerate((1, 4, 32)):
        for mi in (m.MATCH_FEATS_NCHW, m.MATCH_LAYER1_NCHW):
            d = e.desc(B, 7, 16, 96, 128, P=2, prior_mode=pm, matching_input=mi)
            with A.observe() as plans:
                s = e.sizes(d, B)
            assert len(plans) == 1
            p = plans[0]
            if mi == m.MATCH_FEATS_NCHW:
                assert s.plan_key == PLAN_KEYS[(volume, decoder, use_prior)][bi]
            found = _check(p, f"model {volume}/{decoder}/prior={use_prior} B={B} head={mi != m.MATCH_FEATS_NCHW}")
            assert len(p.ops) == s.conv_ops and (p.n_first > 0) == (mi != m.MATCH_FEATS_NCHW)
            assert p.ws[1] <= s.workspace_floats and p.blob[1] <= s.weight_floats, "the conv stage is the head of the model's workspace and blob"
            # not vacuous
            assert sum(op.kind == A.OP_CONV for op in p.ops) > 100 and found.largest_group >= 2 and found.decided > 100
            if B == 32:
                assert _rewritten(p) >= 1, "recycled activation buffers at B = 32"
    with A.observe() as plans:
        pass
    e.sizes(e.desc(1, 7, 16, 96, 128, P=2, prior_mode=pm), 1)
    assert not plans, "the hook is cleared"


def _net_plans():
    """(label, call -> (rc, NetSizes)) for the *_sizes entries of include/idh_net.h at the shapes of tests/test_net_abi_gpu.py (+ the
    matching stem at the two sizes of tests/test_matching_stem_cpu.py)."""
    from implicit_depth_amd import _lib
    from implicit_depth_amd import net_abi as na
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.layers import BasicBlock

    L = _lib.lib()
    keep = []
    out = []

    def add(label, fn):
        s = na.NetSizes()
        out.append((label, lambda: (fn(s), s)))

    for tag, (cin, cout, stride) in (("id", (24, 24, 1)), ("proj", (24, 40, 1)), ("down", (24, 40, 2))):
        blk = na.block_params(BasicBlock(cin, cout, stride), keep)
        Ho, Wo = (12 - 1) // stride + 1, (20 - 1) // stride + 1
        add(f"basic_block {tag} nchw", lambda s, blk=blk, cout=cout, Ho=Ho, Wo=Wo: L.idh_basic_block_sizes(
            C.byref(blk), 2, C.byref(na.nchw(None, 24, 12, 20)), C.byref(na.nchw(None, cout, Ho, Wo)), C.byref(s)))
        add(f"basic_block {tag} nhwc", lambda s, blk=blk, cout=cout, Ho=Ho, Wo=Wo: L.idh_basic_block_sizes(
            C.byref(blk), 2, C.byref(na.nhwc(None, 24, 12, 20, 32)), C.byref(na.nhwc(None, cout, Ho, Wo, cout + 16)), C.byref(s)))
    chans = [64, 128, 256, 384]
    for N, D, Hm, Wm in ((1, 16, 24, 32), (6, 64, 96, 128)):
        cve = net.CVEncoder(num_ch_cv=D, num_ch_enc=[48, 64, 160, 256], num_ch_outs=chans)
        blocks = na.cvencoder_blocks(cve, keep)
        imgs = na.tensors([na.nchw(None, c, Hm >> i, Wm >> i) for i, c in enumerate([48, 64, 160, 256])])
        for lay in ("nhwc", "nchw"):
            mk = na.nhwc if lay == "nhwc" else na.nchw
            cost = mk(None, D, Hm, Wm)
            outs = na.tensors([mk(None, c, Hm >> i, Wm >> i) for i, c in enumerate(chans)])
            add(f"cvencoder N={N} {Hm}x{Wm} {lay}", lambda s, b=blocks, N=N, cost=cost, imgs=imgs, outs=outs: L.idh_cvencoder_sizes(
                b, 4, N, C.byref(cost), imgs, outs, C.byref(s)))
        for cls in (net.BDDecoderPP, net.DepthDecoderPP):
            blocks_d, heads = na.unetpp_blocks(cls([24, 64, 128, 256, 384]), keep)
            H0, W0 = 2 * Hm, 2 * Wm
            fouts = na.tensors([na.nhwc(None, c, H0 >> i, W0 >> i) for i, c in enumerate([64, 64, 128, 256])])
            for l0 in ("nchw", "nhwc"):
                f0 = na.nchw(None, 24, H0, W0) if l0 == "nchw" else na.nhwc(None, 24, H0, W0, 32)
                feats = na.tensors([f0] + [na.nhwc(None, c, H0 >> (i + 1), W0 >> (i + 1)) for i, c in enumerate(chans)])
                add(f"unetpp {cls.__name__} N={N} {H0}x{W0} level0 {l0}", lambda s, b=blocks_d, h=heads, N=N, feats=feats, fouts=fouts: L.idh_unetpp_sizes(
                    b, na.UNETPP_BLOCKS, h, N, feats, fouts, C.byref(s)))
                if heads is None:
                    for mask in (0b0101, 0b0000):  # pruned scales: reserve_block takes blob slots and builds no op
                        add(f"unetpp_ex mask {mask:04b} N={N} {H0}x{W0} level0 {l0}", lambda s, b=blocks_d, N=N, feats=feats, fouts=fouts, mask=mask:
                            L.idh_unetpp_sizes_ex(b, na.UNETPP_BLOCKS, None, N, feats, fouts, mask, C.byref(s)))
    sp = na.stem_params(net.ResnetMatchingEncoder(None).eval().net[:5], keep)
    for N, Hi, Wi in ((16, 384, 512), (1, 8, 8)):
        add(f"matching_stem N={N} {Hi}x{Wi}", lambda s, N=N, Hi=Hi, Wi=Wi: L.idh_matching_stem_sizes(
            C.byref(sp), N, C.byref(na.nchw(None, 3, Hi, Wi)), C.byref(na.nhwc(None, 64, Hi // 4, Wi // 4, 64)), C.byref(s)))
    out.append(keep)
    return out


def test_net_plans_are_clean():
    *calls, keep = _net_plans()
    assert len(calls) == 6 + 2 * (2 + 4 + 4) + 2
    recycled = groups = 0
    for label, call in calls:
        with A.observe() as plans:
            rc, s = call()
        assert rc == 0 and len(plans) == 1, (label, rc)
        p = plans[0]
        found = _check(p, label)
        assert (p.ws[1], p.blob[1], len(p.ops)) == (s.workspace_floats, s.weight_floats, s.ops), label
        # (a recycled buffer may have several writers - the slices of a concat buffer - so the count seen in the plan is no smaller)
        assert _rewritten(p) >= s.recycled and (_rewritten(p) > 0) == (s.recycled > 0), label
        recycled += s.recycled
        groups += found.groups
    assert recycled >= 1 and groups >= 10, "not vacuous: recycled buffers and launch groups among the audited plans"
