"""What the two plan builders promise about recording an op and about the arguments of an entry point, host side.

nhwc.Plan: every recorder goes through ``Plan._record`` - one op, one meta entry, the cached ctypes array dropped, the documented return
value - and an index handed out before ``schedule()`` addresses the same op afterwards.  csrc/networks.hip: the pointer checks every
``extern "C"`` network entry makes before it builds anything, and the two places where an entry differs from its siblings.  Nothing is
launched: the plans live on the CPU and the entry points are given made-up aligned addresses on paths that return before the pass."""
import ctypes as C

import pytest
import torch

EINVAL, EWORKSPACE = -1, -4  # include/idh.h


# ----------------------------------------------------------------------------------------------------------------------------------------
# nhwc.Plan recorders
# ----------------------------------------------------------------------------------------------------------------------------------------
def _record(name, p):
    """Calls one recorder on plan ``p``: (what it returned, what its docstring says it returns, the op kind)."""
    from implicit_depth_amd import nhwc

    x = p.buffer(2, 4, 8, 16)
    if name in ("upsample2", "upsample2_nearest"):
        out = p.buffer(2, 8, 16, 32).slice(16, 16)
        return p.upsample2(x, out, nearest=name == "upsample2_nearest"), out, nhwc.OP_UPSAMPLE2_NEAREST if name == "upsample2_nearest" else nhwc.OP_UPSAMPLE2
    if name == "copy":
        out = p.buffer(2, 4, 8, 32).slice(0, 16)
        return p.copy(x, out), out, nhwc.OP_COPY
    if name == "import_nchw":
        return p.import_nchw((2, 16, 4, 8), x), len(p.ops) - 1, nhwc.OP_IMPORT
    if name == "export_nchw":
        return p.export_nchw(x), len(p.ops) - 1, nhwc.OP_EXPORT
    if name == "instance_norm":
        out = p.buffer(2, 4, 8, 16)
        return p.instance_norm(x, out, act=nhwc.ACT_LRELU), out, nhwc.OP_INSTNORM
    assert name == "instance_norm_stats"
    return p.instance_norm(x, None), "stats", nhwc.OP_INSTNORM


@pytest.mark.parametrize("name", ["upsample2", "upsample2_nearest", "copy", "import_nchw", "export_nchw", "instance_norm", "instance_norm_stats"])
def test_recorder_contract(name):
    from implicit_depth_amd import nhwc

    p = nhwc.Plan(torch.device("cpu"))
    p.export_nchw(p.buffer(1, 2, 2, 16))  # (an op before: the index a recorder returns is not just 0)
    n = len(p.ops)
    stale = p._array()
    assert p._arr is stale and len(stale) == n
    got, want, kind = _record(name, p)
    assert len(p.ops) == n + 1 and len(p.meta) == n + 1, "exactly one op and one meta entry"
    assert p._arr is None and len(p._array()) == n + 1, "the materialised array is dropped"
    op, meta = p.ops[n], p.meta[n]
    assert op.kind == kind and set(meta) == {"reads", "writes"}
    if isinstance(want, int):
        assert got == want == n, "the op's build index"
    elif isinstance(want, str):  # statistics only: the (N, 2, C) mean / rstd tensor inside the op's workspace, and the region a consumer waits on
        assert isinstance(got, torch.Tensor) and tuple(got.shape) == (2, 2, 16) and op.out is None
        assert op.ws <= got.data_ptr() < op.ws + 4 * 2 * 2 * 2 * 16 and meta["writes"] == [(got.data_ptr(), 0, 1)]
    else:
        assert got is want and op.out == want.ptr and op.out_cs == want.cs and meta["writes"] == [nhwc._region(want)]
    if name != "import_nchw":  # (its source is the caller's tensor, patched per call)
        s = op.src[0]
        assert (s.in_, s.cs, s.H, s.W, s.Cin) == (meta["reads"][0][0], 16, 4, 8, 16) and len(meta["reads"]) == 1


def test_build_indices_survive_schedule():
    """Two independent chains, recorded interleaved: whatever order the scheduler picks, the indices returned at build time patch the ops
    they were returned for (told apart by kind and output view)."""
    from implicit_depth_amd import nhwc

    p = nhwc.Plan(torch.device("cpu"))
    a, i_a = p.input_nchw((1, 16, 4, 8))
    b = p.buffer(1, 8, 16, 16)
    p.upsample2(a, b)
    c, i_c = p.input_nchw((1, 32, 4, 8))
    i_b = p.export_nchw(b)
    i_e = p.export_nchw(c)
    assert (i_a, i_c, i_b, i_e) == (0, 2, 3, 4)
    p.schedule()
    t = {i: torch.empty(4) for i in (i_a, i_c, i_b, i_e)}
    for i in (i_a, i_c):
        p.set_in(i, t[i])
    for i in (i_b, i_e):
        p.set_out(i, t[i])
    ops = list(p._array())
    find = lambda kind, **f: [o for o in ops if o.kind == kind and all(getattr(o, k) == v for k, v in f.items())]
    (imp_a,), (imp_c,) = find(nhwc.OP_IMPORT, out=a.ptr), find(nhwc.OP_IMPORT, out=c.ptr)
    assert imp_a.src[0].in_ == t[i_a].data_ptr() and imp_c.src[0].in_ == t[i_c].data_ptr()
    exp_b, exp_c = [o for o in ops if o.kind == nhwc.OP_EXPORT and o.src[0].in_ == b.ptr], [o for o in ops if o.kind == nhwc.OP_EXPORT and o.src[0].in_ == c.ptr]
    assert exp_b[0].out == t[i_b].data_ptr() and exp_c[0].out == t[i_e].data_ptr() and len(exp_b) == len(exp_c) == 1
    assert sorted(p._pos) == list(range(5)) and [ops[p._pos[i]].kind for i in range(5)] == [nhwc.OP_IMPORT, nhwc.OP_UPSAMPLE2, nhwc.OP_IMPORT, nhwc.OP_EXPORT, nhwc.OP_EXPORT]
    print("build index -> position:", p._pos)


# ----------------------------------------------------------------------------------------------------------------------------------------
# csrc/networks.hip entry points
# ----------------------------------------------------------------------------------------------------------------------------------------
ADDR = lambda k: (1 << 40) + (k << 32)  # made-up device addresses, 256-byte aligned, never dereferenced


class _Nets:
    """Per network: call(mode, blob=, ws=, ws_floats=, sizes=, weight_floats=) with valid descriptors on made-up tensors."""

    def __init__(self):
        from implicit_depth_amd import _lib
        from implicit_depth_amd import net_abi as na
        from implicit_depth_amd import networks as net
        from implicit_depth_amd.layers import BasicBlock

        L, self.keep, k = _lib.lib(), [], iter(range(1, 100))
        nchw = lambda c, h, w: na.Tensor(ADDR(next(k)), na.LAYOUT_NCHW, c, h, w, 0)
        nhwc = lambda c, h, w: na.Tensor(ADDR(next(k)), na.LAYOUT_NHWC, c, h, w, c)
        R = C.byref
        blk, x, o = na.block_params(BasicBlock(24, 40, 2), self.keep), nchw(24, 12, 20), nchw(40, 6, 10)
        chans = [64, 128, 256, 384]
        blocks = na.cvencoder_blocks(net.CVEncoder(num_ch_cv=16, num_ch_enc=[48, 64, 160, 256], num_ch_outs=chans), self.keep)
        cost, imgs = nchw(16, 24, 32), na.tensors([nchw(c, 24 >> i, 32 >> i) for i, c in enumerate([48, 64, 160, 256])])
        outs = na.tensors([nhwc(c, 24 >> i, 32 >> i) for i, c in enumerate(chans)])
        dblocks, heads = na.unetpp_blocks(net.BDDecoderPP([24, 64, 128, 256, 384]), self.keep)
        assert heads is None
        feats = na.tensors([nchw(24, 48, 64)] + [nhwc(c, 24 >> i, 32 >> i) for i, c in enumerate(chans)])
        fouts = na.tensors([nhwc(c, 48 >> i, 64 >> i) for i, c in enumerate([64, 64, 128, 256])])
        sp = na.stem_params(net.ResnetMatchingEncoder(None).eval().net[:5], self.keep)
        img, l1 = nchw(3, 16, 16), nhwc(64, 4, 4)
        U = na.UNETPP_BLOCKS
        self.calls = {
            "basic_block": {"sizes": lambda a: L.idh_basic_block_sizes(R(blk), 2, R(x), R(o), a["sizes"]),
                            "pack": lambda a: L.idh_basic_block_pack(R(blk), 2, R(x), R(o), a["blob"], None),
                            "fwd": lambda a: L.idh_basic_block_fwd(R(blk), a["blob"], 2, R(x), R(o), a["ws"], a["ws_floats"], None)},
            "cvencoder": {"sizes": lambda a: L.idh_cvencoder_sizes(blocks, 4, 1, R(cost), imgs, outs, a["sizes"]),
                          "pack": lambda a: L.idh_cvencoder_pack(blocks, 4, 1, R(cost), imgs, outs, a["blob"], None),
                          "fwd": lambda a: L.idh_cvencoder_fwd(blocks, 4, a["blob"], 1, R(cost), imgs, outs, a["ws"], a["ws_floats"], None)},
            "unetpp": {"sizes": lambda a: L.idh_unetpp_sizes(dblocks, U, None, 1, feats, fouts, a["sizes"]),
                       "pack": lambda a: L.idh_unetpp_pack(dblocks, U, None, 1, feats, fouts, a["blob"], None),
                       "fwd": lambda a: L.idh_unetpp_fwd(dblocks, U, None, a["blob"], 1, feats, fouts, None, None, a["ws"], a["ws_floats"], None)},
            "unetpp_ex": {"sizes": lambda a: L.idh_unetpp_sizes_ex(dblocks, U, None, 1, feats, fouts, 0b0101, a["sizes"]),
                          "pack": lambda a: L.idh_unetpp_pack_ex(dblocks, U, None, 1, feats, fouts, 0b0101, a["blob"], None),
                          "fwd": lambda a: L.idh_unetpp_fwd_ex(dblocks, U, None, a["blob"], a["weight_floats"], 1, feats, fouts, 0b0101, None, None, a["ws"],
                                                               a["ws_floats"], None)},
            "matching_stem": {"sizes": lambda a: L.idh_matching_stem_sizes(R(sp), 2, R(img), R(l1), a["sizes"]),
                              "pack": lambda a: L.idh_matching_stem_pack(R(sp), 2, R(img), R(l1), a["blob"], None),
                              "fwd": lambda a: L.idh_matching_stem_fwd(R(sp), a["blob"], 2, R(img), R(l1), a["ws"], a["ws_floats"], None)},
        }

    def call(self, net, mode, **args):
        a = dict(blob=ADDR(200), ws=ADDR(201), ws_floats=1 << 20, sizes=None, weight_floats=0)
        a.update(args)
        return self.calls[net][mode](a)

    def sizes(self, net):
        from implicit_depth_amd import net_abi as na

        s = na.NetSizes()
        assert self.call(net, "sizes", sizes=C.byref(s)) == 0
        return s


@pytest.fixture(scope="module")
def nets():
    return _Nets()


NETS = ["basic_block", "cvencoder", "unetpp", "unetpp_ex", "matching_stem"]


@pytest.mark.parametrize("net", NETS)
def test_entry_points_check_their_pointers_first(nets, net):
    assert nets.call(net, "sizes", sizes=None) == EINVAL
    for mode in ("pack", "fwd"):
        assert nets.call(net, mode, blob=None) == EINVAL, mode
        assert nets.call(net, mode, blob=ADDR(200) + 4) == EINVAL, mode
    if net != "basic_block":
        assert nets.call(net, "fwd", ws=None, ws_floats=1 << 20) == EINVAL
    s = nets.sizes(net)  # (... and the descriptors behind these calls are valid ones)
    assert s.ops > 0 and s.weight_floats > 0


def test_basic_block_alone_accepts_a_null_workspace_of_zero_floats(nets):
    """A BasicBlock on NHWC tensors may need no workspace, so idh_basic_block_fwd lets ws == NULL with ws_floats == 0 through to the builder -
    which here (NCHW tensors: the block needs one) answers IDH_EWORKSPACE.  Every other entry refuses a NULL workspace outright."""
    assert nets.sizes("basic_block").workspace_floats > 0
    assert nets.call("basic_block", "fwd", ws=None, ws_floats=0) == EWORKSPACE
    assert nets.call("cvencoder", "fwd", ws=None, ws_floats=0) == EINVAL


def test_unetpp_fwd_ex_checks_weight_floats_after_the_build(nets):
    s = nets.sizes("unetpp_ex")
    for off in (1, -1):
        assert nets.call("unetpp_ex", "fwd", weight_floats=s.weight_floats + off, ws_floats=s.workspace_floats) == EINVAL
    # the build comes first: a workspace one float short is its answer, whatever weight_floats says
    for wf in (s.weight_floats, s.weight_floats + 1):
        assert nets.call("unetpp_ex", "fwd", weight_floats=wf, ws_floats=s.workspace_floats - 1) == EWORKSPACE
