"""Decoder plans that build only the output heads the caller reads (nhwc.build_decoder(scales=...), include/idh_net.h idh_unetpp_*_ex,
HotPath._scales).  BDDecoderPP's output_1..3[0] are BasicBlocks on top of the grid nodes X(i, 4-i) (reference modules/networks.py:56-62); the
occlusion MLP reads scale 0 only (experiment_modules/bd_model.py:273-280), so a plan for it leaves those three blocks - six 3x3 convs - out.
What must hold: the ops that remain are the SAME ops (kernel, tile code, split-K), so scale 0 is bit-identical; a caller that asks for the
feature maps still gets all four, bit-identical to before; decoders whose every scale is an output are untouched.  Every case runs through the
Python plan and through the native entry."""
import ctypes as C
from collections import Counter

import pytest
import torch

import implicit_depth_amd.synthetic as syn

pytestmark = pytest.mark.gpu

CH = [24, 64, 128, 256, 384]  # the five-level pyramid: image-encoder level 0 + the four CVEncoder outputs
DEC_CH = [64, 64, 128, 256]  # BDDecoderPP's feature_s{i} channels
UNETPP_CONVS = 2 * 49  # IDH_UNETPP_BLOCKS BasicBlocks, two 3x3 convs each (a projection shortcut is a second source of conv2, not an op)
HEAD_CONVS = 2 * 3  # output_1[0], output_2[0], output_3[0]


def _decoder(cls_name="BDDecoderPP", seed=13):
    from implicit_depth_amd import networks as net

    dec = getattr(net, cls_name)(CH).cuda()
    syn.fill_state_dict(dec, seed=seed)
    return dec


def _pyramid(N, H0, W0, seed=40):
    return [syn.randn((N, c, H0 >> i, W0 >> i), seed + i, f"scales_f{i}").cuda() for i, c in enumerate(CH)]


def _sig(op):
    """What decides an op's arithmetic: kind, shapes, kernel choice - not its pointers, not its place in the schedule."""
    return (op.kind, op.N, op.Ho, op.Wo, op.Cout, op.tile_m, op.tile_n, op.split_k, op.act,
            tuple((s.Cin, s.H, s.W, s.cs, s.ks, s.stride, s.pad_mode) for s in op.src))


def _python_plan(dec, feats, scales, build=None):
    """One nhwc.Plan over NCHW imports of ``feats``, run twice (the replay meets whatever the first pass left in recycled buffers).
    Returns (plan, final, scheduled indices of the ops of the output_1..3 blocks)."""
    from implicit_depth_amd import nhwc

    p = nhwc.Plan(feats[0].device)
    views, i_in = [], []
    for f in feats:
        v = p.buffer(f.shape[0], f.shape[2], f.shape[3], f.shape[1])
        i_in.append(p.import_nchw(f.shape, v))
        views.append(v)
    head_blocks = {id(dec.convs[f"output_{i}"][0]) for i in (1, 2, 3)} if hasattr(dec, "convs") else set()
    head_ops, plain = [], p.basic_block

    def spy(x, blk, out=None):
        n0 = len(p.ops)
        y = plain(x, blk, out=out)
        if id(blk) in head_blocks:
            head_ops.extend(range(n0, len(p.ops)))
        return y

    p.basic_block = spy
    final = (build or nhwc.build_decoder)(p, dec, views, scales)
    p.schedule()
    for i, f in zip(i_in, feats):
        p.set_in(i, f)
    p.run()
    p.run()
    torch.cuda.synchronize()
    return p, final, sorted(p._idx(k) for k in head_ops)


def _native(dec, feats, scales, blob=None, pack_scales=None):
    """idh_unetpp_{sizes,pack,fwd}_ex the way a C host calls them: NCHW inputs, the four outputs written in place into NHWC tensors (NaN before
    the pass: an output the pass does not write stays NaN).  ``blob``: reuse a blob packed by an earlier call."""
    from implicit_depth_amd import _lib
    from implicit_depth_amd import net_abi as na

    L = _lib.lib()
    keep = []
    blocks, heads = na.unetpp_blocks(dec, keep)
    assert heads is None
    N, _, H0, W0 = feats[0].shape
    ft = na.tensors([na.nchw(f) for f in feats])
    outs = [torch.full((N, H0 >> i, W0 >> i, c), float("nan"), device="cuda") for i, c in enumerate(DEC_CH)]
    fouts = na.tensors([na.nhwc(t) for t in outs])
    sz = na.NetSizes()
    _lib.check(L.idh_unetpp_sizes_ex(blocks, na.UNETPP_BLOCKS, None, N, ft, fouts, scales, C.byref(sz)), "sizes_ex")
    if blob is None:
        blob = torch.empty(sz.weight_floats + 64, device="cuda")
        _lib.check(L.idh_unetpp_pack_ex(blocks, na.UNETPP_BLOCKS, None, N, ft, fouts, scales if pack_scales is None else pack_scales, blob.data_ptr(),
                                        _lib.stream_ptr()), "pack_ex")
    ws = torch.full((sz.workspace_floats + 64,), float("nan"), device="cuda")
    assert blob.data_ptr() % 256 == 0 and ws.data_ptr() % 256 == 0
    args = (ft, fouts, scales, None, None, ws.data_ptr(), sz.workspace_floats, _lib.stream_ptr())
    # a blob of another size is refused before anything is launched
    assert L.idh_unetpp_fwd_ex(blocks, na.UNETPP_BLOCKS, None, blob.data_ptr(), sz.weight_floats - 64, N, *args) == -1
    assert all(bool(torch.isnan(t).all()) for t in outs)
    for _ in range(2):
        _lib.check(L.idh_unetpp_fwd_ex(blocks, na.UNETPP_BLOCKS, None, blob.data_ptr(), sz.weight_floats, N, *args), "fwd_ex")
    torch.cuda.synchronize()
    return outs, sz.as_dict(), blob


def _nchw(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2)


def _check_pruned_against_full(N, H0, W0, expect_wino4_level0):
    from implicit_depth_amd import _lib, nhwc
    from implicit_depth_amd import net_abi as na

    dec = _decoder()
    feats = _pyramid(N, H0, W0)
    full, final_f, heads_f = _python_plan(dec, feats, nhwc.ALL_SCALES)
    one, final_1, heads_1 = _python_plan(dec, feats, 0b0001)
    assert sorted(final_f) == [0, 1, 2, 3] and sorted(final_1) == [0] and heads_1 == []
    # scale 0: bit-identical, because the ops that make it are the same ops with the same tile codes
    f0 = final_f[0].dense().clone()
    assert bool(torch.isfinite(f0).all()) and torch.equal(final_1[0].dense(), f0)
    sig_f, sig_1 = [_sig(op) for op in full.ops], [_sig(op) for op in one.ops]
    gone = [full.ops[k] for k in heads_f]
    assert len(gone) == HEAD_CONVS and all(op.kind == nhwc.OP_CONV for op in gone)
    assert Counter(sig_f) - Counter(sig_1) == Counter(_sig(op) for op in gone) and not Counter(sig_1) - Counter(sig_f)
    convs = lambda p: [op for op in p.ops if op.kind == nhwc.OP_CONV]
    assert (len(convs(full)), len(convs(one))) == (UNETPP_CONVS, UNETPP_CONVS - HEAD_CONVS)  # (d) exactly six conv ops fewer
    level0 = lambda p: [op for op in convs(p) if (op.Ho, op.Wo) == (H0, W0)]
    assert len(level0(full)) == len(level0(one)) > 0
    for p in (full, one):
        assert all((op.tile_m == nhwc.TILE_WINO4) == expect_wino4_level0 for op in level0(p) if op.src[0].Cin > 16), "level 0's kernel family"
    # (d) launches: the full schedule without the six head ops is the pruned schedule, and idh_count_launches says so
    rest = [op for k, op in enumerate(full._array()) if k not in set(heads_f)]
    arr = (nhwc.Op * len(rest))(*rest)
    drop = full.count_launches() - one.count_launches()
    assert _lib.lib().idh_count_launches(C.cast(arr, C.c_void_p), len(rest)) == one.count_launches() and 0 <= drop <= HEAD_CONVS
    print(f"N={N} {H0}x{W0}: python plan {len(full.ops)} -> {len(one.ops)} ops, {full.count_launches()} -> {one.count_launches()} launches, "
          f"recycled {full.recycled} -> {one.recycled}")

    # the native entry: same results as the Python plan, and one blob for both masks
    outs_f, sz_f, blob = _native(dec, feats, na.SCALES_ALL)
    outs_1, sz_1, _ = _native(dec, feats, 0b0001, blob=blob)  # the blob packed under the other mask
    print(f"native: all scales {sz_f}; scale 0 only {sz_1}")
    assert torch.equal(_nchw(outs_f[0]), _nchw(f0)) and torch.equal(outs_1[0], outs_f[0])
    for i in (1, 2, 3):
        assert torch.equal(_nchw(outs_f[i]), _nchw(final_f[i].dense())), f"scale {i}: same op list as the Python plan"
        assert bool(torch.isnan(outs_1[i]).all()), f"scale {i} is not written by the scale-0 plan"
    assert (sz_f["ops"], sz_1["ops"]) == (len(full.ops), len(one.ops)) and sz_f["weight_floats"] == sz_1["weight_floats"]
    assert sz_f["launches"] - sz_1["launches"] == drop, "idh_count_launches of the pruned native plan"
    assert sz_1["workspace_floats"] < sz_f["workspace_floats"]
    return dec, feats, outs_f, blob


def test_scale0_plan_is_bit_identical_at_the_smallest_size():
    """(a) + (d): level 0 at 32x32 (level 4 is 2x2: the smallest pyramid the x2 steps allow), one frame, direct / LDS-staged kernels only."""
    from implicit_depth_amd import net_abi as na

    dec, feats, outs_f, _ = _check_pruned_against_full(1, 32, 32, expect_wino4_level0=False)
    # the other direction: a blob packed under the scale-0 mask holds the output blocks' weights as well
    outs, _, _ = _native(dec, feats, na.SCALES_ALL, pack_scales=0b0001)
    for i in range(4):
        assert torch.equal(outs[i], outs_f[i]), i
    # and a mask in between: scales 0 and 2
    outs, sz, _ = _native(dec, feats, 0b0101)
    assert torch.equal(outs[0], outs_f[0]) and torch.equal(outs[2], outs_f[2]) and bool(torch.isnan(outs[1]).all() and torch.isnan(outs[3]).all())


def test_scale0_plan_is_bit_identical_where_level0_runs_on_wino4():
    """(b): the smallest batch at which level 0 (32x32, 64 channels: one 8x32-pixel tile per row of tiles, 4 x 1 x 1 tiles per frame) reaches
    WINO4_MIN_TILES = 768 by itself - 192 frames - so the top level runs conv3x3_wino4_k and its 192-channel concat buffers (144 MiB) are above
    REUSE_MIN_BYTES: Plan.release hands them to later blocks, in the full plan and in the pruned one."""
    from torch import nn

    from implicit_depth_amd import nhwc

    class V:
        pass

    c64 = nn.Conv2d(64, 64, 3, 1, 1)
    B = next(n for n in range(1, 4096) if nhwc.wino4_eligible([(V(), c64)], 64, n, 32, 32, nhwc.PAD_ZEROS, nhwc.ACT_LRELU))
    assert B == nhwc.WINO4_MIN_TILES // 4 == 192
    _check_pruned_against_full(B, 32, 32, expect_wino4_level0=True)


def _hot_path(decoder="BDDecoderPP", seed=0):
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from implicit_depth_amd.pipeline import HotPath

    B, K, H, W, D, P = 1, 2, 16, 16, 16, 2  # decoder level 0 = 32x32
    cve = net.CVEncoder(D, [48, 64, 160, 256], [64, 128, 256, 384])
    dec = getattr(net, decoder)([24] + cve.num_ch_enc)
    mlp = net.BinaryMLPNetwork(dec.num_ch_dec) if decoder != "DepthDecoderPP" else None
    for i, m in enumerate([cve, dec] + ([mlp] if mlp is not None else [])):
        syn.fill_state_dict(m, seed=seed + 60 + i)
    model = HotPath(CostVolumeManager(H, W, D), cve, dec, mlp).cuda()
    inp = {k: v.cuda() for k, v in syn.cost_volume_inputs(B, K, 16, H, W, seed=seed).items()}
    pyr = [t.cuda() for t in syn.encoder_pyramid(B, H * 4, W * 4, seed=seed)]
    rd = syn.rendered_depth_planes(B, H * 2, W * 2, P).cuda() if mlp is not None else None

    def call(**kw):
        return model(inp["cur_feats"], inp["src_feats"], pyr, inp["src_extrinsics"], inp["src_poses"], inp["src_Ks"], inp["cur_invK"],
                     rendered_depth=rd, **kw)

    return model, call


def _plan_convs(ent):
    from implicit_depth_amd import nhwc

    return sum(op.kind == nhwc.OP_CONV for op in ent["plan"].ops)


CVENC_CONVS = 2 * 12  # four levels of ds_conv, conv[0], conv[1]


def test_return_features_builds_the_full_plan_on_demand():
    """(c): a plain call builds the scale-0 plan; return_features=True on the same module then builds the full plan next to it and returns all
    four maps, bit-identical to a module that was only ever asked for them."""
    model, call = _hot_path()
    plain = call(return_mask=True)
    assert [_plan_convs(e) for e in model._plans.values()] == [CVENC_CONVS + UNETPP_CONVS - HEAD_CONVS]
    assert not any(k.startswith("feature_s") for k in plain)
    feat = call(return_mask=True, return_features=True)
    assert sorted(_plan_convs(e) for e in model._plans.values()) == [CVENC_CONVS + UNETPP_CONVS - HEAD_CONVS, CVENC_CONVS + UNETPP_CONVS]
    fresh_model, fresh_call = _hot_path()
    fresh = fresh_call(return_mask=True, return_features=True)
    assert [_plan_convs(e) for e in fresh_model._plans.values()] == [CVENC_CONVS + UNETPP_CONVS]
    for i in range(4):
        k = f"feature_s{i}_b1hw"
        assert feat[k].shape[1] == DEC_CH[i] and bool(torch.isfinite(feat[k]).all()) and torch.equal(feat[k], fresh[k]), k
    assert torch.equal(plain["pred_0"], fresh["pred_0"]) and torch.equal(feat["pred_0"], fresh["pred_0"])
    # alternating callers replay the two cached plans
    ids = sorted(id(e["plan"]) for e in model._plans.values())
    assert torch.equal(call(return_mask=True)["pred_0"], plain["pred_0"])
    assert torch.equal(call(return_mask=True, return_features=True)["feature_s3_b1hw"], fresh["feature_s3_b1hw"])
    assert sorted(id(e["plan"]) for e in model._plans.values()) == ids


def test_decoders_whose_every_scale_is_an_output_are_unchanged():
    """(e): DepthDecoderPP (four 1x1 heads on output_i[0]) and the skip decoders (scale i feeds scale i-1) keep every op, whatever is asked."""
    from implicit_depth_amd import networks as net
    from implicit_depth_amd import nhwc

    model, call = _hot_path("DepthDecoderPP")
    out = call()
    assert [_plan_convs(e) for e in model._plans.values()] == [CVENC_CONVS + UNETPP_CONVS]
    assert all(bool(torch.isfinite(out[f"log_depth_pred_s{i}_b1hw"]).all()) for i in range(4))
    feats = _pyramid(1, 32, 32)
    ddec = _decoder("DepthDecoderPP")
    p_all, final_all, _ = _python_plan(ddec, feats, nhwc.ALL_SCALES, build=nhwc.build_any_decoder)
    assert sorted(final_all) == [0, 1, 2, 3] and sum(op.kind == nhwc.OP_CONV for op in p_all.ops) == UNETPP_CONVS
    SKIP_CONVS = 4 * 2 * 2  # four ConvUpsampleAndConcatBlocks: two ConvBlocks of two 3x3 convs
    for cls in (net.SkipDecoder, net.SkipDecoderRegression):
        sdec = cls(CH).cuda()
        syn.fill_state_dict(sdec, seed=17)
        p_all, final_all, _ = _python_plan(sdec, feats, nhwc.ALL_SCALES, build=nhwc.build_any_decoder)
        p_one, final_one, _ = _python_plan(sdec, feats, 0b0001, build=nhwc.build_any_decoder)
        assert [_sig(op) for op in p_one.ops] == [_sig(op) for op in p_all.ops] and sorted(final_one) == [0, 1, 2, 3]
        assert sum(op.kind == nhwc.OP_CONV for op in p_all.ops) == SKIP_CONVS
        for i in range(4):
            assert torch.equal(final_one[i].dense(), final_all[i].dense())
    # a skip decoder behind the occlusion MLP: HotPath asks for scale 0 and the plan is still whole
    model, call = _hot_path("SkipDecoder")
    assert bool(torch.isfinite(call()["pred_0"]).all())
    assert [_plan_convs(e) for e in model._plans.values()] == [CVENC_CONVS + SKIP_CONVS]
