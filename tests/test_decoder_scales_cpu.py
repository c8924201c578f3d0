"""Decoder scale masks, host side (include/idh_net.h idh_unetpp_sizes_ex): the size query builds the plan without a GPU, so what the mask does to
the op list, the workspace and the weight blob is checked here; tests/test_decoder_scales_gpu.py runs the plans.  Reference: BDDecoderPP /
DepthDecoderPP, modules/networks.py:20-84 / :118-183 (output_1..3[0] are BasicBlocks, output_0[0] is nn.Identity)."""
import ctypes as C

import pytest


def _query(dec_cls, N, H0, W0, scales=None, level0="nchw"):
    from implicit_depth_amd import _lib
    from implicit_depth_amd import net_abi as na

    L = _lib.lib()
    keep = []
    dec = dec_cls([24, 64, 128, 256, 384])
    blocks, heads = na.unetpp_blocks(dec, keep)
    f0 = na.nchw(None, 24, H0, W0) if level0 == "nchw" else na.nhwc(None, 24, H0, W0, 32)
    feats = na.tensors([f0] + [na.nhwc(None, c, H0 >> (i + 1), W0 >> (i + 1)) for i, c in enumerate([64, 128, 256, 384])])
    fouts = na.tensors([na.nhwc(None, c, H0 >> i, W0 >> i) for i, c in enumerate([64, 64, 128, 256])])
    s = na.NetSizes()
    if scales is None:
        rc = L.idh_unetpp_sizes(blocks, na.UNETPP_BLOCKS, heads, N, feats, fouts, C.byref(s))
    else:
        rc = L.idh_unetpp_sizes_ex(blocks, na.UNETPP_BLOCKS, heads, N, feats, fouts, scales, C.byref(s))
    return rc, s.as_dict()


@pytest.mark.parametrize("N,H0,W0", [(1, 32, 32), (32, 192, 256)])
def test_scale_mask_prunes_the_output_blocks_and_keeps_the_blob(N, H0, W0):
    from implicit_depth_amd import net_abi as na
    from implicit_depth_amd import networks as net

    rc, legacy = _query(net.BDDecoderPP, N, H0, W0)
    assert rc == 0
    rc, full = _query(net.BDDecoderPP, N, H0, W0, na.SCALES_ALL)
    assert rc == 0 and full == legacy, "the plain entry is the _ex entry with every scale"
    rc, s0 = _query(net.BDDecoderPP, N, H0, W0, 0b0001)
    assert rc == 0
    # output_1..3[0]: three BasicBlocks, two 3x3 convs each; nothing else leaves the plan
    assert s0["ops"] == full["ops"] - 6
    print(f"N={N} {H0}x{W0}: all scales {full}; scale 0 only {s0}")
    assert 0 <= full["launches"] - s0["launches"] <= 6  # (grouped launches: a small conv may have shared its grid with others of its level)
    assert s0["weight_floats"] == full["weight_floats"], "the blob layout does not depend on the mask"
    assert s0["workspace_floats"] < full["workspace_floats"], "the pruned blocks' buffers are gone"
    assert s0["wino4"] + s0["wino2"] <= full["wino4"] + full["wino2"]
    for mask, blocks_gone in ((0b0011, 2), (0b0101, 2), (0b1001, 2), (0b0111, 1), (0b1110, 0), (0b0000, 3)):
        rc, s = _query(net.BDDecoderPP, N, H0, W0, mask)
        assert rc == 0 and s["ops"] == full["ops"] - 2 * blocks_gone and s["weight_floats"] == full["weight_floats"], (mask, s)


def test_scale_mask_is_refused_where_every_scale_is_an_output():
    from implicit_depth_amd import net_abi as na
    from implicit_depth_amd import networks as net

    rc, legacy = _query(net.DepthDecoderPP, 1, 32, 32)
    assert rc == 0
    rc, full = _query(net.DepthDecoderPP, 1, 32, 32, na.SCALES_ALL)
    assert rc == 0 and full == legacy
    assert _query(net.DepthDecoderPP, 1, 32, 32, 0b0001)[0] == -1  # IDH_EINVAL: the four 1x1 heads are outputs
    assert _query(net.BDDecoderPP, 1, 32, 32, 0b10001)[0] == -1  # bits beyond the four scales
