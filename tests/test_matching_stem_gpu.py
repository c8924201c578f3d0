"""The native ResNet18 matching stem on the MI355X: IDH_OP_STEM alone, the whole native ResnetMatchingEncoder, batch independence,
dropin.fused_forward(native_matching_stem=True) against the same modules run in torch, and the C entry idh_matching_stem_fwd.
Reference for every comparison: torch's float64 CPU composition of the same modules in eval mode (random non-trivial BatchNorm
statistics, random images), scale-relative error against TOL."""
import ctypes

import pytest
import torch
from torch import nn

import implicit_depth_amd.synthetic as syn
from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu


def _randomise_bns(mods, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mods.modules() if isinstance(mods, nn.Module) else [x for mm in mods for x in mm.modules()]:
            if isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(1.0 + 0.3 * torch.randn(c, generator=g))
                m.bias.copy_(0.2 * torch.randn(c, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(c, generator=g))
                m.running_var.copy_(0.5 + torch.rand(c, generator=g))
                m.eps = 1e-5


def _encoder(seed=3, num_ch_out=16):
    from implicit_depth_amd import networks as net

    e = net.ResnetMatchingEncoder(None, num_ch_out)
    syn.fill_state_dict(e, seed=seed, gain=1.4)
    _randomise_bns(e, seed)
    return e.eval()


def _images(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _ref(e, x, upto):
    """float64 CPU composition of e.net[:upto] (eval mode)."""
    from implicit_depth_amd import networks as net

    m = net.ResnetMatchingEncoder(None, e.num_ch_out).double().eval()
    m.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.cpu() for k, v in e.state_dict().items()})
    y = x.double()
    with torch.no_grad():
        for i in range(upto):
            y = m.net[i](y)
    return y


def _run_stem_op(e, images, out_buf, c0):
    """IDH_OP_STEM alone through a Plan, written into channels [c0, c0 + 64) of ``out_buf`` (N, Ho, Wo, cs)."""
    from implicit_depth_amd import nhwc

    fs = nhwc.folded_stem(e, images.device)
    imgs, shape, strides = nhwc.image_strides(images)
    p = nhwc.Plan(images.device)
    idx = p.stem(shape, strides, fs.blob, nhwc.View(out_buf, c0, 64))
    p.set_in(idx, imgs)
    p.run()
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,H,W", [(2, 384, 512), (9, 100, 140), (3, 8, 8), (2, 190, 254)])
def test_stem_kernel_alone(N, H, W):
    e = _encoder()
    x = _images((N, 3, H, W), seed=H + W)
    ref = _ref(e, x, 4).permute(0, 2, 3, 1)  # conv1, bn1, relu, maxpool+blur -> NHWC
    Ho, Wo = ((H + 1) // 2) // 2, ((W + 1) // 2) // 2
    assert ref.shape == (N, Ho, Wo, 64)
    out = torch.full((N, Ho, Wo, 64), float("nan"), device="cuda")
    _run_stem_op(e.cuda(), x.cuda(), out, 0)
    err = rel_err(out.cpu(), ref)
    print(f"stem {N}x{H}x{W}: scale-rel err {err:.2e}")
    assert err < TOL


def test_stem_kernel_strided_batch_view_and_channel_slice():
    e = _encoder().cuda()
    B, K1, H, W = 2, 4, 100, 140
    big = _images((B, K1 + 2, 3, H, W), seed=7).cuda()
    view = big[:, 1:K1 + 1]  # (B, K+1, 3, H, W) with a group stride of K+2 images
    assert not view.is_contiguous()
    Ho, Wo = ((H + 1) // 2) // 2, ((W + 1) // 2) // 2
    out = torch.full((B * K1, Ho, Wo, 96), -7.0, device="cuda")
    _run_stem_op(e, view, out, 16)
    ref = _ref(e, view.reshape(B * K1, 3, H, W).cpu(), 4).permute(0, 2, 3, 1)
    err = rel_err(out[..., 16:80].cpu(), ref)
    print(f"stem strided view into a channel slice: scale-rel err {err:.2e}")
    assert err < TOL
    assert bool((out[..., :16] == -7.0).all()) and bool((out[..., 80:] == -7.0).all())


@pytest.mark.parametrize("channels_last", [False, True])
def test_native_encoder_matches_torch_float64(channels_last):
    e = _encoder()
    x = _images((3, 3, 384, 512), seed=11)
    ref = _ref(e, x, 10)
    got = e.cuda()(x.cuda(), channels_last=channels_last)
    torch.cuda.synchronize()
    if channels_last:
        got = got.permute(0, 3, 1, 2)
    err = rel_err(got.cpu(), ref)
    l1 = e.backbone(x.cuda())
    err1 = rel_err(l1.cpu(), _ref(e, x, 5))
    print(f"native encoder (channels_last={channels_last}): scale-rel err {err:.2e}; layer1 map {err1:.2e}")
    assert err < TOL and err1 < TOL


def test_batch_independence():
    e = _encoder().cuda()
    x = _images((256, 3, 384, 512), seed=13).cuda()
    full = e.backbone(x)
    one = e.backbone(x[77:78].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(one[0], full[77])  # the stem pass and layer1's four F(4x4) convs at N = 1 and N = 256


class _RunOpts:
    matching_scale = 1
    min_matching_depth = 0.25
    max_matching_depth = 5.0
    use_prior = False


def _model(K, decoder, seed):
    from implicit_depth_amd import backbone
    from implicit_depth_amd import cost_volume as cv
    from implicit_depth_amd import networks as net

    m = nn.Module()
    m.encoder = syn.StubImageEncoder()
    H, W, D = 96, 128, 16
    m.cost_volume = cv.FeatureVolumeManager(H, W, D, num_source_views=K)
    m.matching_model = net.ResnetMatchingEncoder(backbone.resnet18_stem(), 16)  # torch-module stem: the current path
    m.cost_volume_net = net.CVEncoder(D, [48, 64, 160, 256], [64, 128, 256, 384])
    if decoder == "bd":
        m.depth_decoder = net.BDDecoderPP([24] + m.cost_volume_net.num_ch_enc)
        m.binary_mlp = net.BinaryMLPNetwork(m.depth_decoder.num_ch_dec, mlp_size=128, use_prior=False)
    else:
        m.depth_decoder = net.DepthDecoderPP([24] + m.cost_volume_net.num_ch_enc)
    m.run_opts = _RunOpts()
    m.thresholder = None
    syn.fill_state_dict(m, seed=seed)
    _randomise_bns(m.matching_model, seed)
    return m.cuda().eval()


@pytest.mark.parametrize("decoder", ["bd", "depth"])
def test_fused_forward_native_stem_matches_torch_stem(decoder):
    from implicit_depth_amd import _lib
    from implicit_depth_amd.dropin import fused_forward

    K = 7
    m = _model(K, decoder, seed=40)
    cur, src = syn.frame_tuple(1, K, 384, 512, seed=41, P=3)
    cur = {k: v.cuda() for k, v in cur.items()}
    src = {k: v.cuda() for k, v in src.items()}
    ref = fused_forward(m)("test", cur, src, return_mask=True)
    nat = fused_forward(m, native_matching_stem=True)("test", cur, src, return_mask=True)
    torch.cuda.synchronize()
    if decoder == "bd":
        err = rel_err(nat["pred_0"].cpu(), ref["pred_0"].cpu())
        mask = (nat["overall_mask_bhw"] != ref["overall_mask_bhw"]).float().mean().item()
        print(f"fused_forward BDModel native stem vs torch stem: pred_0 {err:.2e}, mask disagreement {mask:.1e}")
        assert err < TOL and mask < 2e-3
        r2 = fused_forward(m)("test", cur, src, infer_depth=True)
        n2 = fused_forward(m, native_matching_stem=True)("test", cur, src, infer_depth=True)
        agree = ((n2["search_depths"] - r2["search_depths"]).abs() < 1e-6).float().mean().item()
        print(f"infer_depth: identical search depths at {agree:.4f} of the pixels")
        assert agree > 0.98  # the rest: knife-edge pixels whose last search steps sit within fp32 noise of the threshold
    else:
        for i in range(4):
            err = rel_err(nat[f"log_depth_pred_s{i}_b1hw"].cpu(), ref[f"log_depth_pred_s{i}_b1hw"].cpu())
            print(f"fused_forward DepthModel native stem vs torch stem: log_depth s{i} {err:.2e}")
            assert err < TOL
    m.matching_model.net[1].train()
    with pytest.raises(_lib.IdhError):
        fused_forward(m, native_matching_stem=True)("test", cur, src)


def test_c_entry_is_bit_identical_to_the_python_path():
    """idh_matching_stem_fwd (NHWC, cs = 64: what idh_model_fwd reads as IDH_MATCH_LAYER1_NHWC) gives the layer1 map of
    nhwc.build_matching_stem bit for bit, and HotPath fed that map channels-last (the model entry's layer1 path) equals HotPath on the
    raw images."""
    from implicit_depth_amd import _lib, net_abi, nhwc
    from implicit_depth_amd.dropin import hot_path_of

    K, B, H, W = 7, 2, 384, 512
    m = _model(K, "bd", seed=50)
    enc = m.matching_model
    imgs = _images((B, K + 1, 3, H, W), seed=51).cuda()
    flat = imgs.reshape(B * (K + 1), 3, H, W)
    N, Ho, Wo = B * (K + 1), H // 4, W // 4
    L = _lib.lib()
    keep = []
    sp = net_abi.stem_params(enc.net[:5], keep)
    x_t, out_t = net_abi.nchw(flat), None
    l1_c = torch.empty(N, Ho, Wo, 64, device="cuda")
    out_t = net_abi.nhwc(l1_c)
    sz = net_abi.NetSizes()
    _lib.check(L.idh_matching_stem_sizes(ctypes.byref(sp), N, ctypes.byref(x_t), ctypes.byref(out_t), ctypes.byref(sz)), "sizes")
    blob = torch.empty(sz.weight_floats + 64, device="cuda")
    ws = torch.empty(sz.workspace_floats + 64, device="cuda")
    _lib.check(L.idh_matching_stem_pack(ctypes.byref(sp), N, ctypes.byref(x_t), ctypes.byref(out_t), blob.data_ptr(), _lib.stream_ptr()), "pack")
    _lib.check(L.idh_matching_stem_fwd(ctypes.byref(sp), blob.data_ptr(), N, ctypes.byref(x_t), ctypes.byref(out_t), ws.data_ptr(), sz.workspace_floats,
                                       _lib.stream_ptr()), "fwd")
    p = nhwc.Plan(flat.device)
    y, i_in = nhwc.build_matching_stem(p, enc, flat)
    p.schedule()
    p.set_in(i_in, flat)
    p.run()
    torch.cuda.synchronize()
    assert torch.equal(l1_c, y.dense())
    assert rel_err(l1_c.permute(0, 3, 1, 2).cpu(), _ref(enc, flat.cpu(), 5)) < TOL

    cur, src = syn.frame_tuple(B, K, H, W, seed=52, P=3)
    cur = {k: v.cuda() for k, v in cur.items()}
    src = {k: v.cuda() for k, v in src.items()}
    feats = list(m.encoder(imgs[:, 0].contiguous()))
    src_T = src["cam_T_world_b44"] @ cur["world_T_cam_b44"].unsqueeze(1)
    cur_T = cur["cam_T_world_b44"].unsqueeze(1) @ src["world_T_cam_b44"]
    hot = hot_path_of(m, native_matching_stem=True)
    args = (None, None, feats, src_T, cur_T, src["K_s1_b44"], cur["invK_s1_b44"])
    a = hot(*args, rendered_depth=cur["rendered_depth"], matching_images=imgs)["pred_0"]
    l1_cl = l1_c.view(B, K + 1, Ho, Wo, 64).permute(0, 1, 4, 2, 3)  # channels-last per image
    b = hot(*args, rendered_depth=cur["rendered_depth"], matching_layer1=l1_cl)["pred_0"]
    torch.cuda.synchronize()
    assert torch.equal(a, b)
