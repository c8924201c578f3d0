"""Swap the hot-path modules of a reference model for the MI355X drop-ins.

``convert(model)`` does for all four modules what the reference's own
``model.cost_volume = model.cost_volume.to_fast()`` (test_bd.py:80-81) does for one: it builds
the drop-in twin *from the structure of the module it replaces* (channel counts are read off
the layers, so no Options object is needed), copies the state_dict (names are identical), and
assigns it over the attribute.  ``BDModel.forward`` / ``DepthModel.forward`` then run unchanged.
"""
from __future__ import annotations

import torch
from torch import nn

from . import cost_volume as cv
from . import networks as net
from .pipeline import HotPath


def _device(m: nn.Module):
    for t in list(m.parameters()) + list(m.buffers()):
        return t.device
    return None


def infer_volume_dims(n_in: int):
    """(num_source_views, matching_dim_size) from the input width of the feature-volume MLP, C (K+1) + 10 K + 4
    (reference cost_volume.py:405-423): the reference keeps neither number on the module.  Unique for C in {16, 32} and
    K <= 16 (the first coincidence, 540 = 16*21 + 204 = 32*13 + 124, needs 20 views)."""
    for C in (16, 32):
        K, r = divmod(n_in - C - 4, C + 10)
        if r == 0 and 1 <= K <= 16:
            return K, C
    raise ValueError(f"cannot infer the number of source views / matching channels from an MLP input width of {n_in}")


def convert_cost_volume(ref: nn.Module) -> nn.Module:
    name = type(ref).__name__
    H, W, D = ref.matching_height, ref.matching_width, ref.num_depth_bins
    if name in ("CostVolumeManager", "EfficientCostVolumeManager"):
        new = cv.CostVolumeManager(H, W, D)
    elif name == "ZeroCostVolumeManager":
        new = cv.ZeroCostVolumeManager(H, W, D)
    elif name in ("FeatureVolumeManager", "FastFeatureVolumeManager"):
        K, C = infer_volume_dims(ref.mlp.net[0].in_features)
        new = cv.FeatureVolumeManager(H, W, D, num_source_views=K, matching_dim_size=C)
    else:
        raise ValueError(f"unrecognised cost volume class {name}")
    new.load_state_dict(ref.state_dict())
    return new.to(_device(ref))


def convert_cv_encoder(ref: nn.Module) -> nn.Module:
    n = ref.num_blocks
    outs = [ref.convs[f"ds_conv_{i}"].conv1.out_channels for i in range(n)]
    enc = [ref.convs[f"conv_{i}"][0].conv1.in_channels - outs[i] for i in range(n)]
    new = net.CVEncoder(ref.convs["ds_conv_0"].conv1.in_channels, enc, outs)
    new.load_state_dict(ref.state_dict())
    return new.to(_device(ref))


def convert_decoder(ref: nn.Module) -> nn.Module:
    if hasattr(ref, "block1"):  # SkipDecoder / SkipDecoderRegression (networks_fast.py)
        blocks = [ref.block1, ref.block2, ref.block3, ref.block4]
        outs = [b.pre_concat_conv.conv2.out_channels for b in blocks]
        enc_rev = [ref.block1.pre_concat_conv.conv1.in_channels] + [b.post_concat_conv.conv1.in_channels - o for b, o in zip(blocks, outs)]
        new = (net.SkipDecoderRegression if hasattr(ref, "out1") else net.SkipDecoder)(enc_rev[::-1])
        new.load_state_dict(ref.state_dict())
        return new.to(_device(ref))
    enc = [ref.convs[f"right_conv_{i}0"].conv1.in_channels for i in range(4)] + [ref.convs["diag_conv_40"].conv1.in_channels]
    head = len(ref.convs["output_0"]) == 2
    new = (net.DepthDecoderPP if head else net.BDDecoderPP)(enc)
    new.load_state_dict(ref.state_dict())
    return new.to(_device(ref))


def convert_binary_mlp(ref: nn.Module) -> nn.Module:
    scales = sorted(ref.mlps.keys())
    first = ref.mlps["s0"][0]
    use_prior = getattr(ref, "use_prior", None)
    widths = [ref.mlps[s][0].in_features for s in scales]
    if use_prior is None:
        use_prior = (widths[0] - 64) == 2  # scale-0 features have num_ch_dec[0] = 64 channels (networks.py:30)
    extra = 2 if use_prior else 1
    new = net.BinaryMLPNetwork([w - extra for w in widths], mlp_size=first.out_features, use_prior=use_prior)
    new.load_state_dict(ref.state_dict())
    return new.to(_device(ref))


def _check_native_stem(model: nn.Module) -> None:
    from . import _lib
    from .backbone import stem_is_native_eligible

    mm = getattr(model, "matching_model", None)
    net_ = getattr(mm, "net", None)
    if net_ is None or len(net_) != 10 or not stem_is_native_eligible(net_[:5]):
        raise _lib.IdhError("native_matching_stem=True needs a ResnetMatchingEncoder whose net[:5] is the eval-mode resnet18(filter_size=4, "
                            "pool_only=True) stem (backbone.stem_is_native_eligible)")


def convert_normal_generator(ref: nn.Module) -> nn.Module:
    from .geometry import NormalGenerator

    return NormalGenerator(ref.height, ref.width, ref.kernel_size, ref.std).to(_device(ref))


def _convert_losses(model: nn.Module) -> None:
    """``grad_loss``, ``normals_loss`` and ``mv_depth_loss`` of a DepthModel (depth_model.py:177-182) -> the modules of ``losses``."""
    from . import losses

    if all(hasattr(model, n) for n in ("grad_loss", "normals_loss", "mv_depth_loss")):
        if not isinstance(model.grad_loss, losses.MSGradientLoss):
            model.grad_loss = losses.MSGradientLoss(getattr(model.grad_loss, "num_scales", 4))
        if not isinstance(model.normals_loss, losses.NormalsLoss):
            model.normals_loss = losses.NormalsLoss()
        if not isinstance(model.mv_depth_loss, losses.MVDepthLoss):
            model.mv_depth_loss = losses.MVDepthLoss(model.mv_depth_loss.height, model.mv_depth_loss.width).to(_device(model.mv_depth_loss))


def convert(model: nn.Module, math: str = None, native_matching_stem: bool = False, native_normals: bool = False,
            native_losses: bool = False) -> nn.Module:
    """In-place: replace ``cost_volume``, ``cost_volume_net``, ``depth_decoder`` and (BDModel)
    ``binary_mlp`` of a reference model.  Idempotent.  ``math``: None keeps the default (fp32 MFMA); "f16x3" selects the split-precision
    kernels for this model's convs (and, for "f16x3", its MLP feature volume and BinaryMLP).  ``native_matching_stem``: additionally check
    that the matching encoder's ResNet18 stem can run on the native kernels (``IdhError`` if not); its modules and state dict are left
    as they are.  ``native_normals``: additionally replace ``compute_normals`` (DepthModel's ``NormalGenerator``, depth_model.py:191) by
    ``geometry.NormalGenerator`` of the same height, width, kernel size and std, so that the reference's own ``step`` produces
    ``normals_pred_b3hw`` / ``normals_b3hw`` on the fused kernel, without kornia; a model without that attribute is left as it is.
    ``native_losses``: additionally replace ``grad_loss``, ``normals_loss`` and ``mv_depth_loss`` (DepthModel, depth_model.py:177-182)
    by ``losses.MSGradientLoss`` / ``NormalsLoss`` / ``MVDepthLoss``, forward value only, so that the reference's own ``compute_losses``
    runs without kornia under ``torch.no_grad()``; a model without the three attributes is left as it is."""
    if native_losses:
        _convert_losses(model)
    if native_matching_stem:
        _check_native_stem(model)
    if native_normals and hasattr(model, "compute_normals"):
        from .geometry import NormalGenerator

        if not isinstance(model.compute_normals, NormalGenerator):
            model.compute_normals = convert_normal_generator(model.compute_normals)
    if not isinstance(model.cost_volume, cv.CostVolumeManager):
        model.cost_volume = convert_cost_volume(model.cost_volume)
    if not isinstance(model.cost_volume_net, net.CVEncoder):
        model.cost_volume_net = convert_cv_encoder(model.cost_volume_net)
    if not isinstance(model.depth_decoder, (net._DecoderPP, net.SkipDecoder)):
        model.depth_decoder = convert_decoder(model.depth_decoder)
    if hasattr(model, "binary_mlp") and not isinstance(model.binary_mlp, net.BinaryMLPNetwork):
        model.binary_mlp = convert_binary_mlp(model.binary_mlp)
    if math is not None:
        from . import nhwc

        if math not in nhwc.MATH_MODES:
            raise ValueError(f"math must be one of {nhwc.MATH_MODES}")
        mlp_math = "f16x3" if math == "f16x3" else "fp32"
        model.cost_volume_net.conv_math = model.depth_decoder.conv_math = math
        if isinstance(model.cost_volume, cv.FeatureVolumeManager):
            model.cost_volume.mlp_math = mlp_math
        if hasattr(model, "binary_mlp"):
            model.binary_mlp.mlp_math = mlp_math
    return model


def hot_path_of(model: nn.Module, min_depth: float = 0.25, max_depth: float = 5.0, math: str = None, native_matching_stem: bool = False) -> HotPath:
    """Fused pipeline sharing the (converted) modules of ``model``.  ``native_matching_stem``: see ``convert``; the caller then passes
    ``matching_images`` to the pipeline."""
    convert(model, math, native_matching_stem)
    o = getattr(model, "run_opts", None)
    if o is not None:
        min_depth, max_depth = o.min_matching_depth, o.max_matching_depth
    mm = getattr(model, "matching_model", None)
    if mm is not None and not (hasattr(mm, "net") and len(mm.net) == 10 and isinstance(mm.net[5], nn.Conv2d) and isinstance(mm.net[8], nn.Conv2d)):
        mm = None  # FPNMatchingEncoder etc.: the caller keeps running it and passes finished matching features
    hot = HotPath(model.cost_volume, model.cost_volume_net, model.depth_decoder, getattr(model, "binary_mlp", None), min_depth, max_depth,
                  conv_math=getattr(model.cost_volume_net, "conv_math", None), matching_model=mm)
    hot.thresholder = getattr(model, "thresholder", None)  # test_bd.py:103 sets it on the model for the infer_depth search
    return hot


def _reference_get_edge_mask():
    """The reference's ``utils.generic_utils.get_edge_mask``, or an ``IdhError`` that says what to do without it."""
    from . import _lib

    try:
        from utils.generic_utils import get_edge_mask
    except ImportError as e:
        raise _lib.IdhError("run_opts.bd_edge_regularision needs the reference's utils.generic_utils.get_edge_mask (kornia) on the "
                            "import path to fill inputs['edge_mask']; pass fused_forward(..., native_edge_mask=True) for the "
                            "native mask (geometry.edge_mask), or unset the option for pure inference") from e
    return get_edge_mask


def fused_forward(model: nn.Module, math: str = None, native_matching_stem: bool = False, native_edge_mask: bool = False):
    """A replacement for ``BDModel.forward`` / ``DepthModel.forward`` at inference time (bd_model.py:175-311,
    depth_model.py:280-440): same arguments, same output dictionary, but everything between the third-party backbones
    and the outputs runs as ONE fused pass of ``HotPath`` (matching-encoder head, volume, CVEncoder, decoder, occlusion
    MLP / depth heads) instead of module by module.  The third-party image encoder and ResNet18 stem still run as the
    model's own torch modules - unless ``native_matching_stem`` is set: the stem (conv1 .. layer1, which must pass
    ``backbone.stem_is_native_eligible``; ``IdhError`` otherwise) then runs on the gfx950 kernels inside the same pass, from the raw images.  ``model.forward = fused_forward(model)`` installs it; the model's config / checkpoint
    surface is untouched (the hot-path modules are converted in place and share their parameters with the pipeline).
    If ``cur_data`` carries ``sampled_rays`` (B,N,2) and ``sampled_depths`` (B,N,S), the outputs gain ``ray_pred_0..3``: the occlusion
    logits of ``BDModel.run_mlp_train`` (bd_model.py:313-387) at those rays (``HotPath.query_rays``); ``phase == "train"`` keeps raising.
    Side effects on the input dicts are the reference's: ``cur_data["prior_mask"]`` and, with ``bd_edge_regularision``,
    ``cur_data["edge_mask"]``: with ``native_edge_mask`` from ``geometry.edge_mask`` (the gfx950 kernels, no kornia, the reference never
    imported), without it from the reference's own ``get_edge_mask``, which must then be importable."""
    from . import _lib

    hot = hot_path_of(model, math=math, native_matching_stem=native_matching_stem)
    is_bd = hasattr(model, "binary_mlp")
    opts = model.run_opts
    if getattr(opts, "matching_scale", 1) != 1:
        raise _lib.IdhError("the fused forward covers matching_scale = 1: the only value the reference's BDModel / DepthModel constructors accept "
                            "(0 and 2 raise IndexError in their channel lists, bd_model.py:75-83) and the one every shipped configuration uses")

    def forward(phase, cur_data, src_data, unbatched_matching_encoder_forward=False, return_mask=False, infer_depth=False, infer_res=None):
        if phase == "train":
            raise _lib.IdhError("the fused forward is an inference path (no autograd, no flip augmentation)")
        del infer_res  # unused by the reference as well
        ms = opts.matching_scale
        cur_image, src_image = cur_data["image_b3hw"], src_data["image_b3hw"]
        src_K, cur_invK = src_data[f"K_s{ms}_b44"], cur_data[f"invK_s{ms}_b44"]
        # relative poses, bd_model.py:196-204
        src_cam_T_cur_cam = src_data["cam_T_world_b44"] @ cur_data["world_T_cam_b44"].unsqueeze(1)
        cur_cam_T_src_cam = cur_data["cam_T_world_b44"].unsqueeze(1) @ src_data["world_T_cam_b44"]
        hot.thresholder = getattr(model, "thresholder", None)
        with torch.inference_mode():
            cur_feats = list(model.encoder(cur_image))  # third-party image encoder (strong image prior), bd_model.py:218
            kw = {}
            mc = msrc = None
            if native_matching_stem:
                # the whole matching encoder (stem + layer1 + head) inside the pipeline, straight from the images; the batched and the
                # image-by-image (unbatched_matching_encoder_forward) reference orders give the same per-image results here
                _check_native_stem(model)
                kw["matching_images"] = torch.cat([cur_image.unsqueeze(1), src_image], 1)
            elif hot.matching_model is not None:
                # third-party stem on frame b's current image followed by its K source images (bd_model.py:149-160);
                # the encoder head runs inside the pipeline
                frames = torch.cat([cur_image.unsqueeze(1), src_image], 1)
                stem = model.matching_model.net[:5]
                flat = frames.flatten(0, 1)
                l1 = torch.cat([stem(f) for f in flat.split(1, 0)], 0) if unbatched_matching_encoder_forward else stem(flat)
                kw["matching_layer1"] = l1.unflatten(0, frames.shape[:2])
            else:
                mc, msrc = model.compute_matching_feats(cur_image, src_image, unbatched_matching_encoder_forward)
            if is_bd:
                sparse = cur_data.get("sampled_rays") is not None and cur_data.get("sampled_depths") is not None
                kw["rendered_depth"] = cur_data.get("rendered_depth") if sparse else cur_data["rendered_depth"]
                kw["infer_depth"] = infer_depth
                if sparse:
                    # the ray path of run_mlp_train (bd_model.py:313-387) at inference: ray_pred_0..3 at the reference's shapes, the rays in
                    # pixel-centre units of the supervision map (:314-318, :325-326), the prior the constant -1 (run_mlp_val :433-434).
                    # cur_data["sampled_rays"] is left as it is (the reference normalises it in place, :320-326)
                    g = cur_data.get("full_res_depth_b1hw") if getattr(opts, "full_depth_supervision", False) else cur_data.get("depth_b1hw")
                    kw.update(query_rays=cur_data["sampled_rays"], query_depths=cur_data["sampled_depths"], query_scales=(0, 1, 2, 3),
                              query_grid=None if g is None else tuple(g.shape[-2:]))
                if getattr(opts, "use_prior", False) and cur_data.get("prior_prediction", None) is not None:
                    kw["prior_inputs"] = {k: cur_data[k] for k in ("prior_prediction", "world_T_cam_b44", "prior_cam_T_world", "K_s0_b44", "invK_s0_b44")}
            out = hot(mc, msrc, cur_feats, src_cam_T_cur_cam, cur_cam_T_src_cam, src_K, cur_invK, return_mask=return_mask, **kw)
        if "prior_mask" in out:
            cur_data["prior_mask"] = out.pop("prior_mask")  # run_mlp_val stores it on the inputs (bd_model.py:431)
        if is_bd and getattr(opts, "bd_edge_regularision", False) and "depth_b1hw" in cur_data:
            # run_mlp_val's other side effect (bd_model.py:444-447): the edge mask compute_binary_losses reads.  It is the
            # reference's own loss-side helper (utils/generic_utils.py:286, needs kornia) unless the native one is asked for
            if native_edge_mask:
                from .geometry import edge_mask as get_edge_mask
            else:
                get_edge_mask = _reference_get_edge_mask()
            cur_data["edge_mask"] = get_edge_mask(cur_data["depth_b1hw"])
        return out

    return forward
