"""Host side of the fused per-pixel occlusion MLP (csrc/mlp.hip).

``occlusion_logits`` is the fused form of the reference's per-plane loop
(experiment_modules/bd_model.py:293-304, :412-442); ``binary_mlp_forward`` keeps the exact
``BinaryMLPNetwork.forward(list_of_BHWC, max_scale_only)`` interface
(modules/networks.py:106-115) on top of the same kernel.
"""
from __future__ import annotations

import ctypes
import types
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib


def mlp_math_of(net) -> str:
    """Arithmetic of the per-plane 128x128 layer: ``net.mlp_math`` if set, else
    ``cost_volume.DEFAULT_MLP_MATH`` ("fp32" | "f16x3", see cost_volume.MLP_MATH_MODES)."""
    from . import cost_volume as _cv

    m = getattr(net, "mlp_math", None) or _cv.DEFAULT_MLP_MATH
    if m not in _cv.MLP_MATH_MODES:
        raise _lib.IdhError(f"unknown MLP math mode {m!r} (expected one of {_cv.MLP_MATH_MODES})")
    return m


def _prepared(seq: nn.Sequential, n_feat: int, use_prior: bool, math: str = "fp32"):
    """Fragment-ordered copies of one scale's three Linear layers, cached on the module."""
    l1, l2, l3 = seq[0], seq[2], seq[4]
    key = (math,) + tuple((p.data_ptr(), _lib.param_version(p)) for p in seq.parameters())
    c = seq.__dict__.get("_idh_mlp")
    if c is not None and c[0] == key:
        return c[1]
    w1, w2 = l1.weight.detach().contiguous(), l2.weight.detach().contiguous()
    _lib.require_cuda_f32(w1, w2)
    if w1.shape[0] != 128 or tuple(w2.shape) != (128, 128) or l3.weight.shape != (1, 128):
        raise _lib.IdhError("binary MLP kernel is specialised for mlp_size=128 (reference networks.py:88)")
    if w1.shape[1] != n_feat + (2 if use_prior else 1):
        raise _lib.IdhError(f"first Linear has {w1.shape[1]} inputs, expected depth + {n_feat} features" + (" + prior" if use_prior else ""))
    L = _lib.lib()
    dev = w1.device
    w1p = torch.empty(L.idh_packed_mlp_weight_floats(n_feat), device=dev)
    st = _lib.stream_ptr()
    _lib.check(L.idh_pack_mlp_weight(w1.data_ptr(), w1p.data_ptr(), w1.shape[1], 1, n_feat, st), "idh_pack_mlp_weight")
    if math == "f16x3":
        w2p = torch.empty(L.idh_packed_mlp_weight_f16_bytes(128) // 4, device=dev, dtype=torch.int32)
        _lib.check(L.idh_pack_mlp_weight_f16(w2.data_ptr(), w2p.data_ptr(), 128, 0, 128, st), "idh_pack_mlp_weight_f16")
    else:
        w2p = torch.empty(L.idh_packed_mlp_weight_floats(128), device=dev)
        _lib.check(L.idh_pack_mlp_weight(w2.data_ptr(), w2p.data_ptr(), 128, 0, 128, st), "idh_pack_mlp_weight")
    vecs = torch.zeros(6, 128, device=dev)
    vecs[0] = l1.bias.detach()
    vecs[1] = w1[:, 0]
    if use_prior:
        vecs[2] = w1[:, n_feat + 1]
    vecs[3] = l2.bias.detach()
    vecs[4] = l3.weight.detach()[0]
    vecs[5, 0] = l3.bias.detach()[0]
    out = (w1p, w2p, vecs.contiguous())
    seq.__dict__["_idh_mlp"] = (key, out)
    return out


def occlusion_logits(net, feat_nhwc: torch.Tensor, feat_c0: int, n_feat: int, depth_bphw: torch.Tensor,
                     prior_bphw: Optional[torch.Tensor] = None, scale: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """feat_nhwc: dense (B,H,W,CS) buffer, features are channels [feat_c0, feat_c0+n_feat).
    Returns logits (B,P,H,W).  With a prior-enabled network and ``prior_bphw=None`` the prior
    channel is the constant -1 (reference bd_model.py:433-434)."""
    _lib.require_cuda_f32(feat_nhwc, depth_bphw, prior_bphw)
    B, H, W, CS = feat_nhwc.shape
    P = depth_bphw.shape[1]
    if tuple(depth_bphw.shape) != (B, P, H, W):
        raise _lib.IdhError(f"rendered depth {tuple(depth_bphw.shape)} does not match features {(B, H, W)}")
    math = mlp_math_of(net)
    w1p, w2p, vecs = _prepared(net.mlps[f"s{scale}"], n_feat, net.use_prior, math)
    depth = depth_bphw.contiguous()
    prior = None
    if prior_bphw is not None:
        if not net.use_prior:
            raise _lib.IdhError("prior given to a network built with use_prior=False")
        prior = prior_bphw.expand(B, P, H, W).contiguous()
    if out is None:
        out = torch.empty(B, P, H, W, device=feat_nhwc.device, dtype=torch.float32)
    L = _lib.lib()
    fwd = L.idh_binary_mlp_f16x3_fwd if math == "f16x3" else L.idh_binary_mlp_fwd
    _lib.check(
        fwd(feat_nhwc.data_ptr() + 4 * feat_c0, CS, n_feat, depth.data_ptr(), _lib.ptr(prior), int(net.use_prior), -1.0,
            w1p.data_ptr(), w2p.data_ptr(), vecs.data_ptr(), B, P, H * W, out.data_ptr(), _lib.stream_ptr()),
        "idh_binary_mlp_fwd")
    return out


def _thresholder_tables(thresholder, dev):
    """(bins, logit(thresholds)) fp32 on ``dev`` for the search kernels, (None, None) without a thresholder."""
    if thresholder is None:
        return None, None
    bins = thresholder.bins.to(device=dev, dtype=torch.float32).contiguous()
    thr = thresholder.thresholds.to(device=dev, dtype=torch.float32)
    if bins.dim() != 1 or thr.shape != bins.shape or not bool(((thr > 0) & (thr < 1)).all()):
        raise _lib.IdhError("thresholder needs 1-D bins / thresholds of equal length with thresholds in (0, 1)")
    return bins, torch.log(thr / (1 - thr)).contiguous()


def _threshold_args(threshold, thresholder, dev):
    """(threshold, bins, thr_logits, n_bins) as the ray and view search entry points take them, and the tables, to be held until the launch is
    enqueued."""
    bins, thr_logits = _thresholder_tables(thresholder, dev)
    return (threshold, _lib.ptr(bins), _lib.ptr(thr_logits), 0 if bins is None else bins.numel()), (bins, thr_logits)


def infer_depth(net, feat_nhwc: torch.Tensor, feat_c0: int, n_feat: int, prior_b1hw: Optional[torch.Tensor] = None,
                iters: int = 12, lo: float = 0.5, hi: float = 8.0, threshold: float = 0.5, thresholder=None):
    """Fused form of the reference's ``infer_depth`` loop (bd_model.py:273-292): returns
    (search_depths (B,1,H,W), logits of the last evaluation (B,1,H,W)).  ``thresholder``: an object
    with ``bins`` / ``thresholds`` tensors (metrics.Thresholder, reference binary_metrics_utils.py:42-52)
    -> per-depth thresholds as in bd_model.py:282-283; None -> the constant ``threshold``."""
    _lib.require_cuda_f32(feat_nhwc, prior_b1hw)
    B, H, W, CS = feat_nhwc.shape
    math = mlp_math_of(net)
    w1p, w2p, vecs = _prepared(net.mlps["s0"], n_feat, net.use_prior, math)
    prior = prior_b1hw.contiguous() if prior_b1hw is not None else None
    sd = torch.empty(B, 1, H, W, device=feat_nhwc.device)
    logits = torch.empty(B, 1, H, W, device=feat_nhwc.device)
    bins, thr_logits = _thresholder_tables(thresholder, feat_nhwc.device)
    if math == "f16x3":
        _lib.check(
            _lib.lib().idh_binary_mlp_search_f16x3_fwd(feat_nhwc.data_ptr() + 4 * feat_c0, CS, n_feat, _lib.ptr(prior), int(net.use_prior), -1.0,
                                                       w1p.data_ptr(), w2p.data_ptr(), vecs.data_ptr(), B, H * W, iters, lo, hi, threshold,
                                                       _lib.ptr(bins), _lib.ptr(thr_logits), 0 if bins is None else bins.numel(),
                                                       sd.data_ptr(), logits.data_ptr(), _lib.stream_ptr()),
            "idh_binary_mlp_search_f16x3_fwd")
        return sd, logits
    if thresholder is not None:
        _lib.check(
            _lib.lib().idh_binary_mlp_search_thr_fwd(feat_nhwc.data_ptr() + 4 * feat_c0, CS, n_feat, _lib.ptr(prior), int(net.use_prior), -1.0,
                                                     w1p.data_ptr(), w2p.data_ptr(), vecs.data_ptr(), B, H * W, iters, lo, hi,
                                                     bins.data_ptr(), thr_logits.data_ptr(), bins.numel(), sd.data_ptr(), logits.data_ptr(),
                                                     _lib.stream_ptr()),
            "idh_binary_mlp_search_thr_fwd")
        return sd, logits
    _lib.check(
        _lib.lib().idh_binary_mlp_search_fwd(feat_nhwc.data_ptr() + 4 * feat_c0, CS, n_feat, _lib.ptr(prior), int(net.use_prior), -1.0,
                                             w1p.data_ptr(), w2p.data_ptr(), vecs.data_ptr(), B, H * W, iters, lo, hi, threshold,
                                             sd.data_ptr(), logits.data_ptr(), _lib.stream_ptr()),
        "idh_binary_mlp_search_fwd")
    return sd, logits


def sample_prior(rendered_depth: torch.Tensor, prior_prediction: torch.Tensor, cur_world_T_cam: torch.Tensor,
                 prior_cam_T_world: torch.Tensor, K: torch.Tensor, invK: torch.Tensor) -> torch.Tensor:
    """BDModel.sample_prior (reference bd_model.py:395-410) on the GPU kernel; returns the prior
    channel (B,P,H,W) with -1 where invalid."""
    _lib.require_cuda_f32(rendered_depth, prior_prediction, cur_world_T_cam, prior_cam_T_world, K, invK)
    B, P, H, W = rendered_depth.shape
    if prior_prediction.shape[0] != B or tuple(prior_prediction.shape[2:]) != (H, W):
        raise _lib.IdhError(f"prior prediction {tuple(prior_prediction.shape)} does not match rendered depth {tuple(rendered_depth.shape)}")
    out = torch.empty(B, P, H, W, device=rendered_depth.device, dtype=torch.float32)
    # hold the contiguous copies in locals until the launch is enqueued
    rd, pp, cw, pc, Kc, iKc = (t.contiguous() for t in (rendered_depth, prior_prediction, cur_world_T_cam, prior_cam_T_world, K, invK))
    _lib.check(
        _lib.lib().idh_sample_prior_fwd(rd.data_ptr(), pp.data_ptr(), prior_prediction.shape[1],
                                        cw.data_ptr(), pc.data_ptr(), Kc.data_ptr(),
                                        iKc.data_ptr(), B, P, H, W, out.data_ptr(), _lib.stream_ptr()),
        "idh_sample_prior_fwd")
    return out


def ray_logits(net, feat_view, rays: torch.Tensor, depths: torch.Tensor, prior=None, scale: int = 0, grid=None, ray_step: int = 1) -> torch.Tensor:
    """The occlusion MLP of ``scale`` at sparse rays: the fused form of one scale of ``BDModel.run_mlp_train`` (reference
    bd_model.py:348-387) on ``idh_binary_mlp_rays_fwd``.  ``feat_view``: an ``nhwc.View`` of that scale's decoder output (B,H,W,Cf slice);
    ``rays`` (B,N,2): (x, y) in pixel-centre units of ``grid`` = (grid_h, grid_w) - the shape of the reference's ``depth_b1hw`` /
    ``full_res_depth_b1hw``; None = the feature map's own (H, W); ``depths`` (B,N,S); ``prior``: None (a prior-enabled network then sees
    the constant -1, bd_model.py:433-434), a float constant or a (B,N,S) tensor; ``ray_step``: every ray_step-th ray and its depths (the
    reference's ``[:, ::(scale + 1)]``).  Returns logits (B,1,Nq,S), Nq = ceil(N / ray_step): the reference's output layout (:387).
    ``rays`` is never written: the reference normalises ``inputs["sampled_rays"]`` IN PLACE through its ``unsqueeze(2)`` view
    (:320-326), so a caller that passes the same dictionary twice there samples different rays the second time."""
    if mlp_math_of(net) != "fp32":
        raise _lib.IdhError("ray queries are fp32 only (IDH_EUNSUPPORTED): there is no f16x3 form of idh_binary_mlp_rays_fwd; set mlp_math = 'fp32'")
    prior_t = prior if isinstance(prior, torch.Tensor) else None
    _lib.require_cuda_f32(feat_view.buf, rays, depths, prior_t)
    B, H, W = feat_view.N, feat_view.H, feat_view.W
    if rays.dim() != 3 or rays.shape[0] != B or rays.shape[2] != 2:
        raise _lib.IdhError(f"rays must be ({B}, N, 2), got {tuple(rays.shape)}")
    N = rays.shape[1]
    if depths.dim() != 3 or tuple(depths.shape[:2]) != (B, N):
        raise _lib.IdhError(f"depths must be ({B}, {N}, S), got {tuple(depths.shape)}")
    S = depths.shape[2]
    if ray_step < 1:
        raise _lib.IdhError(f"ray_step must be >= 1, got {ray_step}")
    if prior is not None and not net.use_prior:
        raise _lib.IdhError("prior given to a network built with use_prior=False")
    gh, gw = (H, W) if grid is None else (int(grid[0]), int(grid[1]))
    w1p, w2p, vecs = _prepared(net.mlps[f"s{scale}"], feat_view.C, net.use_prior, "fp32")
    r, d = rays.contiguous(), depths.contiguous()  # alive until enqueued
    pt = prior_t.expand(B, N, S).contiguous() if prior_t is not None else None
    Nq = (N + ray_step - 1) // ray_step
    out = torch.empty(B, 1, Nq, S, device=rays.device, dtype=torch.float32)
    _lib.check(
        _lib.lib().idh_binary_mlp_rays_fwd(feat_view.ptr, feat_view.cs, feat_view.C, B, H, W, r.data_ptr(), d.data_ptr(), _lib.ptr(pt),
                                           int(net.use_prior), -1.0 if prior is None or prior_t is not None else float(prior), N, S, ray_step,
                                           gw, gh, w1p.data_ptr(), w2p.data_ptr(), vecs.data_ptr(), out.data_ptr(), _lib.stream_ptr()),
        "idh_binary_mlp_rays_fwd")
    return out


def ray_depths(net, feat_view, rays: torch.Tensor, prior=None, grid=None, iters: int = 12, lo: float = 0.5, hi: float = 8.0, threshold: float = 0.5,
               thresholder=None, invK: Optional[torch.Tensor] = None, world_T_cam: Optional[torch.Tensor] = None):
    """Where each ray hits the scene: the ``infer_depth`` search (bd_model.py:273-292) at sparse rays, on ``idh_binary_mlp_rays_search_fwd`` -
    one launch gathers each ray's feature row once and runs the ``iters`` dependent evaluations in registers.  ``feat_view`` / ``rays`` /
    ``grid`` as ``ray_logits`` (scale 0); ``prior``: None (a prior-enabled network sees the constant -1, bd_model.py:433-434), a float
    or a (B,N) tensor; ``thresholder`` as ``infer_depth``.  ``invK`` (B,4,4) at the resolution of ``grid``: also return the hit points
    ``d * invK (x, y, 1)`` (BackprojectDepth, geometry_utils.py:39,60-61), taken to the world by ``world_T_cam`` (B,4,4) when given.
    Returns (depth (B,N), logits of the last evaluation (B,N), hit (B,N) uint8, points (B,N,3) | None); hit: bit 0 = the far bound moved,
    bit 1 = the near bound moved - 3: the surface lies inside [lo, hi]; 1 / 2: the search ran into ``lo`` / ``hi``, no hit in range."""
    if mlp_math_of(net) != "fp32":
        raise _lib.IdhError("ray queries are fp32 only (IDH_EUNSUPPORTED): there is no f16x3 form of idh_binary_mlp_rays_search_fwd; set mlp_math = 'fp32'")
    prior_t = prior if isinstance(prior, torch.Tensor) else None
    _lib.require_cuda_f32(feat_view.buf, rays, prior_t, invK, world_T_cam)
    B, H, W = feat_view.N, feat_view.H, feat_view.W
    if rays.dim() != 3 or rays.shape[0] != B or rays.shape[2] != 2:
        raise _lib.IdhError(f"rays must be ({B}, N, 2), got {tuple(rays.shape)}")
    N = rays.shape[1]
    if prior is not None and not net.use_prior:
        raise _lib.IdhError("prior given to a network built with use_prior=False")
    if prior_t is not None and tuple(prior_t.shape) != (B, N):
        raise _lib.IdhError(f"prior must be ({B}, {N}), got {tuple(prior_t.shape)}")
    if world_T_cam is not None and invK is None:
        raise _lib.IdhError("world_T_cam without invK: the hit points need the intrinsics of the rays' grid")
    for m in (invK, world_T_cam):
        if m is not None and tuple(m.shape) != (B, 4, 4):
            raise _lib.IdhError(f"invK / world_T_cam must be ({B}, 4, 4), got {tuple(m.shape)}")
    gh, gw = (H, W) if grid is None else (int(grid[0]), int(grid[1]))
    w1p, w2p, vecs = _prepared(net.mlps["s0"], feat_view.C, net.use_prior, "fp32")
    thr, _tables = _threshold_args(threshold, thresholder, rays.device)
    r = rays.contiguous()  # alive until enqueued
    pt = prior_t.contiguous() if prior_t is not None else None
    iK = invK.contiguous() if invK is not None else None
    wT = world_T_cam.contiguous() if world_T_cam is not None else None
    buf = torch.empty((5 if iK is not None else 2) * B * N, device=rays.device)  # one allocation for the float outputs, as project_points
    depth, logits = buf[: B * N].view(B, N), buf[B * N: 2 * B * N].view(B, N)
    points = buf[2 * B * N:].view(B, N, 3) if iK is not None else None
    hit = torch.empty(B, N, device=rays.device, dtype=torch.uint8)
    _lib.check(
        _lib.lib().idh_binary_mlp_rays_search_fwd(feat_view.ptr, feat_view.cs, feat_view.C, B, H, W, r.data_ptr(), _lib.ptr(pt), int(net.use_prior),
                                                  -1.0 if prior is None or prior_t is not None else float(prior), N, gw, gh, w1p.data_ptr(),
                                                  w2p.data_ptr(), vecs.data_ptr(), iters, lo, hi, *thr, _lib.ptr(iK), _lib.ptr(wT), depth.data_ptr(),
                                                  logits.data_ptr(), hit.data_ptr(), _lib.ptr(points), _lib.stream_ptr()),
        "idh_binary_mlp_rays_search_fwd")
    return depth, logits, hit, points


def project_points(points_bn3: torch.Tensor, cam_T_world: torch.Tensor, K: torch.Tensor, H: int, W: int, prior_pred: Optional[torch.Tensor] = None,
                   prior_cam_T_world: Optional[torch.Tensor] = None, prior_K: Optional[torch.Tensor] = None):
    """World points (B,N,3) -> (rays (B,N,2), depth (B,N), valid (B,N) bool, prior (B,N) | None) in the H x W view of ``K`` /
    ``cam_T_world`` (B,4,4), as ``Project3D`` (reference geometry_utils.py:77-89); with ``prior_pred`` (B,1,H,W) also its nearest sample
    in the prior camera (``BDModel.sample_prior``, bd_model.py:395-410; -1 behind that camera or outside).  ``idh_project_points_fwd``."""
    _lib.require_cuda_f32(points_bn3, cam_T_world, K, prior_pred, prior_cam_T_world, prior_K)
    if points_bn3.dim() != 3 or points_bn3.shape[2] != 3:
        raise _lib.IdhError(f"points must be (B, N, 3), got {tuple(points_bn3.shape)}")
    B, N, _ = points_bn3.shape
    mats = [cam_T_world, K] + ([prior_cam_T_world, prior_K] if prior_pred is not None else [])
    for m in mats:
        if m is None or tuple(m.shape) != (B, 4, 4):
            raise _lib.IdhError(f"cam_T_world / K (and the prior's) must be ({B}, 4, 4)")
    if prior_pred is not None and tuple(prior_pred.shape) != (B, 1, H, W):
        raise _lib.IdhError(f"prior prediction {tuple(prior_pred.shape)} must be ({B}, 1, {H}, {W})")
    dev = points_bn3.device
    pts, keep = points_bn3.contiguous(), [m.contiguous() for m in mats]
    pp = prior_pred.contiguous() if prior_pred is not None else None
    # one allocation for the float outputs (a query of a few hundred points is bound by host work, not by the kernel)
    buf = torch.empty((4 if pp is not None else 3) * B * N, device=dev)
    rays, depth = buf[: 2 * B * N].view(B, N, 2), buf[2 * B * N: 3 * B * N].view(B, N)
    prior = buf[3 * B * N:].view(B, N) if pp is not None else None
    valid = torch.empty(B, N, device=dev, dtype=torch.uint8)
    _lib.check(
        _lib.lib().idh_project_points_fwd(pts.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), B, N, H, W, rays.data_ptr(), depth.data_ptr(),
                                          valid.data_ptr(), _lib.ptr(pp), keep[2].data_ptr() if pp is not None else None,
                                          keep[3].data_ptr() if pp is not None else None, _lib.ptr(prior), _lib.stream_ptr()),
        "idh_project_points_fwd")
    return rays, depth, valid.view(torch.bool), prior  # the kernel writes 0 / 1: reinterpreted, no conversion pass


MAX_VIEW_KEYS, MAX_VIEW_KEY_CAMERAS = 16, 128  # idh_binary_mlp_view_keys_fwd: M <= 16, M * B <= 128


def _view_query(net, entry, public, feat_view, ring, cams, prior, rendered=None, size=None, rays=None, refine=None, return_points=False, planes=1):
    """The host side the ``view_*`` wrappers share: every check that is made before the C call ``entry``, in one order, and the arguments
    all of them pass.  ``feat_view``: the keyframe's ``nhwc.View``, or None with ``ring`` = (feat_ring, feat_c0, n_feat, key_slots);
    ``cams``: (invK, world_T_cam, key_cam_T_world, key_K_s0) - the last two are rings with ``ring``; ``prior`` as ``view_logits``; the rays
    are the pixels of ``rendered`` (B,P,h,w), or exactly one of ``size`` and ``rays`` (``public`` names the wrapper in that message).
    Returns a namespace: ``head`` (feat, feat_cs, Cf, B, H, W [, key_stride, n_slots, key_slots, M]), ``source`` (rendered, P, h, w) |
    (h, w, rays, N), ``cams`` (the matrices, the prior map and its cameras, has_prior, prior_const, the packed weights) - three runs of
    the C argument list -, the outputs ``a`` / ``b`` (two float maps of the rays' shape) and ``points`` | None, views of ONE allocation,
    ``u8`` (planes, *shape) bytes, ``dev``, and ``keep``: the contiguous copies, alive as long as the namespace is."""
    if mlp_math_of(net) != "fp32":
        raise _lib.IdhError(f"ray queries are fp32 only (IDH_EUNSUPPORTED): there is no f16x3 form of {entry}; set mlp_math = 'fp32'")
    if rendered is None and (size is None) == (rays is None):
        raise _lib.IdhError(f"{public} takes exactly one of size=(h, w) and rays=(B,N,2)")
    if refine is not None and int(refine) < 0:
        raise _lib.IdhError(f"refine must be >= 0, got {refine}")
    pmap = prior if isinstance(prior, (tuple, list)) else None
    mats = list(cams) + ([pmap[1], pmap[2]] if pmap is not None else [])
    feat_t = feat_view.buf if ring is None else ring[0]
    _lib.require_cuda_f32(feat_t, rendered, rays, *mats, pmap[0] if pmap is not None else None)
    if ring is None:
        B, H, W, cs, Cf, feat_ptr = feat_view.N, feat_view.H, feat_view.W, feat_view.cs, feat_view.C, feat_view.ptr
        for m in mats:
            if m is None or tuple(m.shape) != (B, 4, 4):
                raise _lib.IdhError(f"invK / world_T_cam / key_cam_T_world / key_K_s0 (and the prior's) must be ({B}, 4, 4)")
        prior_shape, prior_name = (B, 1, H, W), "prior prediction"
    else:
        feat_ring, feat_c0, Cf, key_slots = ring
        if feat_ring.dim() != 5 or not feat_ring.is_contiguous():
            raise _lib.IdhError(f"the feature ring must be a dense (n_slots, B, H, W, C) tensor, got {tuple(feat_ring.shape)}")
        n_slots, B, H, W, cs = feat_ring.shape
        if feat_c0 < 0 or Cf <= 0 or feat_c0 + Cf > cs:
            raise _lib.IdhError(f"channels [{feat_c0}, {feat_c0 + Cf}) are not inside the ring's {cs}")
        feat_ptr = feat_ring.data_ptr() + 4 * feat_c0
        for m in mats[:2]:
            if tuple(m.shape) != (B, 4, 4):
                raise _lib.IdhError(f"invK / world_T_cam must be ({B}, 4, 4), got {tuple(m.shape)}")
        for m in mats[2:]:
            if tuple(m.shape) != (n_slots, B, 4, 4):
                raise _lib.IdhError(f"the camera rings must be ({n_slots}, {B}, 4, 4), got {tuple(m.shape)}")
        prior_shape, prior_name = (n_slots, B, 1, H, W), "prior ring"
    if rendered is not None:
        if rendered.dim() != 4 or rendered.shape[0] != B:
            raise _lib.IdhError(f"rendered depth must be ({B}, P, h, w), got {tuple(rendered.shape)}")
        shape = tuple(rendered.shape)
    elif rays is not None:
        if rays.dim() != 3 or rays.shape[0] != B or rays.shape[2] != 2:
            raise _lib.IdhError(f"rays must be ({B}, N, 2), got {tuple(rays.shape)}")
        shape = (B, rays.shape[1])
    else:
        h, w = int(size[0]), int(size[1])
        if h < 0 or w < 0:
            raise _lib.IdhError(f"size must be (h, w) >= 0, got {tuple(size)}")
        shape = (B, 1, h, w)
    if prior is not None and not net.use_prior:
        raise _lib.IdhError("prior given to a network built with use_prior=False")
    if pmap is not None and tuple(pmap[0].shape) != prior_shape:
        raise _lib.IdhError(f"{prior_name} {tuple(pmap[0].shape)} must be ({', '.join(str(d) for d in prior_shape)})")
    head = (feat_ptr, cs, Cf, B, H, W)
    if ring is not None:
        slots = [int(k) for k in key_slots]
        if not slots or len(set(slots)) != len(slots) or any(k < 0 or k >= n_slots for k in slots):
            raise _lib.IdhError(f"key_slots must be a non-empty list of distinct slots in [0, {n_slots}), got {slots}")
        if len(slots) > MAX_VIEW_KEYS or len(slots) * B > MAX_VIEW_KEY_CAMERAS:
            raise _lib.IdhError(f"{entry} takes at most {MAX_VIEW_KEYS} keys and {MAX_VIEW_KEY_CAMERAS} key cameras (keys x batch), got {len(slots)} x {B} (IDH_EUNSUPPORTED)")
        head += (B * H * W * cs, n_slots, (ctypes.c_int * len(slots))(*slots), len(slots))
    w1p, w2p, vecs = _prepared(net.mlps["s0"], Cf, net.use_prior, "fp32")
    keep = [m.contiguous() for m in mats]  # alive until enqueued
    src = rendered if rendered is not None else rays
    src = src.contiguous() if src is not None else None
    pp = pmap[0].contiguous() if pmap is not None else None
    q = types.SimpleNamespace(head=head, dev=feat_t.device, keep=(keep, src, pp, w1p, w2p, vecs))
    if rendered is not None:
        q.source = (src.data_ptr(),) + shape[1:]
    else:
        q.source = (0, 0, src.data_ptr(), shape[1]) if rays is not None else shape[2:] + (None, 0)
    q.cams = (keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), _lib.ptr(pp), keep[4].data_ptr() if pp is not None else None,
              keep[5].data_ptr() if pp is not None else None, int(net.use_prior), -1.0 if prior is None or pmap is not None else float(prior),
              w1p.data_ptr(), w2p.data_ptr(), vecs.data_ptr())
    n = torch.Size(shape).numel()
    buf = torch.empty((5 if return_points else 2) * n, device=q.dev)  # one allocation for the float outputs, as project_points
    q.a, q.b = buf[:n].view(shape), buf[n: 2 * n].view(shape)
    q.points = buf[2 * n:].view(*shape, 3) if return_points else None
    q.u8 = torch.empty((planes,) + shape, device=q.dev, dtype=torch.uint8)
    return q


def view_logits(net, feat_view, rendered_bphw: torch.Tensor, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor, key_cam_T_world_b44: torch.Tensor,
                key_K_s0_b44: torch.Tensor, prior=None, fill: float = 0.0, return_points: bool = False):
    """Dense occlusion in another camera on ``idh_binary_mlp_view_fwd``: every pixel of ``rendered_bphw`` (B,P,h,w) - an asset's depth in
    the view of ``invK_b44`` (at h x w) / ``world_T_cam_b44`` - is back-projected (``BackprojectDepth``, reference geometry_utils.py:55-63),
    projected into the keyframe's scale-0 map ``feat_view`` with ``key_K_s0_b44 @ key_cam_T_world_b44`` (``Project3D``, :77-89), and the
    scale-0 MLP is asked there at the point's keyframe depth: one launch, no rays, depths or validity in memory.  ``prior``: None (a
    prior-enabled network sees the constant -1, bd_model.py:433-434), a float, or (prior_pred (B,1,H,W), prior_cam_T_world (B,4,4),
    prior_K (B,4,4)) - sampled nearest at the point's projection into that camera, -1 outside (``BDModel.sample_prior``, :405-409).
    A pixel is valid when its depth is finite and positive and the point lies in front of the keyframe camera and inside its image;
    the others hold ``fill``.  Returns (logits (B,P,h,w), valid (B,P,h,w) bool, view_depth (B,P,h,w): the keyframe z, points (B,P,h,w,3)
    world points | None)."""
    q = _view_query(net, "idh_binary_mlp_view_fwd", "view_logits", feat_view, None, (invK_b44, world_T_cam_b44, key_cam_T_world_b44, key_K_s0_b44),
                    prior, rendered=rendered_bphw, return_points=return_points)
    _lib.check(
        _lib.lib().idh_binary_mlp_view_fwd(*q.head, *q.source, *q.cams, float(fill), q.a.data_ptr(), q.u8.data_ptr(), q.b.data_ptr(), _lib.ptr(q.points),
                                           _lib.stream_ptr()),
        "idh_binary_mlp_view_fwd")
    return q.a, q.u8[0].view(torch.bool), q.b, q.points  # the kernel writes 0 / 1: reinterpreted, no conversion pass


def view_depths(net, feat_view, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor, key_cam_T_world_b44: torch.Tensor, key_K_s0_b44: torch.Tensor,
                size=None, rays: Optional[torch.Tensor] = None, prior=None, iters: int = 12, lo: float = 0.5, hi: float = 8.0,
                threshold: float = 0.5, thresholder=None, fill: float = 0.0, return_points: bool = False):
    """Depth along the rays of another camera on ``idh_binary_mlp_view_search_fwd``: the ``infer_depth`` search (bd_model.py:273-292) with
    the query the z-depth in the view of ``invK_b44`` / ``world_T_cam_b44``; every step is one ``view_logits`` pixel at that depth (its
    projection into the keyframe's scale-0 map ``feat_view``, validity, prior sample, gather and MLP), all ``iters`` steps in one launch.
    Exactly one of ``size`` = (h, w) - every pixel centre of the view at that resolution - and ``rays`` (B,N,2) - (x, y) in pixel-centre
    units of the view, a tap at pixel (i, j) is (j + 0.5, i + 0.5); rays outside the view's image are legal.  ``prior`` as ``view_logits``
    (a map is sampled per probe).  A probe outside the keyframe's view has the logit ``fill``: -inf counts it as visible (the search
    retreats towards ``lo``), +inf as hidden (towards ``hi``).  The threshold of a step is looked up at the probe's KEYFRAME depth.
    Returns (depth (B,1,h,w) | (B,N), logits of the last step, flags uint8: bit 0 = ``hi`` moved, bit 1 = ``lo`` moved, bit 2 = some probe
    was invalid, world points (...,3) | None).  The MLP answers occlusion as seen from the keyframe: the depth is where the view's ray
    crosses into the region hidden from the keyframe - the surface as far as both cameras see the same side of it."""
    q = _view_query(net, "idh_binary_mlp_view_search_fwd", "view_depths", feat_view, None, (invK_b44, world_T_cam_b44, key_cam_T_world_b44, key_K_s0_b44),
                    prior, size=size, rays=rays, return_points=return_points)
    thr, _tables = _threshold_args(threshold, thresholder, q.dev)
    _lib.check(
        _lib.lib().idh_binary_mlp_view_search_fwd(*q.head, *q.source, *q.cams, iters, lo, hi, *thr, float(fill), q.a.data_ptr(), q.b.data_ptr(),
                                                  q.u8.data_ptr(), _lib.ptr(q.points), _lib.stream_ptr()),
        "idh_binary_mlp_view_search_fwd")
    return q.a, q.b, q.u8[0], q.points


def view_keys_logits(net, feat_ring: torch.Tensor, feat_c0: int, n_feat: int, key_slots, rendered_bphw: torch.Tensor, invK_b44: torch.Tensor,
                     world_T_cam_b44: torch.Tensor, key_cam_T_world_sb44: torch.Tensor, key_K_s0_sb44: torch.Tensor, prior=None, fill: float = 0.0,
                     return_points: bool = False):
    """``view_logits`` against several remembered keyframes on ``idh_binary_mlp_view_keys_fwd``: every pixel of ``rendered_bphw`` (B,P,h,w)
    is projected into the keys ``key_slots`` - slots of the dense ring ``feat_ring`` (n_slots,B,H,W,CS), channels [feat_c0, feat_c0 + n_feat),
    with cameras ``key_cam_T_world_sb44`` / ``key_K_s0_sb44`` (n_slots,B,4,4) - in that order, and asked in the first key in which it is
    valid: one launch and one MLP pass per pixel.  ``prior``: None, a float, or rings (prior_pred (n_slots,B,1,H,W), prior_cam_T_world,
    prior_K (n_slots,B,4,4)) - the selected key's own prior is sampled.  Returns (logits (B,P,h,w), ``fill`` where no key is valid, key
    (B,P,h,w) uint8: the position in ``key_slots`` of the selected key, 255 = none, view_depth (B,P,h,w): z in the selected key (in the
    first key where none is valid), points (B,P,h,w,3) | None)."""
    q = _view_query(net, "idh_binary_mlp_view_keys_fwd", "view_keys_logits", None, (feat_ring, feat_c0, n_feat, key_slots),
                    (invK_b44, world_T_cam_b44, key_cam_T_world_sb44, key_K_s0_sb44), prior, rendered=rendered_bphw, return_points=return_points)
    _lib.check(
        _lib.lib().idh_binary_mlp_view_keys_fwd(*q.head, *q.source, *q.cams, float(fill), q.a.data_ptr(), q.u8.data_ptr(), q.b.data_ptr(),
                                                _lib.ptr(q.points), _lib.stream_ptr()),
        "idh_binary_mlp_view_keys_fwd")
    return q.a, q.u8[0], q.b, q.points


def view_keys_depths(net, feat_ring: torch.Tensor, feat_c0: int, n_feat: int, key_slots, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor,
                     key_cam_T_world_sb44: torch.Tensor, key_K_s0_sb44: torch.Tensor, size=None, rays: Optional[torch.Tensor] = None, prior=None,
                     iters: int = 12, lo: float = 0.5, hi: float = 8.0, threshold: float = 0.5, thresholder=None, fill: float = 0.0,
                     return_points: bool = False):
    """``view_depths`` against several remembered keyframes on ``idh_binary_mlp_view_keys_search_fwd``: the same search, every step one
    ``view_keys_logits`` pixel that selects its own key (the first of ``key_slots`` in which the probe is valid); the threshold of a step
    is looked up at the probe's depth in the selected key (in the first key where none is valid).  Ring arguments as ``view_keys_logits``,
    the others as ``view_depths``.  Returns (depth, logits of the last step, flags uint8 - bit 2: no key was valid at some probe -, world
    points | None, key uint8: the position in ``key_slots`` of the key the LAST step selected, 255 = none)."""
    q = _view_query(net, "idh_binary_mlp_view_keys_search_fwd", "view_keys_depths", None, (feat_ring, feat_c0, n_feat, key_slots),
                    (invK_b44, world_T_cam_b44, key_cam_T_world_sb44, key_K_s0_sb44), prior, size=size, rays=rays, return_points=return_points, planes=2)
    thr, _tables = _threshold_args(threshold, thresholder, q.dev)
    _lib.check(
        _lib.lib().idh_binary_mlp_view_keys_search_fwd(*q.head, *q.source, *q.cams, iters, lo, hi, *thr, float(fill), q.a.data_ptr(), q.b.data_ptr(),
                                                       q.u8[0].data_ptr(), _lib.ptr(q.points), q.u8[1].data_ptr(), _lib.stream_ptr()),
        "idh_binary_mlp_view_keys_search_fwd")
    return q.a, q.b, q.u8[0], q.points, q.u8[1]


MAX_MARCH_SAMPLES = 255  # idh_binary_mlp_view_march_fwd: hit_step is a byte, 255 = none


def march_samples(n: int, lo: float = 0.5, hi: float = 8.0, spacing: str = "linear") -> torch.Tensor:
    """``n`` march depths from ``lo`` to ``hi`` as a host fp32 tensor, every operation rounded to fp32: t_i = i / (n - 1);
    "linear": lo + (hi - lo) * t_i; "inverse" (uniform in 1 / depth): 1 / (1 / lo + (1 / hi - 1 / lo) * t_i); the first and last samples are
    ``lo`` and ``hi`` themselves, n = 1 gives [lo]."""
    n = int(n)
    if n < 1 or n > MAX_MARCH_SAMPLES:
        raise _lib.IdhError(f"the march takes 1 to {MAX_MARCH_SAMPLES} samples, got {n}")
    if spacing not in ("linear", "inverse"):
        raise _lib.IdhError(f"spacing must be 'linear' or 'inverse', got {spacing!r}")
    lo_t, hi_t = torch.tensor(float(lo), dtype=torch.float32), torch.tensor(float(hi), dtype=torch.float32)
    if not (torch.isfinite(lo_t) and torch.isfinite(hi_t) and lo_t > 0 and (hi_t > lo_t or n == 1)):
        raise _lib.IdhError(f"the march needs finite 0 < lo < hi, got lo = {lo}, hi = {hi}")
    if n == 1:
        return lo_t.reshape(1)
    t = torch.arange(n, dtype=torch.float32) / torch.tensor(float(n - 1), dtype=torch.float32)
    if spacing == "linear":
        out = lo_t + (hi_t - lo_t) * t
    else:
        one = torch.tensor(1.0, dtype=torch.float32)
        out = one / (one / lo_t + (one / hi_t - one / lo_t) * t)
    out[0], out[-1] = lo_t, hi_t
    return _checked_samples(out)


def _checked_samples(host: torch.Tensor) -> torch.Tensor:
    """The precondition the C entry points cannot check (they never read device memory): finite, positive, strictly increasing."""
    if host.dim() != 1 or host.numel() < 1 or host.numel() > MAX_MARCH_SAMPLES:
        raise _lib.IdhError(f"march samples must be a vector of 1 to {MAX_MARCH_SAMPLES} depths, got shape {tuple(host.shape)}")
    if not bool(torch.isfinite(host).all()) or not bool((host > 0).all()) or not bool((host[1:] > host[:-1]).all()):
        raise _lib.IdhError("march samples must be finite, positive and strictly increasing")
    return host


_march_cache: Dict[tuple, torch.Tensor] = {}
_MARCH_CACHE_MAX = 16  # settings kept on the device; a caller sweeping lo / hi starts over instead of growing the table


def _march_depths(samples, lo, hi, spacing, dev) -> torch.Tensor:
    """The device vector of march depths: a caller's float32 tensor - validated through one host copy, i.e. one synchronisation per call -
    or ``samples`` = an integer n, built by ``march_samples`` and kept per (n, lo, hi, spacing, device), so a per-frame caller uploads
    nothing and never synchronises."""
    if isinstance(samples, torch.Tensor):
        if samples.dtype != torch.float32:
            raise _lib.IdhError(f"march samples must be float32, got {samples.dtype}")
        _checked_samples(samples.detach().cpu())
        return samples.detach().to(dev).contiguous()
    if isinstance(samples, bool) or not isinstance(samples, int):
        raise _lib.IdhError(f"march samples must be a float32 tensor or an integer count, got {type(samples).__name__}")
    key = (samples, float(lo), float(hi), spacing, str(dev))
    t = _march_cache.get(key)
    if t is None:
        if len(_march_cache) >= _MARCH_CACHE_MAX:
            _march_cache.clear()
        t = _march_cache[key] = march_samples(samples, lo, hi, spacing).to(dev)
    return t


def view_march_depths(net, feat_view, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor, key_cam_T_world_b44: torch.Tensor,
                      key_K_s0_b44: torch.Tensor, size=None, rays: Optional[torch.Tensor] = None, prior=None, samples=16, lo: float = 0.5,
                      hi: float = 8.0, spacing: str = "linear", refine: int = 8, threshold: float = 0.5, thresholder=None, fill: float = 0.0,
                      return_points: bool = False):
    """First-hit depth along the rays of another camera on ``idh_binary_mlp_view_march_fwd``: every ray probes the shared depths ``samples``
    - a float32 vector (finite, positive, strictly increasing, at most 255), or an integer n with ``lo`` / ``hi`` / ``spacing`` ("linear" |
    "inverse", ``march_samples``) - in turn until the first probe that is behind the surface (logit < threshold), then bisects ``refine``
    steps inside [previous sample, that sample]; all in one launch.  Where ``view_depths`` assumes one crossing inside [lo, hi], this returns
    the first one at the resolution of the samples.  Every probe is one ``view_logits`` pixel; the other arguments as ``view_depths``.
    A probe outside the keyframe's view has the logit ``fill``: a negative ``fill`` makes it a hit, a positive one marches on.
    Returns (depth (B,1,h,w) | (B,N), logits of each ray's last probe, flags uint8: 3 = bracketed, 1 = behind at the first sample (depth is
    that sample), 2 = no hit (depth is the last sample), bit 2 = some evaluated probe was invalid, hit_step uint8: the first sample that was
    behind, 255 = none, world points (...,3) | None)."""
    q = _view_query(net, "idh_binary_mlp_view_march_fwd", "view_march_depths", feat_view, None, (invK_b44, world_T_cam_b44, key_cam_T_world_b44, key_K_s0_b44),
                    prior, size=size, rays=rays, refine=refine, return_points=return_points, planes=2)
    md = _march_depths(samples, lo, hi, spacing, q.dev)
    thr, _tables = _threshold_args(threshold, thresholder, q.dev)
    _lib.check(
        _lib.lib().idh_binary_mlp_view_march_fwd(*q.head, *q.source, *q.cams, md.data_ptr(), md.numel(), int(refine), *thr, float(fill), q.a.data_ptr(),
                                                 q.b.data_ptr(), q.u8[0].data_ptr(), q.u8[1].data_ptr(), _lib.ptr(q.points), _lib.stream_ptr()),
        "idh_binary_mlp_view_march_fwd")
    return q.a, q.b, q.u8[0], q.u8[1], q.points


def view_keys_march_depths(net, feat_ring: torch.Tensor, feat_c0: int, n_feat: int, key_slots, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor,
                           key_cam_T_world_sb44: torch.Tensor, key_K_s0_sb44: torch.Tensor, size=None, rays: Optional[torch.Tensor] = None,
                           prior=None, samples=16, lo: float = 0.5, hi: float = 8.0, spacing: str = "linear", refine: int = 8,
                           threshold: float = 0.5, thresholder=None, fill: float = 0.0, return_points: bool = False):
    """``view_march_depths`` against several remembered keyframes on ``idh_binary_mlp_view_keys_march_fwd``: the same march and refinement,
    every probe one ``view_keys_logits`` pixel that selects its own key (the first of ``key_slots`` in which it is valid); flag bit 2: no key
    was valid at some evaluated probe.  Ring arguments as ``view_keys_logits``, the others as ``view_march_depths``.  Returns (depth, logits
    of the last probe, flags, hit_step, world points | None, key uint8: the position in ``key_slots`` of the key the ray's LAST evaluated
    probe selected, 255 = none)."""
    q = _view_query(net, "idh_binary_mlp_view_keys_march_fwd", "view_keys_march_depths", None, (feat_ring, feat_c0, n_feat, key_slots),
                    (invK_b44, world_T_cam_b44, key_cam_T_world_sb44, key_K_s0_sb44), prior, size=size, rays=rays, refine=refine,
                    return_points=return_points, planes=3)
    md = _march_depths(samples, lo, hi, spacing, q.dev)
    thr, _tables = _threshold_args(threshold, thresholder, q.dev)
    _lib.check(
        _lib.lib().idh_binary_mlp_view_keys_march_fwd(*q.head, *q.source, *q.cams, md.data_ptr(), md.numel(), int(refine), *thr, float(fill),
                                                      q.a.data_ptr(), q.b.data_ptr(), q.u8[0].data_ptr(), q.u8[1].data_ptr(), _lib.ptr(q.points),
                                                      q.u8[2].data_ptr(), _lib.stream_ptr()),
        "idh_binary_mlp_view_keys_march_fwd")
    return q.a, q.b, q.u8[0], q.u8[1], q.points, q.u8[2]


def binary_mlp_forward(net, inputs: List[torch.Tensor], max_scale_only: bool = False) -> Dict[str, torch.Tensor]:
    """``BinaryMLPNetwork.forward(list of (..., Cin) tensors, max_scale_only)`` (reference networks.py:106-115); row = [depth | features |
    (prior)].  fp32: the rows are read IN PLACE through ``idh_binary_mlp_strided_fwd`` whatever their strides - in particular the
    ``permute(0, 2, 3, 1)`` view of an NCHW concat that ``BDModel.run_mlp_val`` passes (bd_model.py:415-439), whose channel planes the kernel
    reads as they lie - so a module-swapped model pays no (B,H,W,65) materialisation and no copy of the feature slice per query plane."""
    scales = [0] if max_scale_only else list(net.scales)
    outs = {}
    for s in scales:
        x = inputs[s]
        _lib.require_cuda_f32(x)
        cin = x.shape[-1]
        n_feat = cin - (2 if net.use_prior else 1)
        lead = x.shape[:-1]
        math = mlp_math_of(net)
        if math == "fp32" and x.dim() == 4 and x.stride(1) == x.shape[2] * x.stride(2) and min(x.stride()) > 0:
            # (B, H, W, Cin) with a uniform pixel stride: contiguous rows (pixel stride Cin, channel stride 1) or the permuted NCHW view (1, H*W)
            B, H, W, _ = x.shape
            w1p, w2p, vecs = _prepared(net.mlps[f"s{s}"], n_feat, net.use_prior, math)
            depth = x[..., 0].reshape(B, 1, H * W).contiguous()
            prior = x[..., 1 + n_feat].reshape(B, 1, H * W).contiguous() if net.use_prior else None
            y = torch.empty(B, 1, H * W, device=x.device, dtype=torch.float32)
            _lib.check(
                _lib.lib().idh_binary_mlp_strided_fwd(x.data_ptr() + 4 * x.stride(3), x.stride(0), x.stride(2), x.stride(3), n_feat, depth.data_ptr(),
                                                      _lib.ptr(prior), int(net.use_prior), -1.0, w1p.data_ptr(), w2p.data_ptr(), vecs.data_ptr(),
                                                      B, 1, H * W, y.data_ptr(), _lib.stream_ptr()),
                "idh_binary_mlp_strided_fwd")
            outs[f"pred_{s}"] = y.reshape(*lead, 1)
            continue
        rows = x.reshape(1, -1, 1, cin)  # (B=1, H=M, W=1, Cin)
        depth = rows[..., 0].reshape(1, 1, -1, 1)
        prior = rows[..., 1 + n_feat].reshape(1, 1, -1, 1) if net.use_prior else None
        if math == "fp32":  # row stride Cin = 65 / 66 floats, features from column 1: idh_binary_mlp_fwd takes any stride since ABI 105
            y = occlusion_logits(net, rows, 1, n_feat, depth, prior, scale=s)
        else:  # the frozen split-precision kernels keep the 16-byte row alignment
            y = occlusion_logits(net, rows[..., 1 : 1 + n_feat].contiguous(), 0, n_feat, depth, prior, scale=s)
        outs[f"pred_{s}"] = y.reshape(*lead, 1)
    return outs
