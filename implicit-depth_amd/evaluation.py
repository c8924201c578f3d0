"""Fused per-frame test evaluation (csrc/eval_frame.hip).

Reference test_bd.py:185-318 and test_reg.py:189-268 turn a batch's model outputs into per-frame metric rows with
surface / boundary masks, four F.interpolate calls up to the ground-truth resolution and three PlaneEvaluator calls,
materialising several (B, P, H, W) tensors on the way.  ``bd_frame_scores`` / ``reg_frame_scores`` return the same
score dict from one mask pass at model resolution and one counting pass at ground-truth resolution that samples the
low-resolution inputs on the fly.  The dict goes through ``metrics.metric_rows`` unchanged (the payload of the metrics
all-gather)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .metrics import DEPTH_METRIC_KEYS, PlaneEvaluator

TAGS = (None, "surface", "boundary")  # order of the tag axis of plane_scores
_ALL_TAGS = _lib.EVAL_TAG_ALL | _lib.EVAL_TAG_SURFACE | _lib.EVAL_TAG_BOUNDARY
_PLANES = tuple(1.5 + x * 0.5 for x in range(8))  # the key names' depth planes (binary_metrics_utils.py:135, :233)
_EV = PlaneEvaluator()


def _check_planes(depth_b1hw, rendered_bphw):
    _lib.require_cuda_f32(depth_b1hw, rendered_bphw)
    if rendered_bphw.dim() != 4 or depth_b1hw.dim() != 4 or depth_b1hw.shape[1] != 1 or depth_b1hw.shape[0] != rendered_bphw.shape[0] \
            or depth_b1hw.shape[2:] != rendered_bphw.shape[2:]:
        raise _lib.IdhError(f"eval masks: depth {tuple(depth_b1hw.shape)} must be (B,1,h,w) of rendered {tuple(rendered_bphw.shape)}")


def eval_masks(depth_b1hw: torch.Tensor, rendered_depth_bdhw: torch.Tensor, threshold: float = 0.05, surface=True, boundary=True, code=False):
    """(surface, boundary, code): the two float masks of the reference functions and the uint8 per-pixel code (bit 0 surface,
    bit 1 boundary); those not asked for are None.  One kernel for all."""
    _check_planes(depth_b1hw, rendered_depth_bdhw)
    B, P, h, w = rendered_depth_bdhw.shape
    d, r = depth_b1hw.contiguous(), rendered_depth_bdhw.contiguous()
    mk = lambda want, dt: torch.empty(B, P, h, w, device=r.device, dtype=dt) if want else None
    s, b, c = mk(surface, torch.float32), mk(boundary, torch.float32), mk(code, torch.uint8)
    _lib.check(_lib.lib().idh_eval_masks_fwd(d.data_ptr(), r.data_ptr(), B, P, h, w, float(threshold), _lib.ptr(s), _lib.ptr(b), _lib.ptr(c),
                                             _lib.stream_ptr()), "idh_eval_masks_fwd")
    return s, b, c


def get_surface_mask(depth_b1hw, rendered_depth_bdhw, threshold=0.05):
    """utils/binary_metrics_utils.py:35-39: (|depth - rendered| / depth < threshold) as a float (B, P, h, w) mask."""
    return eval_masks(depth_b1hw, rendered_depth_bdhw, threshold, boundary=False)[0]


def get_boundary_mask(depth_b1hw, rendered_depth_bdhw):
    """utils/binary_metrics_utils.py:23-32: 7x7 dilation of the 3x3 occlusion edges of (rendered < depth), 0 where depth is NaN."""
    return eval_masks(depth_b1hw, rendered_depth_bdhw, surface=False)[1]


def _workspace(B, P, h, w, H, W, T, device):
    n = _lib.lib().idh_eval_frame_workspace_bytes(B, P, h, w, H, W, T)
    return torch.empty(max(n, 8), device=device, dtype=torch.uint8), n


def plane_scores(prediction, rendered_bphw, gt_b1HW, depth_b1hw=None, *, regressed=False, nearest=False, sigmoid_multiplier=1.0,
                 thresholds: Sequence[float] = (), bins: Optional[torch.Tensor] = None, bin_thresholds: Optional[torch.Tensor] = None,
                 tag_mask=_ALL_TAGS, surface_threshold=0.05, return_counts=False):
    """(B, 3, P, T, 3) = [iou, iou_pos, iou_neg] per (frame, tag in TAGS, query plane, threshold) after upsampling to gt's resolution.
    ``prediction``: logits (B, P, h, w), or with ``regressed`` a depth (B, 1, h, w) compared with the query (T = 1).  ``bins`` /
    ``bin_thresholds``: the Thresholder (T = 1).  With ``return_counts`` also the (B, 3, P, 2 + 2T) int32 counts
    {valid, target, pred[T], inter[T]}."""
    _lib.require_cuda_f32(prediction, rendered_bphw, gt_b1HW, depth_b1hw, bins, bin_thresholds)
    B, P, h, w = rendered_bphw.shape
    H, W = gt_b1HW.shape[-2:]
    dev = rendered_bphw.device
    if tuple(prediction.shape) != ((B, 1, h, w) if regressed else (B, P, h, w)) or tuple(gt_b1HW.shape) != (B, 1, H, W):
        raise _lib.IdhError(f"plane_scores: shapes prediction {tuple(prediction.shape)}, rendered {tuple(rendered_bphw.shape)}, gt {tuple(gt_b1HW.shape)}")
    if tag_mask & ~_lib.EVAL_TAG_ALL:
        _check_planes(depth_b1hw, rendered_bphw)
    if regressed:
        thr, T = None, 1
    elif bins is not None:
        thr, T = bin_thresholds.contiguous(), 1
        if thr.numel() != bins.numel():
            raise _lib.IdhError("Thresholder needs one threshold per bin")
        bins = bins.contiguous()
    else:
        thr, T = torch.tensor([float(t) for t in thresholds], device=dev, dtype=torch.float32), len(thresholds)
    keep = [prediction.contiguous(), rendered_bphw.contiguous(), gt_b1HW.contiguous(), None if depth_b1hw is None else depth_b1hw.contiguous()]
    a = _lib.EvalArgs()
    a.prediction, a.rendered_bphw, a.gt_b1HW, a.depth_b1hw = [_lib.ptr(t) for t in keep]
    a.pred_kind = _lib.EVAL_PRED_DEPTH if regressed else _lib.EVAL_PRED_LOGITS
    a.sampling = _lib.EVAL_NEAREST if nearest else _lib.EVAL_BILINEAR
    a.sigmoid_multiplier, a.surface_threshold = float(sigmoid_multiplier), float(surface_threshold)
    a.thresholds, a.bins = _lib.ptr(thr), _lib.ptr(bins)
    a.T, a.n_bins, a.tag_mask = T, 0 if bins is None or regressed else bins.numel(), tag_mask
    a.B, a.P, a.h, a.w, a.H, a.W = B, P, h, w, H, W
    out = torch.empty(B, len(TAGS), P, T, 3, device=dev)
    counts = torch.empty(B, len(TAGS), P, 2 + 2 * T, device=dev, dtype=torch.int32) if return_counts else None
    ws, nbytes = _workspace(B, P, h, w, H, W, T, dev)
    _lib.check(_lib.lib().idh_eval_plane_scores_fwd(C.byref(a), out.data_ptr(), _lib.ptr(counts), ws.data_ptr(), nbytes, _lib.stream_ptr()),
               "idh_eval_plane_scores_fwd")
    return (out, counts) if return_counts else out


def upsampled_depth_metrics(gt_b1HW, pred_b1hw, nearest=False, valid_above=0.5, mult_a=False) -> Dict[str, torch.Tensor]:
    """compute_depth_metrics_batched(gt, F.interpolate(pred, gt's size, "nearest" / "bilinear"), gt > valid_above, mult_a)."""
    _lib.require_cuda_f32(gt_b1HW, pred_b1hw)
    B, _, H, W = gt_b1HW.shape
    if pred_b1hw.dim() != 4 or pred_b1hw.shape[:2] != (B, 1) or gt_b1HW.shape[1] != 1:
        raise _lib.IdhError(f"upsampled_depth_metrics: gt {tuple(gt_b1HW.shape)} and prediction {tuple(pred_b1hw.shape)} must be (B,1,.,.)")
    h, w = pred_b1hw.shape[-2:]
    g, p = gt_b1HW.contiguous(), pred_b1hw.contiguous()
    out = torch.empty(B, len(DEPTH_METRIC_KEYS), device=g.device)
    ws, nbytes = _workspace(B, 1, h, w, H, W, 1, g.device)
    _lib.check(_lib.lib().idh_eval_depth_metrics_fwd(g.data_ptr(), p.data_ptr(), B, h, w, H, W, _lib.EVAL_NEAREST if nearest else _lib.EVAL_BILINEAR,
                                                     float(valid_above), int(mult_a), out.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()),
               "idh_eval_depth_metrics_fwd")
    return {k: out[:, i] for i, k in enumerate(DEPTH_METRIC_KEYS)}


def _keep(gt_b1HW, thresh):
    return (gt_b1HW.flatten(1) > thresh).any(1)


def _tag_scores(out, names, is_rendering):
    scores: Dict[str, torch.Tensor] = {}
    for i, tag in enumerate(TAGS):
        scores.update(_EV._scores(out[:, i], names, is_rendering, tag, _PLANES))
    return scores


def _names(thresholder, evaluator_thresholds):
    return [""] if thresholder is not None else [f"{float(t):.1f}_" for t in evaluator_thresholds]


def bd_score_keys(P, thresholder=None, evaluator_thresholds=np.linspace(0.3, 0.7, 5), temporal_eval=False, binary_eval_depth=False):
    """The keys, in order, of bd_frame_scores' dict for P query planes (no device work)."""
    if binary_eval_depth:
        return list(DEPTH_METRIC_KEYS)
    names = _names(thresholder, evaluator_thresholds)
    return list(_tag_scores(torch.zeros(1, len(TAGS), P, len(names), 3), names, temporal_eval))


def reg_score_keys(P, regression_plane_eval=False, temporal_eval=False):
    """The keys, in order, of reg_frame_scores' dict for P query planes (no device work)."""
    if not regression_plane_eval:
        return list(DEPTH_METRIC_KEYS)
    return list(_tag_scores(torch.zeros(1, len(TAGS), P, 1, 3), [""], temporal_eval))


def bd_frame_scores(outputs, cur_data, thresholder=None, evaluator_thresholds=np.linspace(0.3, 0.7, 5), bd_sigmoid_multiplier=1.0,
                    temporal_eval=False, binary_eval_depth=False):
    """test_bd.py:185-318 for one batch: ``(metrics_b_dict, keep_b)``.

    ``outputs``: BDModel.forward's outputs as returned (``pred_0`` logits; ``search_depths`` with ``binary_eval_depth``);
    ``cur_data``: ``depth_b1hw``, ``rendered_depth`` (B, P, h, w) and ``full_res_depth_b1hw``.  ``metrics_b_dict`` has the keys, in
    order, and the values test_bd.py builds; ``keep_b`` (B,) bool is its per-frame test (:275, :323): the frames whose rows it keeps.
    Neither argument is modified."""
    gt = cur_data["full_res_depth_b1hw"]
    if binary_eval_depth:
        scores = upsampled_depth_metrics(gt, outputs["search_depths"], nearest=True, valid_above=0.5, mult_a=False)
        return scores, _keep(gt, 0.5)
    if thresholder is not None:
        dev = gt.device
        thr = dict(bins=thresholder.bins.to(dev).float(), bin_thresholds=thresholder.thresholds.to(dev).float())
    else:
        thr = dict(thresholds=[float(t) for t in evaluator_thresholds])
    out = plane_scores(outputs["pred_0"], cur_data["rendered_depth"], gt, cur_data["depth_b1hw"], nearest=temporal_eval,
                       sigmoid_multiplier=bd_sigmoid_multiplier, **thr)
    return _tag_scores(out, _names(thresholder, evaluator_thresholds), temporal_eval), _keep(gt, 0.0)


def reg_frame_scores(outputs, cur_data, regression_plane_eval=False, temporal_eval=False):
    """test_reg.py:189-268 for one batch: ``(metrics_b_dict, keep_b)`` from DepthModel's ``depth_pred_s0_b1hw`` — the regressed-depth
    plane IoU for the three families with ``regression_plane_eval``, else the depth metrics (mult_a=True) over gt > 0.5."""
    gt = cur_data["full_res_depth_b1hw"]
    pred = outputs["depth_pred_s0_b1hw"]
    if regression_plane_eval:
        out = plane_scores(pred, cur_data["rendered_depth"], gt, cur_data["depth_b1hw"], regressed=True, nearest=temporal_eval)
        return _tag_scores(out, [""], temporal_eval), _keep(gt, 0.0)
    return upsampled_depth_metrics(gt, pred, nearest=temporal_eval, valid_above=0.5, mult_a=True), _keep(gt, 0.5)


class TemporalEvaluator:
    """The reference's ``TemporalEvaluator`` (utils/binary_metrics_utils.py:247-280): over a window of frames, how often the occlusion
    decision at a ground-truth vertex flips.  The renders and the vertex sampling are ``raster.MeshDepthRasterizer``'s kernels; the
    flip count of GPU histories is csrc/raster.hip's integer count.  INTEGRATION.md §2e shows the loop of test_bd.py:157-236 with it."""

    def __init__(self):
        self.rasterizer = None
        self.total_diffs = 0
        self.total_verts = 0

    def initialise_new_scene(self, gt_mesh_path=None, height=192, width=256, verts=None, faces=None, device="cuda"):
        from .raster import MeshDepthRasterizer

        self.rasterizer = MeshDepthRasterizer(height=height, width=width)
        self.rasterizer.load_gt_mesh(gt_mesh_path, verts=verts, faces=faces, device=device)

    def initialise_new_plane(self, depth_gt_b1hw, world_T_cam_b44):
        self.rasterizer.create_plane_from_camera(world_T_cam_b44, distance=torch.nanquantile(depth_gt_b1hw, 0.75))
        self.rasterizer.gt_vertex_predictions = []

    @staticmethod
    def mask_prediction_edges(prediction, edge_size=4):
        """In place, as the reference: -1 on the ``edge_size`` border rows and columns (everywhere when the map is too small to
        have an interior, which is what the reference's mask does)."""
        H, W = prediction.shape[-2:]
        if H <= 2 * edge_size or W <= 2 * edge_size:
            prediction[...] = -1.0
            return
        prediction[..., :edge_size, :] = -1.0
        prediction[..., -edge_size:, :] = -1.0
        prediction[..., :, :edge_size] = -1.0
        prediction[..., :, -edge_size:] = -1.0

    def update_vertex_predictions(self, prediction, cam_T_world_b44, K_b44):
        self.mask_prediction_edges(prediction)
        self.rasterizer.update_gt_vertex_predictions(prediction, cam_T_world_b44, K_b44)

    def compute_vertex_occlusion_changes(self):
        predictions = torch.stack(self.rasterizer.gt_vertex_predictions).float()
        if predictions.is_cuda:
            from .raster import vertex_occlusion_changes

            diffs = vertex_occlusion_changes(predictions)
        else:  # host tensors (fixtures, tests): the reference's own statement (:274-279)
            predictions = predictions.clone()
            predictions[predictions == -1] = torch.nan
            predictions[predictions > 0.5] = 1
            predictions[predictions < 0.5] = 0
            diffs = float(torch.nansum(torch.abs(predictions[1:] - predictions[:-1]).double()))
        self.total_diffs += diffs
        self.total_verts += predictions.shape[1]


def temporal_final_metrics(total_diffs, eval_length, warmup, eval_frame_multiplier, n_scans, temporal_d=-1):
    """The two entries test_bd.py:451-459 adds to the final metrics."""
    return {f"total_diffs_d_{temporal_d:.1f}": total_diffs,
            f"temporal_score_d_{temporal_d:.1f}": total_diffs / ((eval_length - warmup) * eval_frame_multiplier * n_scans)}


def bd_val_losses(outputs, cur_data, bd_regularisation_weight, edge_regularision=True, binary_loss_weighting=1.0, *, positive_weight=1.0,
                  return_counts=False, max_workgroups=0) -> Dict[str, torch.Tensor]:
    """The validation losses of a ``BDModel``: ``compute_losses("val" / "test", cur_data, outputs)`` of the reference
    (experiment_modules/bd_model.py:451-503, the ``phase != "train"`` branch), forward value only, in two launches
    (idh_bd_val_losses_fwd; contract: include/idh_geometry.h).  Reads ``outputs["pred_0"]`` (B,D,h,w),
    ``cur_data["rendered_depth"]`` (B,D,h,w), ``cur_data["depth_b1hw"]`` and - with ``edge_regularision``, the reference's
    ``run_opts.bd_edge_regularision`` - ``cur_data["edge_mask"]`` (``geometry.edge_mask``; ``fused_forward(native_edge_mask=True)`` fills
    it).  ``positive_weight`` is ``run_opts.binary_loss_positive_weight``.  Returns the reference's dictionary: ``binary_loss/0``,
    ``reg_loss/0``, ``binary_loss`` (their weighted sum) and ``loss`` (``binary_loss * binary_loss_weighting``), 0-d fp32 tensors on the
    device; nothing is synchronised.  Because of that the per-scale entries are always present: where the reference has none - no pixel
    with ``depth > 0`` and ``rendered > 0`` - they are NaN and ``binary_loss`` is 0, its edge case; an empty ``reg_mask`` gives a NaN
    ``reg_loss/0`` as the reference's mean of nothing does.  ``return_counts`` adds ``"counts"``: int64 (2,), the sizes of the two masks.
    Deterministic, and the same for every ``max_workgroups`` (0: the default grid).  There is no CPU fallback and no backward pass."""
    pred, rendered, depth = outputs["pred_0"], cur_data["rendered_depth"], cur_data["depth_b1hw"]
    edge = cur_data["edge_mask"] if edge_regularision else None
    _lib.require_cuda_f32(pred, rendered, depth, edge)
    if pred.dim() != 4 or rendered.shape != pred.shape:
        raise _lib.IdhError(f"pred_0 {tuple(pred.shape)} and rendered_depth {tuple(rendered.shape)} must both be (B,D,h,w)")
    B, D, h, w = pred.shape
    for name, t in (("depth_b1hw", depth), ("edge_mask", edge)):
        if t is not None and tuple(t.shape) != (B, 1, h, w):
            raise _lib.IdhError(f"{name} {tuple(t.shape)} must be ({B},1,{h},{w})")
    if min(B, D, h, w) < 1:
        raise _lib.IdhError(f"pred_0 {tuple(pred.shape)} is empty")
    if torch.is_grad_enabled() and pred.requires_grad:
        raise _lib.IdhError("bd_val_losses is forward only (no backward pass): detach pred_0 or call it under torch.no_grad()")
    keep = [pred.contiguous(), rendered.contiguous(), depth.contiguous()]
    a = _lib.BdValLossesArgs()
    a.pred_bdhw, a.rendered_bdhw, a.depth_b1hw = (t.data_ptr() for t in keep)
    if edge is not None:
        keep.append(edge.contiguous())
        a.edge_mask_b1hw = keep[-1].data_ptr()
    out = torch.empty(5, device=pred.device, dtype=torch.float64)
    nbytes = _lib.lib().idh_bd_val_losses_workspace_bytes(B, D, h, w)
    workspace = torch.empty(nbytes // 8, device=pred.device, dtype=torch.float64)
    a.out5, a.workspace, a.workspace_bytes = out.data_ptr(), workspace.data_ptr(), nbytes
    a.bd_regularisation_weight, a.positive_weight, a.max_workgroups = float(bd_regularisation_weight), float(positive_weight), int(max_workgroups)
    a.B, a.D, a.h, a.w = B, D, h, w
    _lib.check(_lib.lib().idh_bd_val_losses_fwd(a, _lib.stream_ptr()), "idh_bd_val_losses_fwd")
    f = out.float()
    losses = {"binary_loss/0": f[2], "reg_loss/0": f[3], "binary_loss": f[4]}
    losses["loss"] = f[4] if binary_loss_weighting == 1.0 else f[4] * binary_loss_weighting
    if return_counts:
        losses["counts"] = out[:2].long()
    return losses


REG_LOSS_KEYS = ("loss", "si_loss", "grad_loss", "abs_loss", "normals_loss", "ms_loss", "inv_abs_loss", "log_l1_loss", "mv_loss")  # out16[:9]
REG_COUNT_KEYS = ("grad_s0", "grad_s1", "grad_s2", "grad_s3", "mask_b", "mask_b_limit", "normals")  # out16[9:]


def _forward_only(what, named):
    if torch.is_grad_enabled():
        for name, t in named:
            if t is not None and t.requires_grad:
                raise _lib.IdhError(f"{what} is forward only (no backward pass): detach {name} or call it under torch.no_grad()")


def _map(name, t, B, C, h, w):
    if t.dim() != 4 or tuple(t.shape) != (B, C, h, w):
        raise _lib.IdhError(f"{name} {tuple(t.shape)} must be ({B},{C},{h},{w})")
    return t.contiguous()


def reg_losses_call(depth_gt=None, depth_pred=None, mask_b=None, log_preds=(), normals_gt=None, normals_pred=None, mv_loss=None, *, terms=0,
                    hypersim=False, si_lambda=0.85, num_scales=4, max_workgroups=0):
    """One idh_reg_val_losses_fwd: the float64 (16,) device tensor of include/idh_geometry.h's ``out16``.  The shape checks of
    ``reg_val_losses``, ``losses.MSGradientLoss`` and ``losses.NormalsLoss``; ``log_preds``: up to four tensors or None, by scale."""
    first = depth_gt if depth_gt is not None else normals_gt
    _lib.require_cuda_f32(depth_gt, depth_pred, normals_gt, normals_pred, mv_loss, *log_preds)
    if first.dim() != 4:
        raise _lib.IdhError(f"{'depth_b1hw' if depth_gt is not None else 'normals_b3hw'} {tuple(first.shape)} must have four dimensions")
    B, _, h, w = first.shape
    keep = []
    a = _lib.RegValLossesArgs()
    if depth_gt is not None:
        keep += [_map("depth_b1hw", depth_gt, B, 1, h, w), _map("depth_pred_s0_b1hw", depth_pred, B, 1, h, w)]
        a.depth_gt_b1hw, a.depth_pred_b1hw = keep[-2].data_ptr(), keep[-1].data_ptr()
    if mask_b is not None:
        if not mask_b.is_cuda or mask_b.dtype != torch.bool:
            raise _lib.IdhError(f"mask_b_b1hw must be a bool tensor on the MI355X, got {mask_b.dtype} on {mask_b.device}")
        keep.append(_map("mask_b_b1hw", mask_b, B, 1, h, w))
        a.mask_b_b1hw = keep[-1].data_ptr()
    for i, t in enumerate(log_preds):
        if t is None:
            continue
        name = f"log_depth_pred_s{i}_b1hw"
        if t.dim() != 4 or tuple(t.shape[:2]) != (B, 1) or min(t.shape[2:]) < 1 or h % t.shape[2] or w % t.shape[3]:
            raise _lib.IdhError(f"{name} {tuple(t.shape)} must be ({B},1,h_i,w_i) with h_i dividing {h} and w_i dividing {w} (an integer "
                                "ratio: nearest-neighbour resizing by another ratio is not covered)")
        keep.append(t.contiguous())
        a.log_depth_pred_s[i], a.scale_h[i], a.scale_w[i] = keep[-1].data_ptr(), t.shape[2], t.shape[3]
    if normals_gt is not None:
        keep += [_map("normals_b3hw", normals_gt, B, 3, h, w), _map("normals_pred_b3hw", normals_pred, B, 3, h, w)]
        a.normals_gt_b3hw, a.normals_pred_b3hw = keep[-2].data_ptr(), keep[-1].data_ptr()
    if mv_loss is not None:
        if mv_loss.numel() != 1:
            raise _lib.IdhError(f"mv_loss {tuple(mv_loss.shape)} must hold one value")
        keep.append(mv_loss.contiguous())
        a.mv_loss = keep[-1].data_ptr()
    dev = first.device
    out = torch.empty(16, device=dev, dtype=torch.float64)
    if min(B, h, w) < 1:
        raise _lib.IdhError(f"the maps {tuple(first.shape)} are empty")
    nbytes = _lib.lib().idh_reg_val_losses_workspace_bytes(B, h, w)
    workspace = torch.empty(max(nbytes, 8) // 8, device=dev, dtype=torch.float64)
    a.out16, a.workspace, a.workspace_bytes = out.data_ptr(), workspace.data_ptr(), nbytes
    a.si_lambda, a.hypersim, a.num_scales, a.terms, a.max_workgroups = float(si_lambda), int(bool(hypersim)), int(num_scales), int(terms), int(max_workgroups)
    a.B, a.h, a.w = B, h, w
    _lib.check(_lib.lib().idh_reg_val_losses_fwd(a, _lib.stream_ptr()), "idh_reg_val_losses_fwd")
    return out


def reg_val_losses(outputs, cur_data, src_data=None, *, hypersim=False, si_lambda=0.85, compute_normals=False, return_counts=False,
                   max_workgroups=0) -> Dict[str, torch.Tensor]:
    """The validation losses of a ``DepthModel``: ``compute_losses(cur_data, src_data, outputs)`` of the reference
    (experiment_modules/depth_model.py:442-540), forward value only, in at most five launches - one per level of the gradient pyramid,
    the first of which also evaluates every point-wise term and the normals, and a finalise (idh_reg_val_losses_fwd; contract:
    include/idh_geometry.h) - plus ``geometry.depth_consistency(return_loss=True)`` for the multi-view term, whose
    device scalar the finalise reads in stream order.  No kornia, nothing is synchronised.

    Reads ``outputs["depth_pred_s0_b1hw"]``, the ``outputs["log_depth_pred_s{i}_b1hw"]`` that are present (scale 0 must be; sizes that
    divide the depth map's), ``outputs["normals_pred_b3hw"]``; ``cur_data["depth_b1hw"]``, ``["mask_b_b1hw"]`` (bool), ``["normals_b3hw"]``,
    ``["invK_s0_b44"]``, ``["world_T_cam_b44"]``; ``src_data["depth_b1hw"]`` (B,K,1,h,w), ``["K_s0_b44"]``, ``["cam_T_world_b44"]``.
    ``hypersim`` is ``run_opts.dataset == "hypersim"``: ``grad_loss``, ``normals_loss`` and ``mv_loss`` are 0 and neither normals nor
    ``src_data`` are read.  ``compute_normals`` fills a missing ``normals_b3hw`` / ``normals_pred_b3hw`` with ``geometry.depth_normals`` of
    the depth (what ``DepthModel.step`` does, :565-570); neither dictionary is modified.  Returns the reference's nine entries as 0-d fp32
    device tensors; ``return_counts`` adds ``"counts"``: a dict of 0-d int64 tensors, the number of elements behind every mean
    (``REG_COUNT_KEYS``).  A mean over nothing is NaN, as in the reference.  Deterministic, and the same for every ``max_workgroups``
    (0: the default grid).  There is no CPU fallback and no backward pass."""
    present = [outputs.get(f"log_depth_pred_s{i}_b1hw") for i in range(4)]
    if all(t is None for t in present):
        raise _lib.IdhError("Could not find a valid scale to compute si loss!")  # (depth_model.py:496)
    for key in ("depth_pred_s0_b1hw", "log_depth_pred_s0_b1hw"):
        if outputs.get(key) is None:
            raise _lib.IdhError(f"reg_val_losses needs outputs['{key}']")
    depth_gt, depth_pred, mask_b = cur_data["depth_b1hw"], outputs["depth_pred_s0_b1hw"], cur_data["mask_b_b1hw"]
    _forward_only("reg_val_losses", [("depth_pred_s0_b1hw", depth_pred)] + [(f"log_depth_pred_s{i}_b1hw", t) for i, t in enumerate(present)] +
                  [("normals_pred_b3hw", outputs.get("normals_pred_b3hw"))])
    normals_gt = normals_pred = mv = None
    if not hypersim:
        if src_data is None:
            raise _lib.IdhError("reg_val_losses needs src_data (depth_b1hw, K_s0_b44, cam_T_world_b44) for mv_loss; only hypersim=True does without")
        from . import geometry

        normals_gt, normals_pred = cur_data.get("normals_b3hw"), outputs.get("normals_pred_b3hw")
        for name, t, depth in (("cur_data['normals_b3hw']", normals_gt, depth_gt), ("outputs['normals_pred_b3hw']", normals_pred, depth_pred)):
            if t is None and not compute_normals:
                raise _lib.IdhError(f"reg_val_losses needs {name}; compute_normals=True fills it with geometry.depth_normals")
        if normals_gt is None:
            normals_gt = geometry.depth_normals(depth_gt, cur_data["invK_s0_b44"])[0]
        if normals_pred is None:
            normals_pred = geometry.depth_normals(depth_pred, cur_data["invK_s0_b44"])[0]
        mv = geometry.depth_consistency(depth_pred, cur_data["invK_s0_b44"], cur_data["world_T_cam_b44"], src_data["depth_b1hw"],
                                        src_data["K_s0_b44"], src_data["cam_T_world_b44"], gate_depth=depth_gt, return_loss=True)["loss"]
    out = reg_losses_call(depth_gt, depth_pred, mask_b, present, normals_gt, normals_pred, mv, hypersim=hypersim, si_lambda=si_lambda,
                          max_workgroups=max_workgroups)
    f = out[:9].float()
    losses = {k: f[i] for i, k in enumerate(REG_LOSS_KEYS)}
    if return_counts:
        c = out[9:].long()
        losses["counts"] = {k: c[i] for i, k in enumerate(REG_COUNT_KEYS)}
    return losses
