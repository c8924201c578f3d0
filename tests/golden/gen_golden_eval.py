#!/usr/bin/env python
"""Generate tests/golden/g14_eval_frame.npz: the reference's per-frame test evaluation (test_bd.py:185-318,
test_reg.py:189-268) replayed statement by statement on CPU with the reference's own get_surface_mask,
get_boundary_mask, sigmoid_custom, PlaneEvaluator, compute_depth_metrics_batched and F.interpolate.

Runs only where the reference checkout is (see gen_golden.py); inputs come from
``implicit_depth_amd.synthetic.eval_frame_case`` (seeded, basic arithmetic), so the fixture holds only outputs:
  masks      the surface / boundary masks of two cases, packed 0/1 bits;
  per case   the score dict's key list and values, keep_b, and for the plane IoU cases the integer counts
             {valid, target, pred[T], inter[T]} per (b, tag, d) from the reference's own thresholded tensors plus the
             number of valid pixels per (b, tag, d) within 2e-6 of their threshold after interpolation (relative 1e-6
             of the query for the regressed compare): an fp32 implementation may legitimately decide those either way.

    python tests/golden/gen_golden_eval.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch
import torch.nn.functional as F

from gen_golden import _stub_pytorch3d, _thresholder, import_reference, save  # noqa: E402  (also puts the repository root on sys.path)

# name, (B, P, h, w, H, W, seed), loop ("bd" = test_bd.py, "reg" = test_reg.py), options of that loop
CASES = [
    ("bd_thr", (2, 4, 192, 256, 480, 640, 1), "bd", dict(thresholder=True)),
    ("bd_const", (2, 4, 192, 256, 480, 640, 1), "bd", dict()),
    ("bd_thr_mult_odd", (2, 3, 100, 140, 333, 467, 2), "bd", dict(thresholder=True, bd_sigmoid_multiplier=2.5)),
    ("bd_temporal_odd", (2, 2, 100, 140, 333, 467, 3), "bd", dict(temporal_eval=True)),
    ("bd_eval_depth", (2, 4, 192, 256, 480, 640, 1), "bd", dict(binary_eval_depth=True)),
    ("reg_plane", (2, 4, 192, 256, 480, 640, 4), "reg", dict(regression_plane_eval=True)),
    ("reg_plane_temporal_odd", (2, 3, 100, 140, 333, 467, 5), "reg", dict(regression_plane_eval=True, temporal_eval=True)),
    ("reg_depth", (2, 1, 192, 256, 480, 640, 4), "reg", dict()),
    ("reg_depth_temporal_odd", (2, 1, 100, 140, 333, 467, 5), "reg", dict(temporal_eval=True)),
]
MASK_CASES = ("bd_thr", "bd_thr_mult_odd")
THR_MARGIN, REG_MARGIN = 2e-6, 1e-6


def _tagged_queries(cur_data, surface_mask_bdhw, boundary_mask_bdhw, size):
    """test_bd.py:244-264 (= test_reg.py:213-233)."""
    upsampled_query_bdhw = F.interpolate(cur_data["rendered_depth"], size=size, mode="nearest")
    boundary_query_bdhw = cur_data["rendered_depth"].clone()
    boundary_query_bdhw[~boundary_mask_bdhw.bool()] = -1
    boundary_query_bdhw = F.interpolate(boundary_query_bdhw, size=size, mode="nearest")
    surface_query_bdhw = cur_data["rendered_depth"].clone()
    surface_query_bdhw[~surface_mask_bdhw.bool()] = -1
    surface_query_bdhw = F.interpolate(surface_query_bdhw, size=size, mode="nearest")
    return upsampled_query_bdhw, surface_query_bdhw, boundary_query_bdhw


def replay_bd(outputs, cur_data, thresholder, evaluator, bd_sigmoid_multiplier=1.0, temporal_eval=False, binary_eval_depth=False):
    from modules.layers import sigmoid_custom
    from utils.binary_metrics_utils import get_boundary_mask, get_surface_mask
    from utils.metrics_utils import compute_depth_metrics_batched

    outputs, cur_data = dict(outputs), dict(cur_data)
    depth_gt_b1hw = cur_data["full_res_depth_b1hw"]
    surface_mask_bdhw = get_surface_mask(cur_data["depth_b1hw"], cur_data["rendered_depth"])
    boundary_mask_bdhw = get_boundary_mask(cur_data["depth_b1hw"], cur_data["rendered_depth"])
    outputs["pred_0"] = sigmoid_custom(outputs["pred_0"], multiplier=bd_sigmoid_multiplier)
    size = (depth_gt_b1hw.shape[-2], depth_gt_b1hw.shape[-1])
    upsampled_pred_bdhw = F.interpolate(outputs["pred_0"], size=size, mode="nearest" if temporal_eval else "bilinear")
    queries = _tagged_queries(cur_data, surface_mask_bdhw, boundary_mask_bdhw, size)
    if binary_eval_depth:
        upsampled_pred_bdhw = F.interpolate(outputs["search_depths"], size=size, mode="nearest")
    thresh_to_check = 0.5 if binary_eval_depth else 0.0
    valid_mask_b = cur_data["full_res_depth_b1hw"] > thresh_to_check
    if binary_eval_depth:
        metrics_b_dict = compute_depth_metrics_batched(depth_gt_b1hw.flatten(start_dim=1).float(), upsampled_pred_bdhw.flatten(start_dim=1).float(),
                                                       valid_mask_b.flatten(start_dim=1), mult_a=False)
    else:
        metrics_b_dict = {}
        for q, tag in zip(queries, (None, "surface", "boundary")):
            metrics_b_dict.update(evaluator.compute_batch_scores_test(query_depth_bdhw=q, gt_depth_b1hw=depth_gt_b1hw, prediction_bdhw=upsampled_pred_bdhw,
                                                                      is_rendering=temporal_eval, tag=tag, thresholder=thresholder))
    return metrics_b_dict, valid_mask_b, surface_mask_bdhw, boundary_mask_bdhw, queries, upsampled_pred_bdhw


def replay_reg(outputs, cur_data, plane_evaluator, regression_plane_eval=False, temporal_eval=False):
    from utils.binary_metrics_utils import get_boundary_mask, get_surface_mask
    from utils.metrics_utils import compute_depth_metrics_batched

    depth_gt = cur_data["full_res_depth_b1hw"]
    size = (depth_gt.shape[-2], depth_gt.shape[-1])
    upsampled_depth_pred_b1hw = F.interpolate(outputs["depth_pred_s0_b1hw"], size=size, mode="nearest" if temporal_eval else "bilinear")
    thresh_to_check = 0.0 if regression_plane_eval else 0.5
    valid_mask_b = cur_data["full_res_depth_b1hw"] > thresh_to_check
    queries = None
    if regression_plane_eval:
        surface_mask_bdhw = get_surface_mask(cur_data["depth_b1hw"], cur_data["rendered_depth"])
        boundary_mask_bdhw = get_boundary_mask(cur_data["depth_b1hw"], cur_data["rendered_depth"])
        queries = _tagged_queries(cur_data, surface_mask_bdhw, boundary_mask_bdhw, size)
        metrics_b_dict = {}
        for q, tag in zip(queries, (None, "surface", "boundary")):
            metrics_b_dict.update(plane_evaluator.compute_regressed_depth_batch_scores(query_depth_bdhw=q, gt_depth_b1hw=depth_gt,
                                                                                       prediction_b1hw=upsampled_depth_pred_b1hw, is_rendering=temporal_eval, tag=tag))
    else:
        metrics_b_dict = compute_depth_metrics_batched(depth_gt.flatten(start_dim=1).float(), upsampled_depth_pred_b1hw.flatten(start_dim=1).float(),
                                                       valid_mask_b.flatten(start_dim=1), mult_a=True)
    return metrics_b_dict, valid_mask_b, queries, upsampled_depth_pred_b1hw


def counts_and_margins(queries, gt_b1hw, pred_bdhw, thresholds=None, thresholder=None, regressed=False):
    """Integer counts (B, 3, P, 2 + 2T) and ambiguous-pixel counts (B, 3, P), from the reference's thresholded tensors
    (binary_metrics_utils.py:143-160 / :199-213)."""
    cnt, amb = [], []
    for q in queries:
        valid = (gt_b1hw.expand(q.shape) > 0) * (q > 0)
        target = (q < gt_b1hw.expand(q.shape)) & valid
        p = pred_bdhw.expand(q.shape)
        if regressed:
            preds = [q < p]
            near = (q - p).abs() <= REG_MARGIN * q.abs()
        elif thresholder is not None:
            t = thresholder.get_thresholds(q.flatten(2)).view(q.shape)
            preds = [p > t]
            near = (p - t).abs() <= THR_MARGIN
        else:
            preds = [p > float(t) for t in thresholds]
            near = torch.zeros_like(valid)
            for t in thresholds:
                near |= (p - float(t)).abs() <= THR_MARGIN
        s = lambda m: m.flatten(2).sum(2)
        cnt.append(torch.stack([s(valid), s(target)] + [s(pr & valid) for pr in preds] + [s(pr & valid & target) for pr in preds], 2))
        amb.append(s(near & valid))
    return torch.stack(cnt, 1).int(), torch.stack(amb, 1).int()


def main():
    import_reference()
    _stub_pytorch3d()
    import implicit_depth_amd.synthetic as syn
    from utils.binary_metrics_utils import PlaneEvaluator

    th = _thresholder()
    out = {"thr_planes": np.array([1.5 + 0.5 * i for i in range(8)], dtype=np.float32), "thr_values": th.thresholds.numpy(),
           "case_names": np.array([c[0] for c in CASES])}
    for name, shape, loop, opts in CASES:
        print("G14", name)
        B, P, h, w, H, W, seed = shape
        outputs, cur = syn.eval_frame_case(B, P, h, w, H, W, seed)
        before = {k: v.clone() for k, v in {**outputs, **cur}.items()}
        out[f"{name}__case"] = np.array(json.dumps(dict(shape=shape, loop=loop, opts=opts)))
        counts = None
        if loop == "bd":
            thresholder = th if opts.get("thresholder") else None
            ev = PlaneEvaluator()
            sc, keep, sm, bm, queries, up = replay_bd(outputs, cur, thresholder, ev, opts.get("bd_sigmoid_multiplier", 1.0),
                                                      opts.get("temporal_eval", False), opts.get("binary_eval_depth", False))
            if not opts.get("binary_eval_depth"):
                counts, amb = counts_and_margins(queries, cur["full_res_depth_b1hw"], up, thresholds=ev.thresholds, thresholder=thresholder)
            if name in MASK_CASES:
                out[f"{name}__surface_bits"] = np.packbits(sm.numpy().astype(np.uint8).ravel())
                out[f"{name}__boundary_bits"] = np.packbits(bm.numpy().astype(np.uint8).ravel())
                print(f"  surface {sm.mean():.3f} boundary {bm.mean():.3f} of pixels")
        else:
            sc, keep, queries, up = replay_reg(outputs, cur, PlaneEvaluator(), opts.get("regression_plane_eval", False), opts.get("temporal_eval", False))
            if queries is not None:
                counts, amb = counts_and_margins(queries, cur["full_res_depth_b1hw"], up, regressed=True)
        for k, v in {**outputs, **cur}.items():
            assert torch.equal(torch.nan_to_num(v), torch.nan_to_num(before[k])), f"{name}: the replay modified {k}"
        keys = list(sc)
        out[f"{name}__keys"] = np.array(keys)
        out[f"{name}__values"] = torch.stack([sc[k].float() for k in keys], 1).numpy()
        out[f"{name}__keep"] = keep.flatten(1).any(1).numpy()
        if counts is not None:
            out[f"{name}__counts"] = counts.numpy()
            out[f"{name}__ambiguous"] = amb.numpy()
            print(f"  {len(keys)} keys, ambiguous pixels per (b, tag, d): max {int(amb.max())}, zero in {float((amb == 0).float().mean()):.2f}")
    save("g14_eval_frame", **out)


if __name__ == "__main__":
    main()
