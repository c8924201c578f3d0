#!/usr/bin/env python
"""Golden of the depth search in a moving camera: per step the chain of gen_golden_view.py composed from the REFERENCE's own modules -
``BackprojectDepth`` in the view camera at the current search depth (utils/geometry_utils.py:55-63), ``Project3D`` into the keyframe camera
(:77-89), ``F.grid_sample(bilinear, zeros, align_corners=False)`` of feature_s0 and ``BinaryMLPNetwork`` on ``[z | feature]`` - inside the
bisection of ``BDModel.forward(infer_depth=True)`` (experiment_modules/bd_model.py:279-290: sigmoid(pred) < 0.5 moves the far bound,
otherwise the near bound, next depth the mean of the bounds), on a 12 x 16 map and a 7 x 9 moved view.  A probe that ``Project3D`` puts
outside the 12 x 16 image or behind the camera has the logit ``fill`` (the project's rule; the reference has no such case).

The fixture holds the matrices and a checksum of the feature map (it is a synthetic.py seed), the final depths, the largest |logit| (the scale of the logit tolerance) and ``search_margin``: per ray the
smallest |logit - 0| over the steps, 0 when a probe lies within view_query_ref.PROJ_MARGIN of the image's border.

    python tests/golden/gen_golden_view_search.py       # rewrites tests/golden/view_search.npz
"""
import os
import sys

os.environ["PYTORCH_JIT"] = "0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch
import torch.nn.functional as F

from gen_golden import chk, import_reference, save


def main():
    import_reference()
    from modules.networks import BinaryMLPNetwork
    from utils.geometry_utils import BackprojectDepth, Project3D

    import view_search_ref as VS

    case = VS.GOLDEN_CASE
    net = VS.golden_net(BinaryMLPNetwork).eval()
    feat, (invK, wTc, cTw, K, _, _) = VS.golden_inputs()
    B, h, w, H, W = case.B, case.h, case.w, case.H, case.W
    near = torch.full((B, 1, h, w), case.lo)
    far = torch.full((B, 1, h, w), case.hi)
    depth = torch.full((B, 1, h, w), (case.hi - case.lo) / 2)
    margin = torch.full((B, 1, h, w), float("inf"))
    scale = 0.0
    back, proj = BackprojectDepth(h, w), Project3D()
    with torch.no_grad():
        for _ in range(case.iters):
            pix = proj(back(depth, invK), K, torch.matmul(cTw, wTc))  # B, 3, hw: (u, v, z) in the keyframe camera
            u, v, z = (pix[:, i].reshape(B, 1, h, w) for i in range(3))
            locs = torch.stack([(u[:, 0] / W - 0.5) * 2, (v[:, 0] / H - 0.5) * 2], -1)
            f = F.grid_sample(feat, locs, mode="bilinear", padding_mode="zeros", align_corners=False)
            rows = torch.cat([z, f], 1).permute(0, 2, 3, 1)
            pred = net([rows], max_scale_only=True)["pred_0"].permute(0, 3, 1, 2)
            valid = (z > 1e-5) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
            m = VS.PROJ_MARGIN
            edge = (z < 1e-5 + m) | (u.abs() < m) | ((u - W).abs() < m) | (v.abs() < m) | ((v - H).abs() < m)
            logit = torch.where(valid, pred, torch.full_like(pred, case.fill))
            scale = max(scale, pred[valid].abs().max().item())
            margin = torch.minimum(margin, torch.where(edge, torch.zeros_like(pred), torch.where(valid, pred.abs(), margin)))
            visible = torch.sigmoid(logit) < 0.5
            far = torch.where(visible, depth, far)
            near = torch.where(visible, near, depth)
            depth = (far + near) / 2
    save("view_search", feat_chk=chk(feat), invK=invK, world_T_cam=wTc, key_cam_T_world=cTw, key_K=K, search_depths=depth, search_margin=margin,
         logit_scale=torch.tensor(scale))
    print("  depths", tuple(depth.shape), "distinct", depth.unique().numel())


if __name__ == "__main__":
    main()
