#!/usr/bin/env python
"""Golden of the first-hit march in a moving camera: per probe the chain of gen_golden_view_search.py composed from the REFERENCE's own
modules - ``BackprojectDepth`` in the view camera at the probe's depth (utils/geometry_utils.py:55-63), ``Project3D`` into the keyframe
camera (:77-89), ``F.grid_sample(bilinear, zeros, align_corners=False)`` of feature_s0 and ``BinaryMLPNetwork`` on ``[z | feature]`` -
inside the project's march rule (include/idh.h): the shared samples in turn until the first probe with sigmoid(pred) < 0.5, then
``refine`` steps of the bisection of ``BDModel.forward(infer_depth=True)`` (experiment_modules/bd_model.py:286-290) inside the bracket, on
the 12 x 16 map and the 7 x 9 moved view of view_search.npz.  A probe outside the image or behind the camera has the logit ``fill``.

The fixture holds the matrices and a checksum of the feature map, the final depths, ``hit_step`` (255 = none), the largest |logit| (the
scale of the logit tolerance), ``march_margin``: per ray the smallest |logit - 0| over the probes the ray EVALUATED, 0 when one of them lies
within view_query_ref.PROJ_MARGIN of the image's border, and ``sample_margin`` (n_march, B, h, w): the same per shared sample, reached or not.

    python tests/golden/gen_golden_view_march.py       # rewrites tests/golden/view_march.npz
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

    import view_march_ref as VM
    import view_search_ref as VS

    case = VM.GOLDEN_CASE
    net = VM.golden_net(BinaryMLPNetwork).eval()
    feat, (invK, wTc, cTw, K, _, _) = VS.golden_inputs()
    B, h, w, H, W = case.B, case.h, case.w, case.H, case.W
    q_s = torch.from_numpy(VM.samples(case))
    n, R = case.n_march, case.refine
    back, proj = BackprojectDepth(h, w), Project3D()
    scale = 0.0

    def probe(depth):
        """(logit with fill, this probe's margin: |pred| where valid, inf where invalid, 0 near the border)."""
        nonlocal scale
        pix = proj(back(depth, invK), K, torch.matmul(cTw, wTc))  # B, 3, hw: (u, v, z) in the keyframe camera
        u, v, z = (pix[:, i].reshape(B, 1, h, w) for i in range(3))
        locs = torch.stack([(u[:, 0] / W - 0.5) * 2, (v[:, 0] / H - 0.5) * 2], -1)
        f = F.grid_sample(feat, locs, mode="bilinear", padding_mode="zeros", align_corners=False)
        rows = torch.cat([z, f], 1).permute(0, 2, 3, 1)
        pred = net([rows], max_scale_only=True)["pred_0"].permute(0, 3, 1, 2)
        valid = (z > 1e-5) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        m = VS.PROJ_MARGIN
        edge = (z < 1e-5 + m) | (u.abs() < m) | ((u - W).abs() < m) | (v.abs() < m) | ((v - H).abs() < m)
        if valid.any():
            scale = max(scale, pred[valid].abs().max().item())
        margin = torch.where(edge, torch.zeros_like(pred), torch.where(valid, pred.abs(), torch.full_like(pred, float("inf"))))
        return torch.where(valid, pred, torch.full_like(pred, case.fill)), margin

    shape = (B, 1, h, w)
    st = torch.full(shape, -1, dtype=torch.long)  # -1 marching, k > 0 refining with k steps left, 0 done
    near, far, depth = torch.zeros(shape), torch.zeros(shape), torch.zeros(shape)
    hit = torch.full(shape, 255, dtype=torch.long)
    margin = torch.full(shape, float("inf"))
    sample_margin = []
    with torch.no_grad():
        for s in range(n):
            sample_margin.append(probe(torch.full(shape, q_s[s].item()))[1])
        for it in range(n + R):
            active = st != 0
            if not active.any():
                break
            marching = st < 0
            q = torch.where(marching, q_s[min(it, n - 1)], depth)
            logit, mg = probe(q)
            behind = torch.sigmoid(logit) < 0.5
            nfar, nnear = torch.where(behind, q, far), torch.where(behind, near, q)
            bracket = marching & behind & (it > 0)
            nst = torch.where(marching, torch.where(behind, torch.full_like(st, R if it > 0 else 0), torch.full_like(st, 0 if it == n - 1 else -1)), st - 1)
            ndepth = torch.where(bracket | ~marching, (nfar + nnear) / 2, q)
            margin = torch.where(active, torch.minimum(margin, mg), margin)
            hit = torch.where(active & marching & behind, torch.full_like(hit, it), hit)
            far, near, depth, st = (torch.where(active, a, b) for a, b in ((nfar, far), (nnear, near), (ndepth, depth), (nst, st)))
    save("view_march", feat_chk=chk(feat), invK=invK, world_T_cam=wTc, key_cam_T_world=cTw, key_K=K, march_depths=depth,
         hit_step=hit.to(torch.uint8), march_margin=margin, sample_margin=torch.stack(sample_margin), samples=q_s, logit_scale=torch.tensor(scale))
    print("  depths", tuple(depth.shape), "distinct", depth.unique().numel(), "hit steps", hit.unique().tolist())


if __name__ == "__main__":
    main()
