#!/usr/bin/env python
"""Golden of the dense occlusion query in a moving camera: the chain composed from the REFERENCE's own modules - ``BackprojectDepth`` in the
view camera (utils/geometry_utils.py:55-63), ``Project3D`` into the keyframe camera (:77-89) with the transform product of
``BDModel.sample_prior`` (experiment_modules/bd_model.py:400-403), ``F.grid_sample(bilinear, zeros, align_corners=False)`` of feature_s0
with that method's normalisation (:405-406) and ``BinaryMLPNetwork`` on ``[z | feature]``, z the depth ``Project3D`` returns.  The
reference is imported as gen_golden.py does (stub modules, PYTORCH_JIT=0).  Inputs and weights come from
``tests/view_query_ref.golden_inputs`` / ``ray_query_ref.golden_net`` (synthetic.py seeds); the fixture holds, per camera, the rendered
depth, the matrices and the logits of EVERY pixel (the test keeps the pixels its margin rule keeps).

    python tests/golden/gen_golden_view.py       # rewrites tests/golden/view_query.npz
"""
import os
import sys

os.environ["PYTORCH_JIT"] = "0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch
import torch.nn.functional as F

from gen_golden import import_reference, save


def main():
    import_reference()
    from modules.networks import BinaryMLPNetwork
    from utils.geometry_utils import BackprojectDepth, Project3D

    import ray_query_ref as Q
    import view_query_ref as V

    net = Q.golden_net(BinaryMLPNetwork).eval()
    out = {}
    for cam in V.GOLDEN_CAMERAS:
        feat, rendered, (invK, wTc, cTw, K, _, _) = V.golden_inputs(cam)
        B, _, h, w = rendered.shape
        H, W = feat.shape[2:]
        with torch.no_grad():
            cam_points = BackprojectDepth(h, w)(rendered, invK)                   # B, 4, hw: in the view camera
            pix = Project3D()(cam_points, K, torch.matmul(cTw, wTc))              # B, 3, hw: (u, v, z) in the keyframe camera
            locs = pix[:, :2].reshape(B, 2, h, w).permute(0, 2, 3, 1).clone()
            locs[..., 0] = (locs[..., 0] / W - 0.5) * 2
            locs[..., 1] = (locs[..., 1] / H - 0.5) * 2
            f = F.grid_sample(feat, locs, mode="bilinear", padding_mode="zeros", align_corners=False)  # B, C, h, w
            rows = torch.cat([pix[:, 2:3].reshape(B, 1, h, w), f], 1).permute(0, 2, 3, 1)
            pred = net([rows], max_scale_only=True)["pred_0"].permute(0, 3, 1, 2)  # B, 1, h, w
        out.update({f"{cam}_rendered": rendered, f"{cam}_invK": invK, f"{cam}_world_T_cam": wTc, f"{cam}_key_cam_T_world": cTw,
                    f"{cam}_key_K": K, f"{cam}_pred": pred})
        print(f"  {cam}: pred", tuple(pred.shape))
    save("view_query", **out)


if __name__ == "__main__":
    main()
