"""Times the dense occlusion query in a moving camera (view_mlp_k, csrc/mlp_rays.hip) against what a caller had without it, B = 1 at the
full size: s0 map 192 x 256 (96 x 128 matching maps, D = 64, K = 7 dot-product volume, synthetic weights), P = 1, view maps 192 x 256
(49 152 pixels) and 480 x 640 (307 200).  One forward fills the decoder's scale-0 map; every timed call below reads it and runs no conv.
The view camera is the keyframe's moved and turned (tests' "moved" pose), the asset a fronto-parallel wall with holes.

"fused_ms": ``HotPath.query_view`` - one launch.  "composition_ms": the composition available before, timed in the same run: torch
back-projection of the depth map to a (1, N, 3) point list (pixel grid precomputed once, outside the window), ``HotPath.query_points``
(``project_points_k`` + ``ray_mlp_k``), then the ``where(valid, pred, fill)`` patch and the reshape.

HIP-event time over --iters back-to-back calls, divided by their number; --reps such windows per side, alternating, after one untimed
window of each; the median with the minimum and maximum beside it.  Host work of a call (ctypes, launches, torch allocations) is inside the
window.  Also reports whether both sides agree on validity and the largest difference of their logits.  Prints one JSON line; --out also writes it.

    python tools/perf_view_queries.py --reps 7 --iters 20 --out profiles/view_queries/run.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from perf_ray_queries import _measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_view_queries.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from implicit_depth_amd.pipeline import HotPath

    B, K, H, W, D = 1, 7, 96, 128, 64
    Hs, Ws = 2 * H, 2 * W
    cve = net.CVEncoder(D, [48, 64, 160, 256], [64, 128, 256, 384])
    dec = net.BDDecoderPP([24] + cve.num_ch_enc)
    mnet = net.BinaryMLPNetwork(dec.num_ch_dec)
    for i, m in enumerate([cve, dec, mnet]):
        syn.fill_state_dict(m, seed=50 + i, gain=1.1 if i == 2 else 1.0)
    hot = HotPath(CostVolumeManager(H, W, D), cve, dec, mnet).cuda()
    d = {k: v.cuda() for k, v in syn.cost_volume_inputs(B, K, 16, H, W, seed=0, behind_view=K - 1).items()}
    pyr = [t.cuda() for t in syn.encoder_pyramid(B, H * 4, W * 4, seed=0)]
    key = syn.source_pose(1)  # the keyframe's world_T_cam
    rel = torch.eye(4, dtype=torch.float64)
    c, s = math.cos(0.31), math.sin(0.31)
    rel[0, 0], rel[0, 2], rel[2, 0], rel[2, 2] = c, s, -s, c
    rel[:3, 3] = torch.tensor([0.35, -0.12, 0.2], dtype=torch.float64)
    wTc = (key @ rel).float()[None].cuda()
    cTw = torch.linalg.inv(key).float()[None].cuda()
    K0 = syn.intrinsics(Ws, Hs).float()[None].cuda()
    fill = -10.0
    res = {}
    with torch.inference_mode():
        hot(d["cur_feats"], d["src_feats"], pyr, d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"],
            rendered_depth=torch.full((B, 1, Hs, Ws), 2.0, device="cuda"))
        for h, w in ((192, 256), (480, 640)):
            g = torch.Generator().manual_seed(h)
            rendered = 1.5 + 2.0 * torch.rand((B, 1, h, w), generator=g)
            rendered[:, :, h // 3: h // 2, w // 4: w // 3] = 0.0  # a hole in the asset
            rendered = rendered.cuda()
            invK = torch.linalg.inv(syn.intrinsics(w, h)).float()[None].cuda()
            yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5, indexing="ij")
            pix = torch.stack([xx.reshape(-1), yy.reshape(-1), torch.ones(h * w)], 0).cuda()  # 3, N: BackprojectDepth's buffer

            def fused():
                return hot.query_view(rendered, invK, wTc, cTw, K0, fill=fill)

            def composition():
                cam = (invK[:, :3, :3] @ pix) * rendered.flatten(2)  # B, 3, N
                pts = (wTc[:, :3, :3] @ cam + wTc[:, :3, 3:]).transpose(1, 2)
                q = hot.query_points(pts, cTw, K0)
                ok = q["point_valid"] & (rendered.view(B, -1) > 0)
                return torch.where(ok, q["point_pred"].view(B, -1), torch.full_like(q["point_depth"], fill)).view(B, 1, h, w), ok.view(B, 1, h, w)

            r = {"pixels": h * w}
            r.update(_measure({"fused_ms": fused, "composition_ms": composition}, a.reps, a.iters))
            fo, (co, cok) = fused(), composition()
            pos = rendered > 0
            r["valid_share"] = fo["view_valid"].float().mean().item()
            r["valid_agree"] = bool(torch.equal(fo["view_valid"], cok))
            both = fo["view_valid"] & cok
            # (the composition's points come from a torch matmul, not from the kernel's fma chains: the same pixels up to their roundings)
            r["max_abs_diff"] = (fo["view_pred"] - co)[both].abs().max().item() if bool(both.any()) else 0.0
            r["positive_share"] = pos.float().mean().item()
            res[f"{h}x{w}"] = r
    res["device"] = torch.cuda.get_device_name(0)
    res["reps"], res["iters"] = a.reps, a.iters
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
