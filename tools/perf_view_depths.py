"""Times the depth search in a moving camera (view_search_k, csrc/mlp_rays.hip) against what a caller had without it, B = 1 at the full
size: s0 map 192 x 256 (96 x 128 matching maps, D = 64, K = 7 dot-product volume, synthetic weights), the view camera the keyframe's moved
and turned (tests' "moved" pose, as tools/perf_view_queries.py), views 192 x 256 (49 152 rays), 480 x 640 (307 200) and a list of 64 rays.
One forward fills the decoder's scale-0 map; every timed call below reads it and runs no conv.

"fused_ms": ``HotPath.query_view_depths`` - one launch, twelve steps in registers.  "composition_ms": the composition available before,
timed in the same run: twelve ``HotPath.query_view`` calls on rendered = q_n with the rule in torch between them (threshold 0.5, the flag
byte kept as the fused call keeps it).  A ray list has no depth map; the 64 rays are the pixel centres of an 8 x 8 view, which both sides
can express (the fused side takes them as a list).

HIP-event time over --iters back-to-back calls, divided by their number; --reps such windows per side, alternating, after one untimed
window of each; the median with the minimum and maximum beside it.  Host work of a call (ctypes, launches, torch allocations) is inside the
window.  Also reports whether both sides give the same bits.  Prints one JSON line; --out also writes it.

    python tools/perf_view_depths.py --reps 7 --iters 10 --out profiles/view_depths/run.json
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

ITERS, LO, HI = 12, 0.5, 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_view_depths.py measures on the GPU; none is visible")
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
        for name, (h, w), listed in (("192x256", (192, 256), False), ("480x640", (480, 640), False), ("list64", (8, 8), True)):
            invK = torch.linalg.inv(syn.intrinsics(w, h)).float()[None].cuda()
            yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5, indexing="ij")
            rays = torch.stack([xx, yy], -1).view(1, h * w, 2).cuda()

            def fused():
                if listed:
                    return hot.query_view_depths(invK, wTc, cTw, K0, rays=rays, fill=fill)
                return hot.query_view_depths(invK, wTc, cTw, K0, size=(h, w), fill=fill)

            def composition():
                lo, hi = torch.full((B, 1, h, w), LO, device="cuda"), torch.full((B, 1, h, w), HI, device="cuda")
                sd = (hi - lo) * 0.5
                flags = torch.zeros(B, 1, h, w, dtype=torch.uint8, device="cuda")
                for _ in range(ITERS):
                    v = hot.query_view(sd, invK, wTc, cTw, K0, fill=fill)
                    vis = v["view_pred"] < 0.0  # logit(0.5)
                    hi, lo = torch.where(vis, sd, hi), torch.where(vis, lo, sd)
                    flags |= (torch.where(vis, 1, 2) | torch.where(v["view_valid"], 0, 4)).to(torch.uint8)
                    sd = (hi + lo) * 0.5
                return sd, v["view_pred"], flags

            r = {"rays": h * w}
            r.update(_measure({"fused_ms": fused, "composition_ms": composition}, a.reps, a.iters))
            fo, (sd, pred, flags) = fused(), composition()
            r["bitwise_equal_to_composition"] = bool(torch.equal(fo["view_search_depths"].reshape(-1), sd.reshape(-1))
                                                     and torch.equal(fo["view_search_logits"].reshape(-1), pred.reshape(-1))
                                                     and torch.equal(fo["view_search_flags"].reshape(-1), flags.reshape(-1)))
            fl = fo["view_search_flags"]
            r["bracketed_share"] = (fl == 3).float().mean().item()
            r["some_probe_invalid_share"] = ((fl & 4) != 0).float().mean().item()
            res[name] = r
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
