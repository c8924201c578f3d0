"""Times the occlusion and depth queries in a moving camera against several remembered keyframes (view_keys_k / view_keys_search_k,
csrc/mlp_rays.hip) against what a caller could compose without them, B = 1 at the full size: s0 map 192 x 256 (96 x 128 matching maps,
D = 64, K = 7 dot-product volume, synthetic weights), M = 4 predictions on different inputs remembered with the keyframe pose yawed by
+0.45, +0.15, -0.15, -0.45 rad (and moved by centimetres), the live camera at the keyframe pose, moved a little, behind a lens half as
long; views 192 x 256 (49 152 pixels) and 480 x 640 (307 200).  The keys are asked newest first, which is ascending yaw here.

"fused_ms": ``HotPath.query_view_keys`` / ``query_view_depths_keys`` - one launch, one MLP pass per pixel (and step).
"composition_ms": M single-key launches (``mlp.view_logits``, what ``HotPath.query_view`` runs) on one remembered feature map each -
the maps a caller would have had to copy aside by hand - plus the torch first-valid select; for the search the twelve-step host loop
over that (threshold 0.5, the flag byte kept as the fused call keeps it).  Both sides in the same run, alternating windows.

HIP-event time over --iters back-to-back calls, divided by their number; --reps such windows per side, alternating, after one untimed
window of each; the median with the minimum and maximum beside it.  Host work of a call (ctypes, launches, torch allocations) is inside the
window.  Also reports whether both sides give the same bits, and the share of pixels (probes, for the search) served by each key and by
none: a tile without a valid pixel skips the MLP on both sides, so the shares tell a gain of the skip from one of the fusion.  Prints one
JSON line; --out also writes it.

    python tools/perf_view_keys.py --reps 7 --iters 10 --out profiles/view_keys/run.json
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

ITERS, LO, HI, NONE = 12, 0.5, 8.0, 255
YAWS = (0.45, 0.15, -0.15, -0.45)  # in the order the predictions are remembered
SHIFTS = ((0.03, -0.01, 0.02), (-0.02, 0.015, -0.01), (0.01, 0.02, 0.03), (0.0, -0.02, 0.01))


def _yaw(theta, t):
    T = torch.eye(4, dtype=torch.float64)
    c, s = math.cos(theta), math.sin(theta)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = c, s, -s, c
    T[:3, 3] = torch.tensor(t, dtype=torch.float64)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_view_keys.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import mlp, nhwc
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from implicit_depth_amd.pipeline import HotPath

    B, K, H, W, D = 1, 7, 96, 128, 64
    Hs, Ws, M = 2 * H, 2 * W, len(YAWS)
    cve = net.CVEncoder(D, [48, 64, 160, 256], [64, 128, 256, 384])
    dec = net.BDDecoderPP([24] + cve.num_ch_enc)
    mnet = net.BinaryMLPNetwork(dec.num_ch_dec)
    for i, m in enumerate([cve, dec, mnet]):
        syn.fill_state_dict(m, seed=50 + i, gain=1.1 if i == 2 else 1.0)
    hot = HotPath(CostVolumeManager(H, W, D), cve, dec, mnet).cuda()
    key = syn.source_pose(1)  # the keyframe's world_T_cam
    wTc = (key @ _yaw(0.0, (0.02, -0.015, 0.01))).float()[None].cuda()
    K0 = syn.intrinsics(Ws, Hs).float()[None].cuda()
    fill = -10.0
    res = {}
    with torch.inference_mode():
        for s in range(M):
            d = {k: v.cuda() for k, v in syn.cost_volume_inputs(B, K, 16, H, W, seed=s, behind_view=K - 1).items()}
            pyr = [t.cuda() for t in syn.encoder_pyramid(B, H * 4, W * 4, seed=s)]
            hot(d["cur_feats"], d["src_feats"], pyr, d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"],
                rendered_depth=torch.full((B, 1, Hs, Ws), 2.0, device="cuda"))
            hot.remember(torch.linalg.inv(key @ _yaw(YAWS[s], SHIFTS[s])).float()[None].cuda(), K0, capacity=M)
        ring = hot._ring
        order = ring.slots_newest_first()
        maps = [nhwc.View(ring.feat[s], 0, ring.feat.shape[-1]) for s in order]  # what a caller would have had to keep by hand
        cams = [(ring.cam_T_world[s], ring.K[s]) for s in order]

        def single_keys(rendered, invK):
            """M single-key launches and the first-valid select: (pred, key, depth)."""
            outs = [mlp.view_logits(mnet, maps[m], rendered, invK, wTc, cams[m][0], cams[m][1], None, fill) for m in range(M)]
            pred, keyi, depth = torch.full_like(outs[0][0], fill), torch.full(outs[0][1].shape, NONE, dtype=torch.uint8, device="cuda"), outs[0][2]
            for m in reversed(range(M)):
                lg, valid, z, _ = outs[m]
                pred, depth = torch.where(valid, lg, pred), torch.where(valid, z, depth)
                keyi = torch.where(valid, torch.full_like(keyi, m), keyi)
            return pred, keyi, depth

        for name, (h, w) in (("192x256", (192, 256)), ("480x640", (480, 640))):
            Kv = syn.intrinsics(w, h).clone()
            Kv[0, 0], Kv[1, 1] = 0.5 * Kv[0, 0], 0.5 * Kv[1, 1]
            invK = torch.linalg.inv(Kv).float()[None].cuda()
            rendered = (1.0 + 3.0 * torch.rand((B, 1, h, w), generator=torch.Generator().manual_seed(3))).cuda()

            def fused_search():
                return hot.query_view_depths_keys(invK, wTc, size=(h, w), fill=fill)

            def composed_search():
                lo, hi = torch.full((B, 1, h, w), LO, device="cuda"), torch.full((B, 1, h, w), HI, device="cuda")
                sd = (hi - lo) * 0.5
                flags = torch.zeros(B, 1, h, w, dtype=torch.uint8, device="cuda")
                for _ in range(ITERS):
                    pred, keyi, _ = single_keys(sd, invK)
                    vis = pred < 0.0  # logit(0.5)
                    hi, lo = torch.where(vis, sd, hi), torch.where(vis, lo, sd)
                    flags |= (torch.where(vis, 1, 2) | torch.where(keyi != NONE, 0, 4)).to(torch.uint8)
                    sd = (hi + lo) * 0.5
                return sd, pred, flags, keyi

            shares = lambda k: {**{f"key{m}": (k == m).float().mean().item() for m in range(M)}, "none": (k == NONE).float().mean().item()}
            r = {"pixels": h * w, "keys": M}
            r.update(_measure({"fused_ms": lambda: hot.query_view_keys(rendered, invK, wTc, fill=fill),
                               "composition_ms": lambda: single_keys(rendered, invK)}, a.reps, a.iters))
            fo, (pred, keyi, depth) = hot.query_view_keys(rendered, invK, wTc, fill=fill), single_keys(rendered, invK)
            r["bitwise_equal_to_composition"] = bool(torch.equal(fo["view_pred"], pred) and torch.equal(fo["view_key"], keyi)
                                                     and torch.equal(fo["view_depth"], depth))
            r["pixel_shares"] = shares(fo["view_key"])
            res["dense_" + name] = r
            r = {"rays": h * w, "keys": M, "steps": ITERS}
            r.update(_measure({"fused_ms": fused_search, "composition_ms": composed_search}, a.reps, a.iters))
            fs, (sd, pred, flags, keyi) = fused_search(), composed_search()
            r["bitwise_equal_to_composition"] = bool(torch.equal(fs["view_search_depths"], sd) and torch.equal(fs["view_search_logits"], pred)
                                                     and torch.equal(fs["view_search_flags"], flags) and torch.equal(fs["view_search_key"], keyi))
            probes = torch.stack([hot.query_view_depths_keys(invK, wTc, size=(h, w), fill=fill, iters=n)["view_search_key"] for n in range(1, ITERS + 1)])
            r["probe_shares"] = shares(probes)
            r["bracketed_share"] = (fs["view_search_flags"] == 3).float().mean().item()
            r["some_probe_without_key_share"] = ((fs["view_search_flags"] & 4) != 0).float().mean().item()
            res["search_" + name] = r
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
