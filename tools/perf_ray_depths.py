"""Times the ray depth search (ray_search_k, csrc/mlp_rays.hip) against what a caller had without it, B = 1 at the full size: s0 map
192 x 256 (96 x 128 matching maps, D = 64, K = 7 dot-product volume, synthetic weights), 12 iterations, constant threshold 0.5.  One
forward fills the decoder's scale-0 map; every timed call below reads it and runs no conv.  Per N in --rays:

"fused_ms":        ``HotPath.query_ray_depths(rays, invK_s0_b44, world_T_cam_b44)``: one launch, depth + flags + world points.
"fused_depth_ms":  the same without the hit points (no invK): what the two alternatives below deliver.
"composition_ms":  twelve ``HotPath.query_rays(S = 1)`` calls with the bound updates in torch between them (the rule of bd_model.py:273-292).
"dense_ms":        ``mlp.infer_depth`` over all 49 152 pixels of the map (independent of N; its rays are the pixel centres).

HIP-event time over --iters back-to-back calls, divided by their number; --reps such windows per side, alternating, after one untimed
window of each; the median with the minimum and maximum beside it.  Host work of a call (ctypes, launches, torch allocations) is inside the
window.  Also checks that the fused depths equal the composition's bit for bit.  Prints one JSON line; --out also writes it.

    python tools/perf_ray_depths.py --reps 7 --iters 20 --out profiles/ray_depths/run.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def _measure(sides, reps, iters):
    for fn in sides.values():
        _window(fn, 2)
    t = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            t[k].append(_window(fn, iters))
    return {k: _stats(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rays", type=int, nargs="+", default=[64, 1024, 4096, 49152])
    ap.add_argument("--search-iters", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_ray_depths.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import mlp
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
    g = torch.Generator().manual_seed(1)
    iK = torch.linalg.inv(syn.intrinsics(Ws, Hs)).float()[None].cuda()
    wTc = syn.source_pose(1).float()[None].cuda()
    n_it = a.search_iters
    res = {"map": [Hs, Ws], "search_iters": n_it, "cases": []}
    with torch.inference_mode():
        hot(d["cur_feats"], d["src_feats"], pyr, d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"])
        f0 = hot._last["final"][0]

        def dense():
            return mlp.infer_depth(mnet, f0.buf, f0.c0, f0.C, iters=n_it)

        for N in a.rays:
            rays = (torch.rand((B, N, 2), generator=g) * torch.tensor([float(Ws), float(Hs)])).cuda()

            def fused():
                return hot.query_ray_depths(rays, invK_s0_b44=iK, world_T_cam_b44=wTc, iters=n_it)

            def fused_depth():
                return hot.query_ray_depths(rays, iters=n_it)

            def composition():
                lo, hi = torch.full((B, N), 0.5, device="cuda"), torch.full((B, N), 8.0, device="cuda")
                sd = (hi - lo) * 0.5
                for _ in range(n_it):
                    logit = hot.query_rays(rays, sd.unsqueeze(-1))["ray_pred_0"][:, 0, :, 0]
                    vis = logit < 0  # logit(0.5)
                    hi, lo = torch.where(vis, sd, hi), torch.where(vis, lo, sd)
                    sd = (hi + lo) * 0.5
                return sd

            row = {"rays": N}
            row.update(_measure({"fused_ms": fused, "fused_depth_ms": fused_depth, "composition_ms": composition, "dense_ms": dense}, a.reps, a.iters))
            q = fused()
            row["bitwise_equal_to_composition"] = bool(torch.equal(q["ray_depth"], composition()))
            row["bracketed_share"] = round((q["ray_hit"] == 3).float().mean().item(), 4)
            res["cases"].append(row)
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
