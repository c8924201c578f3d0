"""Times the sparse occlusion queries (csrc/mlp_rays.hip) against what a caller had without them, B = 1 at the full size: s0 map 192 x 256
(96 x 128 matching maps, D = 64, K = 7 dot-product volume, synthetic weights).  One forward fills the decoder's four output maps; every
timed call below reads them and runs no conv.

(a) "train_shape": the reference's training shape, N = 4096 rays x S = 64 depth samples at all four scales (run_mlp_train,
    bd_model.py:313-393).  "fused_ms": ``HotPath.query_rays(scales=(0,1,2,3))``, four launches.  "composition_ms": the path without the
    new entry points, timed in the same run: export the four maps to NCHW (what ``return_features=True`` does), ``F.grid_sample`` per scale,
    expand + concat to (1, Nq, S, 1 + C) rows, ``mlp.binary_mlp_forward``.  Its parts are also timed alone ("export_ms",
    "sample_concat_ms", "mlp_ms").
(b) "points": N = 1024 world points, S = 1, ``HotPath.query_points`` (projection + one launch) against one dense plane of
    ``mlp.occlusion_logits`` (49 152 pixels), which is what answering "a few points" cost before.

HIP-event time over --iters back-to-back calls, divided by their number; --reps such windows per side, alternating, after one untimed
window of each; the median with the minimum and maximum beside it.  Host work of a call (ctypes, launches, torch allocations) is inside the
window.  Also reports the scale-relative difference of both sides' logits.  Prints one JSON line; --out also writes it.

    python tools/perf_ray_queries.py --reps 7 --iters 20 --out profiles/ray_queries/run.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_ray_queries.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import mlp
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from implicit_depth_amd.pipeline import HotPath, _export

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
    grid = (Hs, Ws)
    rays = (torch.rand((B, a.rays, 2), generator=g) * torch.tensor([float(Ws), float(Hs)])).cuda()
    depths = (0.5 + 5 * torch.rand((B, a.rays, a.samples), generator=g)).cuda()
    with torch.inference_mode():
        hot(d["cur_feats"], d["src_feats"], pyr, d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"], query_rays=rays[:, :16],
            query_depths=depths[:, :16], query_scales=(0, 1, 2, 3))
        final = hot._last["final"]

        def fused():
            return hot.query_rays(rays, depths, grid=grid, scales=(0, 1, 2, 3))

        def export():
            return [_export(final[s]) for s in range(4)]

        def rows_of(feats):
            rows = []
            for s in range(4):
                r = rays[:, ::s + 1]
                gn = torch.stack([(r[..., 0] / Ws - 0.5) * 2, (r[..., 1] / Hs - 0.5) * 2], -1).unsqueeze(2)
                f = F.grid_sample(feats[s], gn, mode="bilinear", align_corners=False).expand(-1, -1, -1, a.samples)
                rows.append(torch.cat((depths[:, ::s + 1].unsqueeze(1), f), 1).permute(0, 2, 3, 1))
            return rows

        def composition():
            return mlp.binary_mlp_forward(mnet, rows_of(export()))

        feats = export()
        rows = rows_of(feats)
        res = {"train_shape": {"rays": a.rays, "samples": a.samples, "scales": 4}}
        res["train_shape"].update(_measure({"fused_ms": fused, "composition_ms": composition}, a.reps, a.iters))
        res["train_shape"].update(_measure({"export_ms": export, "sample_concat_ms": lambda: rows_of(feats),
                                            "mlp_ms": lambda: mlp.binary_mlp_forward(mnet, rows)}, a.reps, a.iters))
        fo, co = fused(), composition()
        res["train_shape"]["scale_rel_diff"] = max(
            ((fo[f"ray_pred_{s}"][:, 0] - co[f"pred_{s}"][..., 0]).abs().max() / co[f"pred_{s}"].abs().max()).item() for s in range(4))

        K0 = syn.intrinsics(Ws, Hs).float()[None].cuda()
        wTc = syn.source_pose(1).float()
        cTw = torch.linalg.inv(wTc)[None].cuda()
        uvz = torch.rand((B, a.points, 3), generator=g) * torch.tensor([float(Ws), float(Hs), 4.0]) + torch.tensor([0.0, 0.0, 0.6])
        Kc = K0[0].cpu()
        cam = torch.stack([(uvz[..., 0] - Kc[0, 2]) / Kc[0, 0] * uvz[..., 2], (uvz[..., 1] - Kc[1, 2]) / Kc[1, 1] * uvz[..., 2], uvz[..., 2]], -1)
        pts = (cam @ wTc[:3, :3].t() + wTc[:3, 3]).cuda()
        plane = torch.full((B, 1, Hs, Ws), 2.0, device="cuda")
        f0 = final[0]
        res["points"] = {"points": a.points, "dense_pixels": Hs * Ws}
        res["points"].update(_measure({"query_points_ms": lambda: hot.query_points(pts, cTw, K0),
                                       "dense_plane_ms": lambda: mlp.occlusion_logits(mnet, f0.buf, f0.c0, f0.C, plane)}, a.reps, a.iters))
        q = hot.query_points(pts, cTw, K0)
        res["points"]["valid_share"] = q["point_valid"].float().mean().item()
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
