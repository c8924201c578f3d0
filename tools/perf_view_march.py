"""Times the first-hit march in a moving camera (view_march_k / view_keys_march_k, csrc/mlp_rays.hip) against what a caller had without it,
B = 1 at the full size: s0 map 192 x 256 (96 x 128 matching maps, D = 64, K = 7 dot-product volume, synthetic weights), the view camera
the keyframe's moved and turned (as tools/perf_view_depths.py), views 192 x 256 (49 152 rays), 480 x 640 (307 200) and a list of 64 rays;
and the M = 4 ring of tools/perf_view_keys.py at 192 x 256 and 480 x 640.  16 samples, linear on [0.5, 8], 8 refinement steps; every row
with fill = +10 (a probe outside the keyframe's view marches on) and fill = -10 (it is a hit).

"fused_ms": ``HotPath.query_view_first_hit`` (``_keys``) - one launch.  "composition_ms": the composition available before, timed in the
same run: n + R = 24 ``HotPath.query_view`` (``query_view_keys``) calls on the per-ray map rendered = q with the rule in torch between them,
rays that are done carried with their state frozen, no host synchronisation.  "bisection_ms": ``query_view_depths`` (``_keys``) at 12
steps, for scale - it answers another question (one crossing assumed).  A ray list has no depth map; the 64 rays are the pixel centres of
an 8 x 8 view, which both sides can express (the fused side takes them as a list).

HIP-event time over --iters back-to-back calls, divided by their number; --reps such windows per side, alternating, after one untimed
window of each; the median with the minimum and maximum beside it.  Host work of a call is inside the window.  Also reports whether both
sides give the same bits, the shares of bracketed / none / s* = 0 rays and the mean number of probes a 16-ray tile evaluates (the steps at
which one of its rays is not done; of 24).  Prints one JSON line; --out also writes it.

    python tools/perf_view_march.py --reps 7 --iters 10 --out profiles/view_march/run.json
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
from perf_view_keys import SHIFTS, YAWS, _yaw  # noqa: E402

N_MARCH, REFINE, LO, HI, BISECT = 16, 8, 0.5, 8.0, 12


def compose(query, q_s, shape, want_active=False):
    """N_MARCH + REFINE dense queries with the rule of include/idh.h in torch between them.  ``query(rendered)`` -> (logits with fill,
    valid, key | None).  Returns (depth, last logit, flags, hit_step, key, per-step active masks | None)."""
    n = q_s.numel()
    st = torch.full(shape, -1, dtype=torch.long, device="cuda")
    lo, hi, sd, logit = (torch.zeros(shape, device="cuda") for _ in range(4))
    flags = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    hit, key = (torch.full(shape, 255, dtype=torch.uint8, device="cuda") for _ in range(2))
    act = []
    for it in range(n + REFINE):
        a, marching = st != 0, st < 0
        q = torch.where(marching, q_s[min(it, n - 1)], sd)
        l, valid, k = query(q)
        behind = l < 0.0  # logit(0.5)
        nhi, nlo = torch.where(behind, q, hi), torch.where(behind, lo, q)
        nst = torch.where(marching, torch.where(behind, torch.full_like(st, REFINE if it > 0 else 0), torch.full_like(st, 0 if it == n - 1 else -1)), st - 1)
        nsd = torch.where((marching & behind & (it > 0)) | ~marching, (nhi + nlo) * 0.5, q)
        flags = torch.where(a, flags | (torch.where(behind, 1, 2) | torch.where(valid, 0, 4)).to(torch.uint8), flags)
        hit = torch.where(a & marching & behind, torch.full_like(hit, it), hit)
        logit = torch.where(a, l, logit)
        if k is not None:
            key = torch.where(a, k, key)
        hi, lo, sd, st = (torch.where(a, x, y) for x, y in ((nhi, hi), (nlo, lo), (nsd, sd), (nst, st)))
        if want_active:
            act.append(a)
    return sd, logit, flags, hit, key, act if want_active else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_view_march.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import mlp
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
    rel = torch.eye(4, dtype=torch.float64)
    c, s = math.cos(0.31), math.sin(0.31)
    rel[0, 0], rel[0, 2], rel[2, 0], rel[2, 2] = c, s, -s, c
    rel[:3, 3] = torch.tensor([0.35, -0.12, 0.2], dtype=torch.float64)
    wTc_moved = (key @ rel).float()[None].cuda()
    wTc_pan = (key @ _yaw(0.0, (0.02, -0.015, 0.01))).float()[None].cuda()
    cTw = torch.linalg.inv(key).float()[None].cuda()
    K0 = syn.intrinsics(Ws, Hs).float()[None].cuda()
    q_s = mlp.march_samples(N_MARCH, LO, HI).cuda()
    res = {}

    def row(name, h, w, fused, query, bisect):
        sh = (B, 1, h, w)
        r = {"rays": h * w, "n_march": N_MARCH, "refine": REFINE}
        r.update(_measure({"fused_ms": fused, "composition_ms": lambda: compose(query, q_s, sh), "bisection_ms": bisect}, a.reps, a.iters))
        fo = fused()
        sd, logit, flags, hit, keyi, act = compose(query, q_s, sh, want_active=True)
        same = all(torch.equal(fo[k].reshape(-1), v.reshape(-1)) for k, v in (("view_march_depths", sd), ("view_march_logits", logit),
                                                                               ("view_march_flags", flags), ("view_march_hit_step", hit)))
        if "view_march_key" in fo:
            same = same and torch.equal(fo["view_march_key"].reshape(-1), keyi.reshape(-1))
        r["bitwise_equal_to_composition"] = bool(same)
        fl, hs = fo["view_march_flags"], fo["view_march_hit_step"]
        r["bracketed_share"] = ((fl & 3) == 3).float().mean().item()
        r["none_share"] = (hs == 255).float().mean().item()
        r["first_sample_share"] = (hs == 0).float().mean().item()
        r["some_probe_invalid_share"] = ((fl & 4) != 0).float().mean().item()
        pad = (-h * w) % 16
        tiles = torch.nn.functional.pad(torch.stack(act).view(len(act), -1), (0, pad)).view(len(act), -1, 16).any(-1)
        r["mean_probes_per_tile"] = tiles.float().sum(0).mean().item()
        r["mean_probes_per_ray"] = torch.stack(act).float().sum(0).mean().item()
        res[name] = r

    def forward(seed):
        d = {k: v.cuda() for k, v in syn.cost_volume_inputs(B, K, 16, H, W, seed=seed, behind_view=K - 1).items()}
        pyr = [t.cuda() for t in syn.encoder_pyramid(B, H * 4, W * 4, seed=seed)]
        hot(d["cur_feats"], d["src_feats"], pyr, d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"],
            rendered_depth=torch.full((B, 1, Hs, Ws), 2.0, device="cuda"))

    with torch.inference_mode():
        forward(0)  # fills the decoder's scale-0 map; every timed call below reads it and runs no conv
        for fill in (10.0, -10.0):
            tag = "fill+10" if fill > 0 else "fill-10"
            for name, (h, w), listed in (("192x256", (192, 256), False), ("480x640", (480, 640), False), ("list64", (8, 8), True)):
                invK = torch.linalg.inv(syn.intrinsics(w, h)).float()[None].cuda()
                yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5, indexing="ij")
                rays = torch.stack([xx, yy], -1).view(1, h * w, 2).cuda()
                kw = dict(rays=rays) if listed else dict(size=(h, w))

                def query(q):
                    v = hot.query_view(q, invK, wTc_moved, cTw, K0, fill=fill)
                    return v["view_pred"], v["view_valid"], None

                row(f"{name}_{tag}", h, w,
                    lambda: hot.query_view_first_hit(invK, wTc_moved, cTw, K0, fill=fill, samples=N_MARCH, lo=LO, hi=HI, refine=REFINE, **kw),
                    query, lambda: hot.query_view_depths(invK, wTc_moved, cTw, K0, fill=fill, iters=BISECT, **kw))
        for sidx in range(M):  # the ring of tools/perf_view_keys.py: M forwards, each remembered with its own camera
            forward(sidx)
            hot.remember(torch.linalg.inv(key @ _yaw(YAWS[sidx], SHIFTS[sidx])).float()[None].cuda(), K0, capacity=M)
        for fill in (10.0, -10.0):
            tag = "fill+10" if fill > 0 else "fill-10"
            for name, (h, w) in (("192x256", (192, 256)), ("480x640", (480, 640))):
                Kv = syn.intrinsics(w, h).clone()
                Kv[0, 0], Kv[1, 1] = 0.5 * Kv[0, 0], 0.5 * Kv[1, 1]
                invK = torch.linalg.inv(Kv).float()[None].cuda()

                def query_keys(q):
                    v = hot.query_view_keys(q, invK, wTc_pan, fill=fill)
                    return v["view_pred"], v["view_valid"], v["view_key"]

                row(f"keys{M}_{name}_{tag}", h, w,
                    lambda: hot.query_view_first_hit_keys(invK, wTc_pan, size=(h, w), fill=fill, samples=N_MARCH, lo=LO, hi=HI, refine=REFINE),
                    query_keys, lambda: hot.query_view_depths_keys(invK, wTc_pan, size=(h, w), fill=fill, iters=BISECT))
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
