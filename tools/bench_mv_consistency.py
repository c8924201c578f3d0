"""Times the multi-view depth consistency check (csrc/mv_consistency.hip, geometry.depth_consistency) at 192 x 256 with K = 7 sources:
B = 1 - what ``StreamingSession.remember_depth`` launches per remembered map - and B = 32.

  "kernel_us"      ``idh_mv_consistency_fwd`` through ctypes with every buffer allocated before the window: counts, weight and filtered
                   depth out, no per-source planes, no loss (the session's call); "kernel_loss_us" with the loss and its second launch.
  "torch_us"       the same computation composed from torch fp32 ops on the GPU (tests/mv_consistency_ref.py's statement moved to the
                   device: matmuls, a gather for the nearest tap, comparisons, sums over the sources): the baseline, not the code under test.
  "bytes"          what the call must move: the tested map and the K source maps read once, counts (3 B), weight and filtered depth
                   (4 B each) written per pixel; "hbm_fraction" = bytes / kernel time / 8 TB/s, the MI355X's HBM3E peak.
  "remember_depth_us"  ``StreamingSession.remember_depth`` with fusion into a 96 x 256 x 256 volume, with and without the check, on a
                   ring of 7 maps (--session; needs the session's model, so it builds one from synthetic weights).

HIP-event time over --iters back-to-back calls divided by their number; --reps such windows per side, alternating, after one untimed
window of each; the median with minimum and maximum.  Prints one JSON line; --out also writes it.

    python tools/bench_mv_consistency.py --reps 9 --iters 50 --out profiles/mv_consistency/run.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from perf_ray_queries import _measure  # noqa: E402

h, w, K = 192, 256, 7
HBM_BYTES_PER_S = 8.0e12


def scene(B):
    """A wall 2 m away seen by B cameras and K sources each, with noise: most pixels are visible in most sources."""
    import mv_consistency_ref as R

    r = np.random.default_rng(0)
    out = {k: [] for k in ("depth", "invK", "world_T_cam", "src_depth", "src_K", "src_cam_T_world")}
    for _ in range(B):
        Kc, T = R._camera(r, h, w, 0.4)
        sd, sK, sE = [], [], []
        for _ in range(K):
            Ks, Ts = R._camera(r, h, w, 0.6)
            sd.append(R._wall_depth(h, w, Ks, Ts) * (1 + 0.01 * r.standard_normal((h, w))))
            sK.append(Ks), sE.append(np.linalg.inv(Ts))
        for k_, v_ in zip(out, (R._wall_depth(h, w, Kc, T)[None] * (1 + 0.02 * r.standard_normal((1, h, w))), np.linalg.inv(Kc), T,
                                np.stack(sd)[:, None], np.stack(sK), np.stack(sE))):
            out[k_].append(v_)
    return {k_: torch.from_numpy(np.stack(v_).astype(np.float32)).cuda() for k_, v_ in out.items()}


def torch_check(s, ratio=1.05, log_tol=0.05, min_consistent=1, max_conflict=0):
    d, B = s["depth"], s["depth"].shape[0]
    ii, jj = torch.meshgrid(torch.arange(h, device=d.device), torch.arange(w, device=d.device), indexing="ij")
    pix = torch.stack([jj + 0.5, ii + 0.5, torch.ones_like(ii)], 0).float().reshape(1, 3, -1)
    cam = d.reshape(B, 1, -1) * (s["invK"][:, :3, :3] @ pix)
    X = s["world_T_cam"] @ torch.cat([cam, torch.ones_like(cam[:, :1])], 1)
    c = (s["src_K"] @ s["src_cam_T_world"])[:, :, :3] @ X[:, None]
    z = c[:, :, 2].clamp_min(1e-5)
    xr, yr = torch.round(c[:, :, 0] / z - 0.5), torch.round(c[:, :, 1] / z - 0.5)
    inside = (xr >= 0) & (xr <= w - 1) & (yr >= 0) & (yr <= h - 1)
    idx = (yr.clamp(0, h - 1) * w + xr.clamp(0, w - 1)).long()
    samp = torch.where(inside, s["src_depth"].reshape(B, K, -1).gather(2, idx), torch.zeros_like(z))
    vis = (z < ratio * samp) & (z > 0) & (samp > 0)
    l = torch.log(samp) - torch.log(z)
    ok = vis & torch.isfinite(samp) & ((d > 0) & torch.isfinite(d)).reshape(B, 1, -1)
    n_con, n_conf = (ok & (l.abs() <= log_tol)).sum(1), (ok & (l > log_tol)).sum(1)
    kept = ((d > 0) & torch.isfinite(d)).reshape(B, -1) & (n_con >= min_consistent) & (n_conf <= max_conflict)
    counts = torch.stack([vis.sum(1), n_con, n_conf], 1).to(torch.uint8)
    return counts, torch.where(kept, 1.0 + n_con, torch.zeros_like(kept, dtype=torch.float32)), torch.where(kept, d.reshape(B, -1), torch.zeros_like(d.reshape(B, -1)))


def kernel_call(s, loss):
    from implicit_depth_amd import _lib

    B, dev = s["depth"].shape[0], s["depth"].device
    out = dict(counts=torch.empty(B, 3, h, w, dtype=torch.uint8, device=dev), weight=torch.empty(B, 1, h, w, device=dev), filtered=torch.empty(B, 1, h, w, device=dev))
    a = _lib.MvConsistencyArgs()
    a.depth_b1hw, a.invK_b44, a.world_T_cam_b44 = s["depth"].data_ptr(), s["invK"].data_ptr(), s["world_T_cam"].data_ptr()
    a.src_depth_bk1hw, a.src_K_bk44, a.src_cam_T_world_bk44 = s["src_depth"].data_ptr(), s["src_K"].data_ptr(), s["src_cam_T_world"].data_ptr()
    a.counts_b3hw, a.weight_b1hw, a.filtered_depth_b1hw = out["counts"].data_ptr(), out["weight"].data_ptr(), out["filtered"].data_ptr()
    a.ratio, a.log_tol, a.min_consistent, a.max_conflict = 1.05, 0.05, 1, 0
    a.B, a.K, a.h, a.w, a.src_h, a.src_w = B, K, h, w, h, w
    if loss:
        n = _lib.lib().idh_mv_consistency_workspace_bytes(B, K, h, w)
        out["ws"], out["loss"] = torch.empty(n // 8, dtype=torch.float64, device=dev), torch.empty((), device=dev)
        a.workspace, a.workspace_bytes, a.loss = out["ws"].data_ptr(), n, out["loss"].data_ptr()
    fn, st = _lib.lib().idh_mv_consistency_fwd, _lib.stream_ptr()

    def call():
        rc = fn(a, st)
        assert rc == 0, rc

    return call, out


def session_times(reps, iters):
    import implicit_depth_amd.synthetic as syn  # noqa: F401
    import mv_consistency_ref as R
    from implicit_depth_amd.streaming import StreamingSession
    from test_warp_session_gpu import _depth_model

    r = np.random.default_rng(1)
    cams = [R._camera(r, h, w, 0.4) for _ in range(8)]
    maps = [(torch.from_numpy((R._wall_depth(h, w, Kc, T) * (1 + 0.01 * r.standard_normal((h, w)))).astype(np.float32))[None, None].cuda(), T,
             torch.from_numpy(np.linalg.inv(Kc).astype(np.float32))[None].cuda()) for Kc, T in cams]
    sides = {}
    for name, kw in (("plain", {}), ("checked", dict(consistency={})), ("weighted", dict(consistency={}, weighted=True))):
        s = StreamingSession(_depth_model("dot", 2), num_source_views=2, buffer_size=4, query_keyframes=7)
        s.start_fusion(voxel_size=0.04, dims=(96, 256, 256), origin=(-5.0, -5.0, -1.0), **kw)
        for m in maps[:7]:
            s.remember_depth(*m)
        sides[name] = lambda s=s: s.remember_depth(*maps[7])  # the ring stays at 7 maps: every call checks against 7 sources
    return _measure(sides, reps, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--session", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mv_consistency.py measures on the GPU; none is visible")
    res = {"h": h, "w": w, "K": K, "cases": {}}
    for B in (1, 32):
        s = scene(B)
        plain, out = kernel_call(s, False)
        with_loss, _ = kernel_call(s, True)
        plain()
        ref = torch_check(s)
        same = float((out["counts"].reshape(ref[0].shape) == ref[0]).float().mean())
        t = _measure({"kernel": plain, "kernel_loss": with_loss, "torch": lambda: torch_check(s)}, a.reps, a.iters)
        nbytes = B * h * w * (4 + 4 * K + 3 + 4 + 4)
        res["cases"][f"B{B}"] = {"kernel_us": {k: round(v * 1e3, 2) for k, v in t["kernel"].items()},
                                 "kernel_loss_us": {k: round(v * 1e3, 2) for k, v in t["kernel_loss"].items()},
                                 "torch_us": {k: round(v * 1e3, 2) for k, v in t["torch"].items()}, "bytes": nbytes,
                                 "hbm_fraction": round(nbytes / (t["kernel"]["median"] * 1e-3) / HBM_BYTES_PER_S, 4),
                                 "counts_equal_torch_fraction": round(same, 5), "visible_mean": round(float(out["counts"][:, 0].float().mean()), 2)}
    if a.session:
        res["remember_depth_us"] = {k: {q: round(x * 1e3, 1) for q, x in v.items()} for k, v in session_times(a.reps, max(a.iters // 5, 4)).items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
