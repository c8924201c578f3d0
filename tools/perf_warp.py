"""Times the depth warp (csrc/depth_warp.hip, raster.warp_depth) at the full size: M = 1 and M = 4 source depth maps of 192 x 256 (a
smooth room about 2.5 m away with a box 1.2 m away in front of it and a few dead taps; the sources' cameras a few centimetres and
hundredths of a radian apart) into one live camera moved 0.25 m and turned 0.2 rad, at 192 x 256 and at 384 x 512.

  "fused_ms"                      ``raster.warp_depth``: fill, face pass (three depth taps and three vertex transforms per face), queued
                                  pass, resolve.  (A second form, with the vertices stored by a vertex pass, was measured with this
                                  script before it was removed: profiles/warp/forms.json.)
  "composition_ms"              the same result from what the library offered before: vertices (back-projection, cam_T_src) and the
                                  torn face list built with torch ops - the pixel grid and the full face list are built once, outside the
                                  timed region - then ``raster.render_depth`` of the M meshes as one.
  "depth_for_view_ms"             beside them, what a BDModel session answers the same question with: ``HotPath.query_view_depths`` at
                                  the same target size (twelve MLP passes per live pixel; the model of tools/perf_view_depths.py).

"bytes" is what the warp must move, from shapes: the depth maps once per face corner (cached: 4 B per source pixel from
memory), the key plane written, read by the atomics' hits and read once more by the resolve pass, the outputs.  HIP-event time over
--iters back-to-back calls, divided by their number; --reps such windows per side, alternating, after one untimed window of each; the
median with the minimum and maximum beside it.  Host work of a call (ctypes, launches, torch allocations) is inside the window.  Also
reports how far the composition's depth is from the fused one (its vertices are rounded differently: torch contracts to FMAs).
Prints one JSON line; --out also writes it.

    python tools/perf_warp.py --reps 7 --iters 20 --out profiles/warp/run.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from perf_ray_queries import _measure  # noqa: E402

h, w = 192, 256


def _pose(ry, t):
    T = np.eye(4)
    c, s = math.cos(ry), math.sin(ry)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = c, s, -s, c
    T[:3, 3] = t
    return T


def source_depth(seed):
    r = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d = 2.5 + 0.3 * np.sin(0.021 * jj + seed) * np.cos(0.017 * ii) + 0.002 * r.standard_normal((h, w))
    d[60:130, 80 + 5 * seed:170 + 5 * seed] = 1.2 + 0.001 * (jj[60:130, 80:170] - 80)
    d[r.integers(0, h, 40), r.integers(0, w, 40)] = 0.0
    return d.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_warp.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import networks as net
    from implicit_depth_amd import raster
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from implicit_depth_amd.pipeline import HotPath

    dev = torch.device("cuda:0")
    # the BDModel whose depth_for_view is timed beside the warp (tools/perf_view_depths.py's)
    B, Kv, Hm, Wm, D = 1, 7, 96, 128, 64
    cve = net.CVEncoder(D, [48, 64, 160, 256], [64, 128, 256, 384])
    dec = net.BDDecoderPP([24] + cve.num_ch_enc)
    mnet = net.BinaryMLPNetwork(dec.num_ch_dec)
    for i, m in enumerate([cve, dec, mnet]):
        syn.fill_state_dict(m, seed=50 + i, gain=1.1 if i == 2 else 1.0)
    hot = HotPath(CostVolumeManager(Hm, Wm, D), cve, dec, mnet).cuda()
    d = {k: v.cuda() for k, v in syn.cost_volume_inputs(B, Kv, 16, Hm, Wm, seed=0, behind_view=Kv - 1).items()}
    pyr = [t.cuda() for t in syn.encoder_pyramid(B, Hm * 4, Wm * 4, seed=0)]
    K0 = syn.intrinsics(w, h).float()[None].to(dev)

    world_T_src = [_pose(0.03 * m, (0.04 * m, 0.0, 0.02 * m)) for m in range(4)]
    world_T_live = _pose(0.2, (0.25, -0.03, 0.05))
    depth_all = torch.from_numpy(np.stack([source_depth(m) for m in range(4)]))[:, None].to(dev)
    invK_src = torch.linalg.inv(syn.intrinsics(w, h)).float().to(dev)
    # what the composition may keep between calls: the pixel grid and the untorn face list
    ii, jj = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    pix = torch.stack([jj + 0.5, ii + 0.5, torch.ones_like(ii)], 0).float().reshape(3, -1)
    v00 = (ii[:-1, :-1] * w + jj[:-1, :-1]).reshape(-1)
    base_faces = torch.stack([torch.stack([v00, v00 + w, v00 + 1], -1), torch.stack([v00 + 1, v00 + w, v00 + w + 1], -1)], 1).reshape(-1, 3)
    eye = torch.eye(4, device=dev)[None]
    res = {}
    with torch.inference_mode():
        hot(d["cur_feats"], d["src_feats"], pyr, d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"],
            rendered_depth=torch.full((B, 1, h, w), 2.0, device=dev))
        wTc = torch.from_numpy(world_T_live).float()[None].to(dev)
        cTw = torch.from_numpy(np.linalg.inv(world_T_src[0])).float()[None].to(dev)
        for M in (1, 4):
            depth, invK = depth_all[:M].contiguous(), invK_src[None].expand(M, 4, 4).contiguous()
            T = raster.relative_poses([world_T_live], world_T_src[:M]).to(dev)
            for H, W in ((192, 256), (384, 512)):
                K = syn.intrinsics(W, H).float()[None].to(dev)
                invK_live = torch.linalg.inv(K)

                def composition():
                    verts, faces = [], []
                    for m in range(M):
                        dm = depth[m].reshape(-1)
                        src = (invK[m, :3, :3] @ pix) * dm
                        verts.append((T[0, m, :3, :3] @ src + T[0, m, :3, 3:]).T)
                        fd = dm[base_faces]
                        ok = (torch.isfinite(fd) & (fd > 0)).all(1) & (fd.amax(1) <= fd.amin(1) * 1.1)
                        faces.append(base_faces[ok] + m * h * w)
                    return raster.render_depth(torch.cat(verts).contiguous(), torch.cat(faces).to(torch.int32), eye, K, H, W)

                sides = {"fused_ms": lambda: raster.warp_depth(depth, invK, T, K, H, W),
                         "composition_ms": composition,
                         "depth_for_view_ms": lambda: hot.query_view_depths(invK_live, wTc, cTw, K0, size=(H, W), fill=0.0)}
                r = {"sources": M, "target": [H, W], "faces": int(M * base_faces.shape[0]),
                     "bytes": M * h * w * 4 + H * W * (8 + 8 + 4)}
                r.update(_measure(sides, a.reps, a.iters))
                f, c = sides["fused_ms"]()["depth"], composition()
                both = (f > 0) & (c > 0)
                r["covered_share"] = (f > 0).float().mean().item()
                r["coverage_differs_from_composition_share"] = ((f > 0) != (c > 0)).float().mean().item()
                r["max_rel_diff_from_composition"] = ((f - c).abs() / c)[both].max().item()
                res[f"M{M}_{H}x{W}"] = r
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
