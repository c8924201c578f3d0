"""Times the TSDF colour calls beside their counterparts without colour, on tools/perf_tsdf.py's scene: the 96 x 256 x 256
grid of 4 cm voxels, maps of 192 x 256, camera frames of 384 x 512.

  integrate   "integrate_color_ms" (idh_tsdf_integrate_color_fwd, one map and its frame) beside "integrate_ms" (idh_tsdf_integrate_fwd, the
              same map) on volumes of their own; "touched_voxels" and "coloured_voxels" of one map on an empty volume.
  raycast     "raycast_color_ms" beside "raycast_ms" at 192 x 256 (plain march, near 0.25, far 6.0, 144 samples), with and without
              normals, on the volume four maps fused.
  mesh        "mesh_colors_ms" (idh_tsdf_mesh_colors_fwd) beside "mesh_emit_ms" (idh_tsdf_mesh_emit_fwd) into preallocated outputs after
              one count call on that volume.

Windows, alternation and statistics are perf_tsdf.py's.  Prints one JSON line; --out also writes it.

    python tools/perf_tsdf_color.py --reps 7 --iters 20 --out profiles/tsdf/color.json
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

import perf_tsdf as P  # noqa: E402
from perf_ray_queries import _measure  # noqa: E402

hc, wc = 384, 512


def frame(seed):
    r = np.random.default_rng(100 + seed)
    ii, jj = np.meshgrid(np.arange(hc), np.arange(wc), indexing="ij")
    c = np.stack([128 + 90 * np.sin(0.011 * jj + seed), 120 + 80 * np.cos(0.013 * ii), 100 + 0.2 * jj], -1) + r.integers(-3, 4, (hc, wc, 3))
    return np.clip(c, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_tsdf_color.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import fusion

    dev = torch.device("cuda:0")
    DIMS, VOXEL, h, w = P.DIMS, P.VOXEL, P.h, P.w
    centre = np.array([0.3, -0.2, 1.4])
    origin = tuple(centre - VOXEL * 0.5 * (np.array([DIMS[2], DIMS[1], DIMS[0]]) - 1.0))
    world_T_src = [P._pose(0.03 * m, centre + np.array([0.02 * m, 0.04 * m, 0.0])) for m in range(4)]
    depth_all = torch.from_numpy(np.stack([P.source_depth(m) for m in range(4)]))[:, None].to(dev)
    frames_all = torch.from_numpy(np.stack([frame(m) for m in range(4)])).to(dev)
    K_src, K_frame = syn.intrinsics(w, h).float().to(dev), syn.intrinsics(wc, hc).float().to(dev)
    cam_T_world = torch.from_numpy(np.stack([np.linalg.inv(T) for T in world_T_src]).astype(np.float32)).to(dev)
    res = {}
    with torch.inference_mode():
        def inputs(M):
            return (depth_all[:M].contiguous(), K_src[None].expand(M, 4, 4).contiguous(), cam_T_world[:M].contiguous(), frames_all[:M].contiguous(),
                    K_frame[None].expand(M, 4, 4).contiguous())

        d, K, E, f, Kf = inputs(1)
        plain, col = fusion.TSDFVolume(DIMS, VOXEL, origin), fusion.TSDFVolume(DIMS, VOXEL, origin, color=True)
        col.integrate(d, K, E, f, Kf)
        touched, coloured = int((col.values[..., 1] > 0).sum()), int((col.colors[..., 3] > 0).sum())
        n = DIMS[0] * DIMS[1] * DIMS[2]
        r = {"voxels": n, "touched_voxels": touched, "coloured_voxels": coloured, "coloured_share": coloured / n, "frame": [hc, wc], "map": [h, w]}
        r.update(_measure({"integrate_ms": lambda: plain.integrate(d, K, E), "integrate_color_ms": lambda: col.integrate(d, K, E, f, Kf)}, a.reps, a.iters))
        res["integrate_M1"] = r
        # ---- the volume four maps fused
        vol = fusion.TSDFVolume(DIMS, VOXEL, origin, color=True)
        vol.integrate(*inputs(4))
        T = torch.from_numpy(P._pose(0.2, centre + np.array([0.05, 0.25, -0.03])).astype(np.float32)).to(dev)
        H, W = 192, 256
        invK = torch.linalg.inv(syn.intrinsics(W, H).float().to(dev))
        kw = dict(near=P.NEAR, far=P.FAR)
        sides = {"raycast_ms": lambda: vol.raycast(T, invK, (H, W), **kw), "raycast_color_ms": lambda: vol.raycast(T, invK, (H, W), return_color=True, **kw),
                 "raycast_normals_ms": lambda: vol.raycast(T, invK, (H, W), return_normals=True, **kw),
                 "raycast_normals_color_ms": lambda: vol.raycast(T, invK, (H, W), return_normals=True, return_color=True, **kw)}
        r = {"target": [H, W]}
        r.update(_measure(sides, a.reps, a.iters))
        out = sides["raycast_color_ms"]()
        r["hit_share"] = ((out["flags"] & 1) > 0).float().mean().item()
        r["alpha_share"] = (out["rgba"][..., 3] == 255).float().mean().item()
        res["raycast_192x256"] = r
        # ---- mesh
        workspace, totals = fusion.mesh_count(vol)
        V, F = totals.tolist()
        verts, faces = torch.empty(V, 3, device=dev), torch.empty(F, 3, device=dev, dtype=torch.int32)
        rgba = torch.empty(V, 4, device=dev, dtype=torch.uint8)
        r = {"verts": V, "faces": F}
        r.update(_measure({"mesh_emit_ms": lambda: fusion.mesh_emit(vol, workspace, verts, faces), "mesh_colors_ms": lambda: fusion.mesh_colors(vol, workspace, rgba)},
                          a.reps, a.iters))
        r["with_colour_share"] = (rgba[:, 3] == 255).float().mean().item()
        res["mesh"] = r
    res["device"] = torch.cuda.get_device_name(0)
    res["reps"], res["iters"] = a.reps, a.iters
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
