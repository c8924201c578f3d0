"""Times the TSDF fusion (csrc/tsdf.hip, fusion.TSDFVolume) at the full size: a 96 x 256 x 256 grid of 4 cm voxels (3.84 m high, 10.24 m
square, z up) around a camera that looks horizontally at a smooth wall about 2.5 m away with a box 1.2 m away in front of it.

  integrate   "integrate_ms" for M = 1 and M = 4 maps of 192 x 256 in one call, beside "copy_ms": ``Tensor.copy_`` of as many bytes as
              the call must move - 8 B read and 8 B written per voxel some map touches ("touched_voxels", counted on an empty volume)
              plus the maps - so copy_ms is the time a memory-bound kernel with perfect access would take.
  raycast     "raycast_skip_ms" / "raycast_plain_ms": ``TSDFVolume.raycast`` (near 0.25, far 6.0, one voxel per step: 144 samples)
              into a live camera moved 0.25 m and turned 0.2 rad, at 192 x 256 and 384 x 512, on the volume the four maps fused;
              "skip_equals_plain" says the two returned the same bits.  A second scene, "sparse", holds one map only and a live camera
              turned 1.2 rad, so most rays cross unobserved space: where jumping can pay.
  "torch_raycast_ms"  the same march composed from torch ops: per step ``grid_sample`` (trilinear) of T, ``grid_sample`` (nearest, at
              the sample's cell) of the known-cell grid, and the hit bookkeeping with ``torch.where``; the channel-first T volume and
              the known-cell grid are prepared outside the timed window.  For scale.
  "warp_ms"   ``raster.warp_depth`` of the same four maps into the same camera: for scale only, it answers a different question.

HIP-event time over --iters back-to-back calls divided by their number; --reps such windows per side, alternating, after one untimed
window of each; the median with minimum and maximum.  Host work of a call (ctypes, the launch, torch's allocation of the outputs) is
inside the window; the volume, the maps and the poses are on the device before it.  Prints one JSON line; --out also writes it.

    python tools/perf_tsdf.py --reps 7 --iters 20 --out profiles/tsdf/run.json
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
DIMS, VOXEL = (96, 256, 256), 0.04
NEAR, FAR = 0.25, 6.0
# camera axes in a z-up world: right = -y, down = -z, forward = +x
LEVEL = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


def _pose(yaw, t):
    c, s = math.cos(yaw), math.sin(yaw)
    T = np.eye(4)
    T[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ LEVEL
    T[:3, 3] = t
    return T


def source_depth(seed):
    r = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d = 2.5 + 0.3 * np.sin(0.021 * jj + seed) * np.cos(0.017 * ii) + 0.002 * r.standard_normal((h, w))
    d[60:130, 80 + 5 * seed:170 + 5 * seed] = 1.2 + 0.001 * (jj[60:130, 80:170] - 80)
    d[r.integers(0, h, 40), r.integers(0, w, 40)] = 0.0
    return d.astype(np.float32)


def torch_raycast(vol5, known5, origin, voxel, dims, world_T_cam, invK, H, W, near, step, max_steps, empty_depth=-1.0):
    """The plain march from torch ops.  vol5 (1,1,Nz,Ny,Nx): T; known5 (1,1,Nz-1,Ny-1,Nx-1): 1 where a cell's eight corners have W > 0."""
    dev = vol5.device
    ii, jj = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    q = torch.stack([jj + 0.5, ii + 0.5, torch.ones_like(ii)], -1).float() @ invK[:3, :3].T
    dc = q / q.norm(dim=-1, keepdim=True)
    dirw = dc @ world_T_cam[:3, :3].T
    og = (world_T_cam[:3, 3] - origin) / voxel
    dg = dirw / voxel
    n = torch.tensor([dims[2], dims[1], dims[0]], device=dev, dtype=torch.float32)
    scale, cscale = 2.0 / (n - 1.0), 2.0 / (n - 2.0)
    hit = torch.zeros(H, W, dtype=torch.bool, device=dev)
    t_star = torch.zeros(H, W, device=dev)
    prev_known = torch.zeros(H, W, dtype=torch.bool, device=dev)
    f_prev = torch.zeros(H, W, device=dev)
    for k in range(max_steps):
        t = near + k * step
        g = og + t * dg
        f = torch.nn.functional.grid_sample(vol5, (g * scale - 1.0)[None, None], mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, 0]
        known = torch.nn.functional.grid_sample(known5, (torch.floor(g) * cscale - 1.0)[None, None], mode="nearest", padding_mode="zeros",
                                                align_corners=True)[0, 0, 0] > 0.5
        new = ~hit & known & prev_known & (f_prev > 0) & (f <= 0)
        t_star = torch.where(new, (t - step) + step * (f_prev / (f_prev - f)), t_star)
        hit |= new
        prev_known, f_prev = known, f
    return torch.where(hit, t_star * dc[..., 2], torch.full_like(t_star, empty_depth))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_tsdf.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import fusion, raster

    dev = torch.device("cuda:0")
    centre = np.array([0.3, -0.2, 1.4])
    origin = tuple(centre - VOXEL * 0.5 * (np.array([DIMS[2], DIMS[1], DIMS[0]]) - 1.0))
    world_T_src = [_pose(0.03 * m, centre + np.array([0.02 * m, 0.04 * m, 0.0])) for m in range(4)]
    depth_all = torch.from_numpy(np.stack([source_depth(m) for m in range(4)]))[:, None].to(dev)
    K_src = syn.intrinsics(w, h).float().to(dev)
    cam_T_world = torch.from_numpy(np.stack([np.linalg.inv(T) for T in world_T_src]).astype(np.float32)).to(dev)
    step = float(np.float32(VOXEL))
    max_steps = int(math.ceil((FAR - NEAR) / step))
    res = {}
    with torch.inference_mode():
        # ---- integrate
        vols = {}
        for M in (1, 4):
            d, K, E = depth_all[:M].contiguous(), K_src[None].expand(M, 4, 4).contiguous(), cam_T_world[:M].contiguous()
            vol = fusion.TSDFVolume(DIMS, VOXEL, origin)
            vol.integrate(d, K, E)
            touched = int((vol.values[..., 1] > 0).sum())
            nbytes = touched * 16 + M * h * w * 4
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            r = {"maps": M, "voxels": DIMS[0] * DIMS[1] * DIMS[2], "touched_voxels": touched, "bytes": nbytes,
                 "flagged_blocks": int(vol.block_flags.sum()), "blocks": vol.block_flags.numel()}
            r.update(_measure({"integrate_ms": lambda: vol.integrate(d, K, E), "copy_ms": lambda: dst.copy_(src)}, a.reps, a.iters))
            res[f"integrate_M{M}"] = r
            vols[M] = fusion.TSDFVolume(DIMS, VOXEL, origin)
            vols[M].integrate(d, K, E)
        # ---- raycast
        scenes = {"room": (vols[4], _pose(0.2, centre + np.array([0.05, 0.25, -0.03]))), "sparse": (vols[1], _pose(1.2, centre + np.array([0.05, 0.25, -0.03])))}
        for name, (vol, world_T_live) in scenes.items():
            T = torch.from_numpy(world_T_live.astype(np.float32)).to(dev)
            vol5 = vol.values[..., 0][None, None].contiguous()
            seen = vol.values[..., 1] > 0
            kc = seen[:-1] & seen[1:]
            kc = kc[:, :-1] & kc[:, 1:]
            known5 = (kc[:, :, :-1] & kc[:, :, 1:]).float()[None, None].contiguous()
            origin_t = torch.tensor(origin, device=dev, dtype=torch.float32)
            for H, W in ((192, 256), (384, 512)):
                K = syn.intrinsics(W, H).float().to(dev)
                invK = torch.linalg.inv(K)
                kw = dict(near=NEAR, far=FAR)
                sides = {"raycast_skip_ms": lambda: vol.raycast(T, invK, (H, W), skip=True, **kw),
                         "raycast_plain_ms": lambda: vol.raycast(T, invK, (H, W), skip=False, **kw),
                         "raycast_skip_normals_ms": lambda: vol.raycast(T, invK, (H, W), skip=True, return_normals=True, **kw)}
                if name == "room":
                    Trel = raster.relative_poses([world_T_live], world_T_src).to(dev)
                    invK_src = torch.linalg.inv(K_src)[None].expand(4, 4, 4).contiguous()
                    sides["torch_raycast_ms"] = lambda: torch_raycast(vol5, known5, origin_t, step, DIMS, T, invK, H, W, NEAR, step, max_steps)
                    sides["warp_ms"] = lambda: raster.warp_depth(depth_all, invK_src, Trel, K[None], H, W)
                r = {"target": [H, W], "max_steps": max_steps}
                r.update(_measure(sides, a.reps, a.iters))
                s, p = sides["raycast_skip_ms"](), sides["raycast_plain_ms"]()
                r["skip_equals_plain"] = bool(torch.equal(s["depth"], p["depth"]) and torch.equal(s["flags"], p["flags"]))
                fl = s["flags"]
                r["hit_share"] = ((fl & 1) > 0).float().mean().item()
                r["none_known_share"] = ((fl & 2) > 0).float().mean().item()
                r["some_known_share"] = ((fl & 4) > 0).float().mean().item()
                if name == "room":
                    c = sides["torch_raycast_ms"]()
                    both = (s["depth"][0, 0] > 0) & (c > 0)
                    r["torch_hit_differs_share"] = ((s["depth"][0, 0] > 0) != (c > 0)).float().mean().item()
                    r["max_rel_diff_from_torch"] = ((s["depth"][0, 0] - c).abs() / c)[both].max().item()
                res[f"{name}_{H}x{W}"] = r
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
