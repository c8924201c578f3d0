"""Times the TSDF pose alignment (csrc/tsdf_align.hip, fusion.align_depth) at the full size of tools/perf_tsdf.py: a
192 x 256 map against the 96 x 256 x 256 volume its four maps fused, starting 2 cm and 0.6 degrees off map 0's pose.

  "align_s1_ms" / "align_s2_ms"   one ``align_depth(iters=8)`` call at stride 1 and stride 2: sixteen launches, no synchronisation.
  "align_1iter_ms"                the same call with ``iters=1``; (align_s1_ms - align_1iter_ms) / 7 is "pair_ms", one further rows + solve pair.
  "torch_rows_ms"                 ONE per-pixel pass and its sums composed from torch ops in fp32 (the eight corners gathered with index
                                  arithmetic, no grid_sample; J^T J by one matmul in fp64): the baseline of one rows launch.  It is a
                                  timing helper and lives here, not in the package.
  "end_*"                         where the 8-iteration fit ends against map 0's own pose.

HIP-event time over --iters back-to-back calls divided by their number; --reps such windows per side, alternating, after one untimed
window of each; the median with minimum and maximum (tools/perf_ray_queries._measure).  Host work of a call (ctypes, the launches, torch's
allocation of outputs and workspace) is inside the window.  Prints one JSON line; --out also writes it.

    python tools/perf_tsdf_align.py --reps 7 --iters 20 --out profiles/tsdf/align.json
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

from perf_ray_queries import _measure  # noqa: E402
from perf_tsdf import DIMS, VOXEL, _pose, h, source_depth, w  # noqa: E402


def torch_rows(values, origin, voxel, trunc_voxels, depth, invK, pose):
    """One per-pixel pass of include/idh_fusion.h's alignment from torch ops: (A (6,6), b (6), cost, count) on the device."""
    dev = depth.device
    Nz, Ny, Nx = values.shape[:3]
    ii, jj = torch.meshgrid(torch.arange(depth.shape[0], device=dev), torch.arange(depth.shape[1], device=dev), indexing="ij")
    q = torch.stack([jj + 0.5, ii + 0.5, torch.ones_like(ii)], -1).float() @ invK[:3, :3].T
    pw = (q * depth[..., None]) @ pose[:3, :3].T + pose[:3, 3]
    g = (pw - origin) / voxel
    cell = torch.floor(g)
    ok = torch.isfinite(depth) & (depth > 0) & (cell >= 0).all(-1) & (cell[..., 0] <= Nx - 2) & (cell[..., 1] <= Ny - 2) & (cell[..., 2] <= Nz - 2)
    c = torch.where(ok[..., None], cell, torch.zeros_like(cell)).long()
    r = g - cell
    flat = values.reshape(-1, 2)
    base = (c[..., 2] * Ny + c[..., 1]) * Nx + c[..., 0]
    T = {}
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                tw = flat[base + (dz * Ny + dy) * Nx + dx]
                T[dz, dy, dx] = tw[..., 0]
                ok = ok & (tw[..., 1] > 0)
    rx, ry, rz = r[..., 0], r[..., 1], r[..., 2]
    L = lambda a, b, t: a + t * (b - a)  # noqa: E731
    f = L(L(L(T[0, 0, 0], T[0, 0, 1], rx), L(T[0, 1, 0], T[0, 1, 1], rx), ry), L(L(T[1, 0, 0], T[1, 0, 1], rx), L(T[1, 1, 0], T[1, 1, 1], rx), ry), rz)
    Gx = L(L(T[0, 0, 1] - T[0, 0, 0], T[0, 1, 1] - T[0, 1, 0], ry), L(T[1, 0, 1] - T[1, 0, 0], T[1, 1, 1] - T[1, 1, 0], ry), rz)
    Gy = L(L(T[0, 1, 0] - T[0, 0, 0], T[0, 1, 1] - T[0, 0, 1], rx), L(T[1, 1, 0] - T[1, 0, 0], T[1, 1, 1] - T[1, 0, 1], rx), rz)
    Gz = L(L(T[1, 0, 0] - T[0, 0, 0], T[1, 0, 1] - T[0, 0, 1], rx), L(T[1, 1, 0] - T[0, 1, 0], T[1, 1, 1] - T[0, 1, 1], rx), ry)
    G = torch.stack([Gx, Gy, Gz], -1)
    ok = ok & ((G * G).sum(-1) != 0)
    n = G * trunc_voxels
    J = torch.cat([n, torch.linalg.cross(pw - pose[:3, 3], n)], -1)
    J = torch.where(ok[..., None], J, torch.zeros_like(J)).reshape(-1, 6).double()
    res = torch.where(ok, f * (trunc_voxels * voxel), torch.zeros_like(f)).reshape(-1).double()
    return J.T @ J, J.T @ res, (res * res).sum(), ok.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_tsdf_align.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import fusion

    dev = torch.device("cuda:0")
    centre = np.array([0.3, -0.2, 1.4])
    origin = tuple(centre - VOXEL * 0.5 * (np.array([DIMS[2], DIMS[1], DIMS[0]]) - 1.0))
    world_T_src = [_pose(0.03 * m, centre + np.array([0.02 * m, 0.04 * m, 0.0])) for m in range(4)]
    depth_all = torch.from_numpy(np.stack([source_depth(m) for m in range(4)]))[:, None].to(dev)
    K = syn.intrinsics(w, h).float().to(dev)
    invK = torch.linalg.inv(K)
    cam_T_world = torch.from_numpy(np.stack([np.linalg.inv(T) for T in world_T_src]).astype(np.float32)).to(dev)
    start = _pose(0.01, centre + np.array([0.012, -0.012, 0.01]))
    res = {}
    with torch.inference_mode():
        vol = fusion.TSDFVolume(DIMS, VOXEL, origin)
        vol.integrate(depth_all, K[None].expand(4, 4, 4).contiguous(), cam_T_world)
        d = depth_all[:1].contiguous()
        T = torch.from_numpy(start.astype(np.float32)).to(dev)
        origin_t = torch.tensor(origin, device=dev, dtype=torch.float32)
        sides = {"align_s1_ms": lambda: fusion.align_depth(vol, d, invK, T, iters=8),
                 "align_s2_ms": lambda: fusion.align_depth(vol, d, invK, T, iters=8, stride=2),
                 "align_1iter_ms": lambda: fusion.align_depth(vol, d, invK, T, iters=1),
                 "torch_rows_ms": lambda: torch_rows(vol.values, origin_t, VOXEL, vol.trunc_voxels, d[0, 0], invK, T)}
        res.update(_measure(sides, a.reps, a.iters))
        res["pair_ms"] = (res["align_s1_ms"]["median"] - res["align_1iter_ms"]["median"]) / 7 if isinstance(res["align_s1_ms"], dict) else None
        out = sides["align_s1_ms"]()
        rec = out["records"].cpu().numpy()
        A, b, cost, count = torch_rows(vol.values, origin_t, VOXEL, vol.trunc_voxels, d[0, 0], invK, T)
        res["count"], res["torch_count"] = int(rec[0, 28]), int(count)
        res["torch_cost_rel_diff"] = abs(float(cost) - rec[0, 27]) / rec[0, 27]
        res["statuses"] = rec[:, 29].tolist()
        end = out["world_T_cam"][0].cpu().numpy().astype(np.float64)
        res["start_translation_m"] = float(np.linalg.norm(start[:3, 3] - world_T_src[0][:3, 3]))
        res["end_translation_m"] = float(np.linalg.norm(end[:3, 3] - world_T_src[0][:3, 3]))
        res["end_rotation_rad"] = float(np.arccos(np.clip((np.trace(end[:3, :3] @ world_T_src[0][:3, :3].T) - 1) / 2, -1, 1)))
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
