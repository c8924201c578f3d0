"""Feature volume, load balance of the task order of the skipping kernel fv_mlp_k<KT, true>: a CPU model, no GPU needed.

  python tools/fv_task_balance.py [cameras ...] [--B 32]        cameras: bench identity tuple31 golden_g2 (tools/perf_fv_skip.py), default all

Since views that see nothing are dropped per (16-pixel tile, plane), a task costs between 352 and 576 MFMAs per plane.  The model restates
prologue()'s bilinear weights in fp64 (a sample has no weight when x falls outside (-1, W) or y outside (-1, H) after the -0.5 shift, z clamped to
1e-5), prices a task at  sum over its planes of (352 + 32 * active_views(tile, plane))  - matrix instructions only, the constant vector work per
plane is not in it - and sums what each wave, SIMD and CU of the persistent grid is handed:
  shipped   the static stride of the uniform-cost kernels: wave w of a workgroup takes sub-slot w of the workgroup's eight tasks of every round
  rotated   the skipping kernel's order, read through idh_feature_volume_skip_task (the function the kernel calls)
Printed per camera set: the dropped shares, the mean cost per wave index relative to the mean, and busiest / mean over the SIMDs (waves w and w + 4
of a workgroup share a SIMD; in brackets: waves 2s and 2s + 1) and over the CUs of the chip, for both orders.  Then, as a record for a later
decision and NOT built: workgroup-local dynamic fetching - the workgroup's tasks of all rounds in one queue, each split into 1 / 2 / 4 plane
ranges, the next item going to the wave that is free first - which would need an LDS word that K = 8 does not have, and tasks split by plane.
"""
import ctypes
import heapq
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import perf_fv_skip as pfs
from implicit_depth_amd import _lib

K, H, W, D = pfs.K, pfs.H, pfs.W, pfs.D


def outside(inp, depths):
    """(B, K, D, N) bool: the sample of view k at plane d, pixel n has four zero bilinear weights.  fp64, one frame at a time."""
    Ks, E, iK = inp["src_Ks"].double().cpu(), inp["src_extrinsics"].double().cpu(), inp["cur_invK"].double().cpu()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=torch.float64)])
    res = []
    for b in range(Ks.shape[0]):
        P = Ks[b] @ E[b]
        q = P[:, :3, :3] @ iK[b, None, :3, :3] @ pix
        cam = depths.view(1, -1, 1, 1) * q[:, None] + P[:, None, :3, 3:4]
        z = cam[..., 2, :].clamp_min(1e-5)
        sx, sy = cam[..., 0, :] / z - 0.5, cam[..., 1, :] / z - 0.5
        res.append((sx <= -1) | (sx >= W) | (sy <= -1) | (sy >= H))
    return torch.stack(res)


def task_costs(out, G, DP):
    """MFMAs of every task (frame, tile, plane group), in task order: task = (frame * tiles + tile) * G + group."""
    B, Kv, Dn, N = out.shape
    pad = (-N) % 16
    if pad:
        out = torch.cat([out, out[..., -1:].expand(B, Kv, Dn, pad)], -1)
    dropped = out.reshape(B, Kv, Dn, -1, 16).all(-1)  # B,K,D,tiles
    active = (~dropped).sum(1)  # B,D,tiles
    per_plane = (352 + 32 * active).permute(0, 2, 1).numpy().astype(np.int64)  # B,tiles,D
    groups = [per_plane[..., g * DP:min(Dn, (g + 1) * DP)] for g in range(G)]
    cost = np.stack([g.sum(-1) for g in groups], -1).reshape(-1)  # tasks
    planes = np.stack([np.pad(g, ((0, 0), (0, 0), (0, DP - g.shape[-1]))) for g in groups], 2).reshape(-1, DP)  # tasks, DP (for the split model)
    return cost, planes, dropped.double().mean().item()


def xcd_remap(bid, nblocks):
    """idh_xcd_remap (csrc/idh_common.h), for the shipped order; the rotated one comes from the library."""
    full, rem = divmod(nblocks, 8)
    xcd, slot = bid % 8, bid // 8
    return xcd * full + min(xcd, rem) + slot


def orders(ntasks, grid):
    """task[order][block][wave][round] (-1: none)."""
    L = _lib.lib()
    rounds = -(-ntasks // (grid * 8))
    shipped = np.full((grid, 8, rounds), -1, dtype=np.int64)
    rotated = np.full((grid, 8, rounds), -1, dtype=np.int64)
    for b in range(grid):
        lb = xcd_remap(b, grid)
        for w in range(8):
            for r in range(rounds):
                t = (r * grid + lb) * 8 + w
                shipped[b, w, r] = t if t < ntasks else -1
                rotated[b, w, r] = L.idh_feature_volume_skip_task(ntasks, grid, b, w, r)
    for o in (shipped, rotated):
        assert sorted(o[o >= 0].tolist()) == list(range(ntasks))
    return {"shipped": shipped, "rotated": rotated}


def balance(order, cost):
    load = np.where(order >= 0, cost[np.maximum(order, 0)], 0).sum(-1).astype(np.float64)  # grid, 8
    mean_wave = load.mean()
    simd_a = load[:, :4] + load[:, 4:]          # waves w, w + 4
    simd_b = load.reshape(-1, 4, 2).sum(-1)     # waves 2s, 2s + 1
    cu = load.sum(-1)
    return {"wave_index_cost": [round(v, 3) for v in (load.mean(0) / mean_wave).tolist()],
            "simd_busiest_over_mean": round(simd_a.max() / simd_a.mean(), 4), "simd_busiest_over_mean_pairs": round(simd_b.max() / simd_b.mean(), 4),
            "cu_busiest_over_mean": round(cu.max() / cu.mean(), 4)}


def dynamic(order, planes, split):
    """Workgroup-local dynamic fetch: busiest SIMD / mean SIMD when each workgroup's tasks (its rounds in order, eight per round) are split into
    `split` plane ranges and handed, in that order, to whichever of the eight waves is free first (waves w, w + 4 share a SIMD)."""
    DP = planes.shape[1]
    edges = [DP * i // split for i in range(split + 1)]
    simd = []
    for b in range(order.shape[0]):
        tasks = sorted(t for t in order[b].T.reshape(-1).tolist() if t >= 0)
        items = [planes[t, edges[i]:edges[i + 1]].sum() for t in tasks for i in range(split)]
        free = [(0, w) for w in range(8)]
        heapq.heapify(free)
        load = [0] * 8
        for c in items:
            t0, w = heapq.heappop(free)
            load[w] += int(c)
            heapq.heappush(free, (t0 + int(c), w))
        simd += [load[w] + load[w + 4] for w in range(4)]
    simd = np.array(simd, dtype=np.float64)
    return round(simd.max() / simd.mean(), 4)


def main():
    args = sys.argv[1:]
    B = 32
    if "--B" in args:
        i = args.index("--B")
        B = int(args[i + 1])
        del args[i:i + 2]
    sets = pfs.camera_sets(B)
    names = args or list(sets)
    depths = pfs.plane_depths(D, pfs.DMIN, pfs.DMAX)
    L = _lib.lib()
    g, dp = ctypes.c_int(), ctypes.c_int()
    _lib.check(L.idh_feature_volume_plane_groups(B, H, W, D, ctypes.byref(g), ctypes.byref(dp)), "idh_feature_volume_plane_groups")
    G, DP = g.value, dp.value
    for name in names:
        out = outside(sets[name], depths)
        cost, planes, dropped = task_costs(out, G, DP)
        ntasks = cost.shape[0]
        grid = L.idh_feature_volume_grid(ntasks)
        res = {"cameras": name, "B": B, "groups": G, "ntasks": ntasks, "grid": grid, "outside_samples": round(out.double().mean().item(), 4),
               "dropped_groups": round(dropped, 4), "task_cost_min_mean_max": [int(cost.min()), round(float(cost.mean()), 1), int(cost.max())]}
        od = orders(ntasks, grid)
        for k, o in od.items():
            res[k] = balance(o, cost)
        res["dynamic_fetch_simd_busiest_over_mean"] = {str(s): dynamic(od["shipped"], planes, s) for s in (1, 2, 4)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
