"""Times the mesh extraction from the TSDF volume (csrc/tsdf_mesh.hip, fusion.extract_mesh) at the full size, on the two scenes of
tools/perf_tsdf.py: the 96 x 256 x 256 grid of 4 cm voxels with four maps fused ("room") and with one ("sparse").

  "count_flags_ms" / "count_plain_ms"   ``fusion.mesh_count`` - the clear of the per-voxel words, classify, the scan - with block skipping
                      on and off; the workspace (8 B per voxel) comes from torch's caching allocator inside the window.
  "count_read_ms"     the same (flags on) followed by the host read of the two totals: what the read adds is the difference.
  "emit_ms"           ``fusion.mesh_emit`` into tensors allocated outside the window, after one count.
  "extract_flags_ms" / "extract_plain_ms"   ``fusion.extract_mesh``: count, read, allocation of the outputs, emit.
  "copy_ms"           ``Tensor.copy_`` of the volume's 8 B per voxel (as many bytes read, as many written): what one pass over the volume
                      costs a memory-bound kernel with perfect access.  Without skipping, classify reads the volume once, and the clear,
                      the two passes over the words and the vertex bases move another 16 B per voxel.
  "raycast_ms"        ``TSDFVolume.raycast`` (plain march) at 192 x 256 into perf_tsdf.py's live camera, for scale.
  "flags_equal_plain" says the two settings returned the same tensors.

Windows as in tools/perf_tsdf.py: HIP-event time over --iters back-to-back calls divided by their number; --reps such windows per side,
alternating, after one untimed window of each; the median with minimum and maximum.  Prints one JSON line; --out also writes it.

    python tools/perf_mesh.py --reps 7 --iters 20 --out profiles/mesh/run.json
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
from perf_tsdf import DIMS, FAR, NEAR, VOXEL, _pose, h, source_depth, w  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_mesh.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import fusion

    dev = torch.device("cuda:0")
    centre = np.array([0.3, -0.2, 1.4])
    origin = tuple(centre - VOXEL * 0.5 * (np.array([DIMS[2], DIMS[1], DIMS[0]]) - 1.0))
    world_T_src = [_pose(0.03 * m, centre + np.array([0.02 * m, 0.04 * m, 0.0])) for m in range(4)]
    depth_all = torch.from_numpy(np.stack([source_depth(m) for m in range(4)]))[:, None].to(dev)
    K_src = syn.intrinsics(w, h).float().to(dev)
    cam_T_world = torch.from_numpy(np.stack([np.linalg.inv(T) for T in world_T_src]).astype(np.float32)).to(dev)
    n = DIMS[0] * DIMS[1] * DIMS[2]
    src = torch.empty(8 * n, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    live = {"room": _pose(0.2, centre + np.array([0.05, 0.25, -0.03])), "sparse": _pose(1.2, centre + np.array([0.05, 0.25, -0.03]))}
    invK = torch.linalg.inv(syn.intrinsics(256, 192).float().to(dev))
    res = {}
    with torch.inference_mode():
        for name, M in (("room", 4), ("sparse", 1)):
            vol = fusion.TSDFVolume(DIMS, VOXEL, origin)
            vol.integrate(depth_all[:M].contiguous(), K_src[None].expand(M, 4, 4).contiguous(), cam_T_world[:M].contiguous())
            on, off = fusion.extract_mesh(vol, return_weights=True, use_block_flags=True), fusion.extract_mesh(vol, return_weights=True, use_block_flags=False)
            V, F = on["verts"].shape[0], on["faces"].shape[0]
            workspace, _ = fusion.mesh_count(vol)
            verts, faces = torch.empty(V, 3, device=dev), torch.empty(F, 3, device=dev, dtype=torch.int32)
            T = torch.from_numpy(live[name].astype(np.float32)).to(dev)
            r = {"maps": M, "voxels": n, "volume_bytes": 8 * n, "workspace_bytes": workspace.numel(), "verts": V, "faces": F,
                 "flagged_blocks": int(vol.block_flags.sum()), "blocks": vol.block_flags.numel(),
                 "flags_equal_plain": bool(all(torch.equal(on[k], off[k]) for k in on))}
            r.update(_measure({
                "count_flags_ms": lambda: fusion.mesh_count(vol, use_block_flags=True),
                "count_plain_ms": lambda: fusion.mesh_count(vol, use_block_flags=False),
                "count_read_ms": lambda: fusion.mesh_count(vol, use_block_flags=True)[1].tolist(),
                "emit_ms": lambda: fusion.mesh_emit(vol, workspace, verts, faces),
                "extract_flags_ms": lambda: fusion.extract_mesh(vol, use_block_flags=True),
                "extract_plain_ms": lambda: fusion.extract_mesh(vol, use_block_flags=False),
                "copy_ms": lambda: dst.copy_(src),
                "raycast_ms": lambda: vol.raycast(T, invK, (192, 256), near=NEAR, far=FAR),
            }, a.reps, a.iters))
            res[name] = r
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
