"""Times DepthModel's native validation losses (csrc/reg_losses.hip) against the torch composition on the same GPU.

  "reg_val_losses"  ``evaluation.reg_val_losses(outputs, cur_data, src_data)`` at (32,1,192,256), four log-depth scales and K = 7 source
                    views - five launches plus the two of the multi-view term - against tests/reg_losses_ref.compute_losses32 on the
                    device: compute_losses as written (the pyramid and Sobel convolutions, boolean indexing, K rounds of projection
                    and grid_sample).
  "entry_us"        ``idh_reg_val_losses_fwd`` alone through ctypes with every buffer allocated before the window (mv_loss a device
                    scalar computed before): what the five launches cost without the wrapper and without the multi-view term.
  "mv"              the multi-view term alone on both sides (geometry.depth_consistency(return_loss=True) / mv_loss32): §4.25's kernels,
                    listed so that the rest can be read off.
  "bytes"           what the five launches must move at least once: level 0 reads both depth maps, the mask, the four log-depth
                    scales and the two normal maps; level l writes and level l + 1 reads both maps of the pyramid as doubles.
                    "hbm_fraction" = bytes / entry time / 8 TB/s, the MI355X's HBM3E peak.

HIP-event time over --iters back-to-back calls divided by their number; --reps such windows per side, alternating, after one untimed
window of each; the median with minimum and maximum.  Prints one JSON line; --out also writes it.

    python tools/time_reg_losses.py --reps 9 --iters 50 --out profiles/reg_losses/run.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from perf_ray_queries import _measure  # noqa: E402

B, H, W, K = 32, 192, 256, 7
HBM_BYTES_PER_S = 8.0e12


def _us(t):
    return {k: {q: round(x * 1e3, 2) for q, x in v.items()} for k, v in t.items()}


def entry_call(cur, outputs, mv):
    from implicit_depth_amd import _lib

    dev = mv.device
    a = _lib.RegValLossesArgs()
    a.depth_gt_b1hw, a.depth_pred_b1hw, a.mask_b_b1hw = cur["depth_b1hw"].data_ptr(), outputs["depth_pred_s0_b1hw"].data_ptr(), cur["mask_b_b1hw"].data_ptr()
    for i in range(4):
        t = outputs[f"log_depth_pred_s{i}_b1hw"]
        a.log_depth_pred_s[i], a.scale_h[i], a.scale_w[i] = t.data_ptr(), t.shape[2], t.shape[3]
    a.normals_gt_b3hw, a.normals_pred_b3hw, a.mv_loss = cur["normals_b3hw"].data_ptr(), outputs["normals_pred_b3hw"].data_ptr(), mv.data_ptr()
    n = _lib.lib().idh_reg_val_losses_workspace_bytes(B, H, W)
    ws, out = torch.empty(n // 8, device=dev, dtype=torch.float64), torch.empty(16, device=dev, dtype=torch.float64)
    a.out16, a.workspace, a.workspace_bytes, a.si_lambda, a.B, a.h, a.w = out.data_ptr(), ws.data_ptr(), n, 0.85, B, H, W
    fn, st = _lib.lib().idh_reg_val_losses_fwd, _lib.stream_ptr()

    def call():
        rc = fn(a, st)
        assert rc == 0, rc

    return call, (ws, out)


def level_bytes():
    """Bytes per launch: [level 0 .. level 3]."""
    sizes = [(H, W)]
    for _ in range(3):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    px = [B * h * w for h, w in sizes]
    logs = sum(4 * B * (H >> i) * (W >> i) for i in range(4))
    out = [px[0] * (4 + 4 + 1 + 24) + logs + 16 * px[1]]
    for l in (1, 2, 3):
        out.append(16 * px[l] + (16 * px[l + 1] if l < 3 else 0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_reg_losses.py measures on the GPU; none is visible")
    import reg_losses_ref as R
    from implicit_depth_amd import evaluation, geometry

    cur, src, outputs = ({k: v.cuda() for k, v in d.items()} for d in R.inputs(B, H, W, K, settle=False))
    mv_args = (outputs["depth_pred_s0_b1hw"], cur["invK_s0_b44"], cur["world_T_cam_b44"], src["depth_b1hw"], src["K_s0_b44"], src["cam_T_world_b44"])
    native_mv = lambda: geometry.depth_consistency(*mv_args, gate_depth=cur["depth_b1hw"], return_loss=True)["loss"]
    torch_mv = lambda: R.mv_loss32(outputs["depth_pred_s0_b1hw"], cur["depth_b1hw"], src["depth_b1hw"], cur["invK_s0_b44"], src["K_s0_b44"],
                                   cur["world_T_cam_b44"], src["cam_T_world_b44"])
    native = lambda: evaluation.reg_val_losses(outputs, cur, src)
    comp = lambda: R.compute_losses32(cur, src, outputs)
    entry, bufs = entry_call(cur, outputs, native_mv())
    with torch.no_grad():
        t = _us(_measure({"native": native, "torch": comp, "entry": entry, "native_mv": native_mv, "torch_mv": torch_mv}, a.reps, a.iters))
        got, ref = native(), comp()
    per_level = level_bytes()
    res = {"B": B, "h": H, "w": W, "K": K,
           "reg_val_losses": {"native_us": t["native"], "torch_us": t["torch"]}, "entry_us": t["entry"],
           "mv": {"native_us": t["native_mv"], "torch_us": t["torch_mv"]},
           "bytes_per_level": per_level, "bytes": sum(per_level),
           "hbm_fraction": round(sum(per_level) / (t["entry"]["median"] * 1e-6) / HBM_BYTES_PER_S, 4),
           "values_native": {k: float(got[k]) for k in R.KEYS}, "values_torch": {k: float(ref[k]) for k in R.KEYS}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
