"""Times the native edge mask and the validation losses (csrc/edge_mask.hip) against their torch compositions on the
same GPU.

  "edge_mask"      ``geometry.edge_mask(depth)`` at (32,1,192,256), defaults (q = 0.95, dilation) - three launches - against the
                   composition the reference runs (tests/edge_mask_ref.composition on the device: F.pad + conv2d + sqrt,
                   ``torch.nanquantile``, the compare and ``F.max_pool2d``).  "entry_us" is ``idh_edge_mask_fwd`` through ctypes with
                   every buffer allocated before the window, at B = 1, 32 and 256: one workgroup per image selects the quantile, so
                   the way the time grows with B says whether that launch is bound by its latency.
  "bd_val_losses"  ``evaluation.bd_val_losses`` at (32,8,192,256) with an edge mask and weight 0.5 - two launches - against
                   tests/edge_mask_ref.losses32 on the device, compute_binary_losses as written (boolean indexing included).
  "bytes"          what each call must move at least once; "hbm_fraction" = bytes / time / 8 TB/s, the MI355X's HBM3E peak.

HIP-event time over --iters back-to-back calls divided by their number; --reps such windows per side, alternating, after one untimed
window of each; the median with minimum and maximum.  Prints one JSON line; --out also writes it.

    python tools/time_edge_mask.py --reps 9 --iters 50 --out profiles/edge_mask/run.json
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

H, W, D = 192, 256, 8
HBM_BYTES_PER_S = 8.0e12


def _us(t):
    return {k: {q: round(x * 1e3, 2) for q, x in v.items()} for k, v in t.items()}


def entry_call(depth):
    from implicit_depth_amd import _lib

    B, dev = depth.shape[0], depth.device
    mask = torch.empty(B, 1, H, W, device=dev)
    n = _lib.lib().idh_edge_mask_workspace_bytes(B, H, W)
    ws = torch.empty(n // 4, device=dev)
    a = _lib.EdgeMaskArgs()
    a.depth_b1hw, a.mask_b1hw, a.workspace, a.workspace_bytes = depth.data_ptr(), mask.data_ptr(), ws.data_ptr(), n
    a.q, a.dilate, a.B, a.H, a.W = 0.95, 1, B, H, W
    fn, st = _lib.lib().idh_edge_mask_fwd, _lib.stream_ptr()

    def call():
        rc = fn(a, st)
        assert rc == 0, rc

    return call, (mask, ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_edge_mask.py measures on the GPU; none is visible")
    import edge_mask_ref as E
    from implicit_depth_amd import evaluation, geometry
    from normals_ref import field

    res = {"h": H, "w": W}
    B = 32
    depth = E.with_zero_patch(field(B, H, W)).cuda()
    got, ref = geometry.edge_mask(depth), E.composition(depth)[0]
    sides = {"native": lambda: geometry.edge_mask(depth), "torch": lambda: E.composition(depth)}
    keep = []
    for b in (1, 32, 256):
        call, bufs = entry_call(E.with_zero_patch(field(b, H, W)).cuda())
        keep.append(bufs)
        sides[f"entry_B{b}"] = call
    t = _us(_measure(sides, a.reps, a.iters))
    nbytes = B * H * W * (4 + 4)  # the depth in, the mask out; the map S in between stays in the caches
    res["edge_mask"] = {"B": B, "native_us": t["native"], "torch_us": t["torch"], "entry_us": {k[6:]: v for k, v in t.items() if k.startswith("entry_")},
                        "bytes": nbytes, "hbm_fraction": round(nbytes / (t["entry_B32"]["median"] * 1e-6) / HBM_BYTES_PER_S, 4),
                        "mask_equal_torch_fraction": round(float((got == ref).float().mean()), 6), "mask_mean": round(float(got.mean()), 4)}

    pred, rendered, d = E.loss_inputs(B, D, H, W)
    cur = {"rendered_depth": rendered.cuda(), "depth_b1hw": d.cuda()}
    cur["edge_mask"] = geometry.edge_mask(cur["depth_b1hw"])
    out = {"pred_0": pred.cuda()}
    native = lambda: evaluation.bd_val_losses(out, cur, 0.5)
    comp = lambda: E.losses32(out["pred_0"], cur["rendered_depth"], cur["depth_b1hw"], cur["edge_mask"], 0.5)
    t = _us(_measure({"native": native, "torch": comp}, a.reps, a.iters))
    nbytes = B * H * W * (8 * D + 8)
    res["bd_val_losses"] = {"B": B, "D": D, "native_us": t["native"], "torch_us": t["torch"], "bytes": nbytes,
                            "hbm_fraction": round(nbytes / (t["native"]["median"] * 1e-6) / HBM_BYTES_PER_S, 4),
                            "loss_native": float(native()["loss"]), "loss_torch": float(comp()[2])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
