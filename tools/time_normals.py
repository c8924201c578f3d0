"""Device time of the fused surface-normal kernel (csrc/normals.hip: depth_normals_k, k = 5) next to the torch fp32 composition the
reference's NormalGenerator executes (tests/normals_ref.py: composition), on the same GPU and inputs.  HIP events around each call, warm,
median of --reps; one JSON line per size with both times, the algorithmic bytes (4 B read + 12 B written per pixel) and the bandwidth they
imply.  python tools/time_normals.py [--reps 50] [--shape B H W ...] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SIZES = ((32, 192, 256), (1, 480, 640))
BYTES_PER_PIXEL = 16


def device_ms(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kernel-size", type=int, default=5)
    ap.add_argument("--shape", type=int, nargs=3, action="append", metavar=("B", "H", "W"), help="instead of the two default sizes; repeatable")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU"
    import normals_ref as NR
    from implicit_depth_amd import geometry

    rows = []
    for B, H, W in (args.shape or SIZES):
        depth, invK = NR.field(B, H, W).cuda(), NR.inv_intrinsics(B, H, W).cuda()
        k = args.kernel_size
        fused = lambda: geometry.depth_normals(depth, invK, kernel_size=k, std=2.0)
        comp = lambda: NR.composition(depth, invK, k, 2.0)
        diff = (fused()[0] - comp()).abs().max().item()
        # alternate the two, twice, so that a drift of the clock shows as a spread between the rounds
        t = {"fused": [], "composition": []}
        for _ in range(2):
            t["fused"].append(device_ms(fused, args.reps))
            t["composition"].append(device_ms(comp, args.reps))
        nbytes = B * H * W * BYTES_PER_PIXEL
        f_med = min(m for m, _ in t["fused"])
        row = {"shape": [B, H, W], "kernel_size": k, "reps": args.reps, "fused_ms_median": [round(m, 5) for m, _ in t["fused"]],
               "fused_ms_min": [round(m, 5) for _, m in t["fused"]], "composition_ms_median": [round(m, 5) for m, _ in t["composition"]],
               "composition_ms_min": [round(m, 5) for _, m in t["composition"]], "bytes": nbytes,
               "fused_GBps": round(nbytes / f_med / 1e6, 1), "max_abs_diff_to_composition": diff}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
