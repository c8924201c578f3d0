"""Times the AR compositing kernels (csrc/composite.hip) at ARKit resolution — 1440 x 1920 camera image, 192 x 256 map, RGBA render,
B = 1 and B = 8 — and, as the streaming yardstick of the same card, layout.hip's NCHW -> NHWC copy of about the same number of bytes.

"us_per_call": HIP-event time per call over --iters back-to-back calls through implicit_depth_amd.compositing after --warmup: output
allocation and launch overhead included, so an upper bound on device time.  Kernel times come from running this script under
`rocprofv3 --kernel-trace --stats` (profiles/composite/README.md); the script prints, per case, the bytes a kernel must move so that the
trace's durations can be turned into GB/s: image 3 + render 4 + output 3 = 10 B per pixel (the map is L2-resident), 8 B per output pixel
for the preparation, 8 B per float for the copy.  --ref-frames N also times tests/composite_ref.py (our numpy restatement, not the
reference's program) on the host.  Prints one JSON line; --out also writes it.

    python tools/perf_composite.py --iters 50 --warmup 10 --out profiles/composite/run.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, MH, MW = 1440, 1920, 192, 256


def _us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ref-frames", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_composite.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import _lib
    from implicit_depth_amd import compositing as cp

    res = {}

    def record(name, fn, nbytes):
        us = _us(fn, a.iters, a.warmup)
        res[name] = {"us_per_call": round(us, 1), "bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1)}

    case1 = syn.composite_case(1, MH, MW, H, W, 1, render_hw=(H, W))
    with torch.inference_mode():
        for B in (1, 8):
            c = {k: v.repeat(B, *([1] * (v.dim() - 1))).cuda() for k, v in case1.items()}
            px = B * H * W
            record(f"composite_logits_rgba_B{B}", lambda: cp.composite_mask(c["image"], c["logits"], virtual_rgba=c["rgba"]), 10 * px)
            record(f"composite_prob_rgba_B{B}", lambda: cp.composite_mask(c["image"], c["prob"], logits=False, virtual_rgba=c["rgba"]), 10 * px)
            record(f"composite_depth_soft_map_B{B}", lambda: cp.composite_depth(c["image"], c["depth"], virtual_depth=c["virtual_depth"], virtual_rgba=c["rgba"]), 14 * px)
            record(f"prep_B{B}", lambda: cp.prepare_rendered_depth(c["render"], (MH, MW)), 8 * B * MH * MW)
            # layout.hip's copy, the streaming yardstick: 64 channels at 96 x 128 as in the hot path, as many images as give 10 B * px
            n_img = max(1, round(10 * px / (8 * 64 * 96 * 128)))
            src = torch.empty(n_img, 64, 96, 128, device="cuda").normal_()
            dst = torch.empty(n_img, 96, 128, 64, device="cuda")
            copy = lambda: _lib.check(_lib.lib().idh_nchw_to_nhwc_f32(src.data_ptr(), dst.data_ptr(), n_img, 64, 96 * 128, _lib.stream_ptr()), "idh_nchw_to_nhwc_f32")
            record(f"layout_nchw_to_nhwc_B{B}", copy, 8 * src.numel())
            del src, dst
    if a.ref_frames:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import composite_ref as cr

        t0 = time.perf_counter()
        for _ in range(a.ref_frames):
            cr.composite(case1["image"], occlusion=case1["logits"], virtual_rgba=case1["rgba"])
        res["composite_ref_cpu_ms_per_frame"] = round(1e3 * (time.perf_counter() - t0) / a.ref_frames, 1)
    res["shape"] = {"H": H, "W": W, "h": MH, "w": MW, "iters": a.iters, "warmup": a.warmup}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
