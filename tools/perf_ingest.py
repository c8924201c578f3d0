"""Times the frame ingest (csrc/ingest.hip) for a batch of 32 frames, and beside it the reference's own procedure on this host:

  arkit_bicubic    load_color, 1920 x 1440 -> 512 x 384, bicubic (ARKit frames; 8.3 MB in per frame)
  scannet_bilinear load_color, 640 x 480 -> 512 x 384, bilinear
  depth            load_depth, 640 x 480 -> 256 x 192 (target-size triple)

"event_ms": HIP-event time per call over --iters back-to-back calls after --warmup.  A call is one or two allocations, a ctypes call and one
kernel launch: an upper bound on device time, not a kernel time.  "bytes" is what the call must move, computed from shapes (frames in,
floats out); "hbm_fraction" is bytes / time over the 8 TB/s peak of the MI355X's HBM.
"host_ms": what the reference does per batch on the CPU (utils/generic_utils.py:193-212, :149-152): ``Image.resize``, ``to_tensor``,
``normalize`` per frame on up to 16 threads, then one ``.cuda()`` of the float batch, timed by the host clock around a device
synchronise; PNG decoding is NOT included.  Skipped (null) when Pillow is not installed.  The comparison recorded is against that
procedure: this code has no parent to compare with.  Prints one JSON line; --out also writes it.

    python tools/perf_ingest.py --iters 50 --warmup 10 --out profiles/ingest.json
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _host_color(frames, size, resample, reps):
    """The reference's loader for one batch, from decoded frames: milliseconds, or None without Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return None
    pf = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[resample]
    mean, std = torch.tensor(MEAN)[:, None, None], torch.tensor(STD)[:, None, None]
    images = [Image.fromarray(f) for f in frames]

    def one(img):
        r = img.resize((size[1], size[0]), resample=pf) if img.size != (size[1], size[0]) else img
        t = torch.from_numpy(np.asarray(r).copy()).permute(2, 0, 1).contiguous().float().div(255)
        return t.sub_(mean).div_(std)

    times = []
    with cf.ThreadPoolExecutor(max_workers=min(16, len(images))) as ex:
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.stack(list(ex.map(one, images))).cuda()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    return min(times[1:])  # the first repetition warms the pool and the allocator


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_ingest.py measures on the GPU; none is visible")
    from implicit_depth_amd import ingest

    dev, B = torch.device("cuda:0"), a.batch
    rng = np.random.default_rng(0)
    res = {}
    for name, (Hs, Ws), (h, w), resample in (("arkit_bicubic", (1440, 1920), (384, 512), "bicubic"), ("scannet_bilinear", (480, 640), (384, 512), "bilinear")):
        host = rng.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)
        frames = torch.from_numpy(host).to(dev)
        ms = _ms(lambda: ingest.load_color(frames, (h, w), resample=resample), a.iters, a.warmup)
        nbytes = B * (Hs * Ws * 3 + h * w * 3 * 4)
        host_ms = _host_color(host, (h, w), resample, a.host_reps)
        res[name] = {"event_ms": round(ms, 4), "frames_per_s": round(B / ms * 1e3, 1), "bytes": nbytes,
                     "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4), "host_ms": None if host_ms is None else round(host_ms, 2),
                     "host_frames_per_s": None if host_ms is None else round(B / host_ms * 1e3, 1),
                     "source": [Hs, Ws], "target": [h, w], "resample": resample}
        del frames
    Hs, Ws, h, w = 480, 640, 192, 256
    depth = torch.from_numpy(rng.integers(0, 12000, (B, Hs, Ws)).astype(np.uint16)).to(dev)
    ms = _ms(lambda: ingest.load_depth(depth, (h, w)), a.iters, a.warmup)
    nbytes = B * h * w * (2 + 4 + 4 + 1)  # the pixels sampled, two float maps and the bool mask
    res["depth"] = {"event_ms": round(ms, 4), "frames_per_s": round(B / ms * 1e3, 1), "bytes": nbytes,
                    "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4), "source": [Hs, Ws], "target": [h, w]}
    res["shape"] = {"batch": B, "iters": a.iters, "warmup": a.warmup, "host_threads": min(16, B)}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
