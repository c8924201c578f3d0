"""Times the native ResNet18 matching stem at the bench shape (256 images of 512 x 384 = 32 frames of K + 1 = 8 views):

  stem_kernel      IDH_OP_STEM alone (conv1 + folded bn1 + ReLU + MaxPool2d(2, 1) + BlurPool, csrc/stem.hip)
  stem_layer1      the stem pass + layer1's four folded 3x3 convs (nhwc.build_matching_stem), one plan
  torch_modules    the same five modules in torch fp32 eval mode (MIOpen), NCHW
  fused_forward    dropin.fused_forward, B = 32, K = 7, BDModel with the MLP feature volume, with and without native_matching_stem

HIP-event device ms per call over --iters calls after --warmup.  Prints one JSON line; the stem kernel's fraction of the fp32 matrix peak
(155 TFLOP/s measured) counts conv1's algorithmic 2 x 147 x 64 flops per conv1 pixel, not the halo recompute.

    python tools/perf_matching_stem.py --iters 10
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def run(iters, warmup, skip_fused=False):
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import nhwc
    from test_matching_stem_gpu import _encoder, _model

    B, K, H, W = 32, 7, 384, 512
    N = B * (K + 1)
    res = {"images": N, "H": H, "W": W}
    e = _encoder().cuda()
    x = torch.randn(N, 3, H, W, device="cuda")

    fs = nhwc.folded_stem(e, x.device)
    p = nhwc.Plan(x.device)
    out = p.buffer(N, H // 4, W // 4, 64)
    i = p.stem((N, 3, H, W), (N, 3 * H * W, N * 3 * H * W), fs.blob, out)
    p.set_in(i, x)
    res["stem_kernel_ms"] = _ms(p.run, iters, warmup)
    conv1_flop = 2 * N * (H // 2) * (W // 2) * 64 * 147
    res["stem_kernel_tflops"] = round(conv1_flop / res["stem_kernel_ms"] / 1e9, 1)
    res["stem_kernel_frac_fp32_matrix_peak"] = round(res["stem_kernel_tflops"] / 155.0, 3)

    p2 = nhwc.Plan(x.device)
    _, i2 = nhwc.build_matching_stem(p2, e, x)
    p2.schedule()
    p2.set_in(i2, x)
    res["stem_layer1_ms"] = _ms(p2.run, iters, warmup)
    res["stem_layer1_launches"] = p2.count_launches()

    stem = e.net[:5]
    with torch.inference_mode():
        res["torch_modules_ms"] = _ms(lambda: stem(x), iters, warmup)
    del x, out, p, p2
    torch.cuda.empty_cache()

    if not skip_fused:
        from implicit_depth_amd.dropin import fused_forward

        m = _model(K, "bd", seed=40)
        cur, src = syn.frame_tuple(B, K, H, W, seed=41, P=8)
        cur = {k: v.cuda() for k, v in cur.items()}
        src = {k: v.cuda() for k, v in src.items()}
        for name, nat in (("fused_forward_torch_stem_ms", False), ("fused_forward_native_stem_ms", True)):
            f = fused_forward(m, native_matching_stem=nat)
            res[name] = _ms(lambda: f("test", cur, src), max(2, iters // 2), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-fused", action="store_true", help="stem timings only (e.g. under a kernel trace)")
    a = ap.parse_args()
    print(json.dumps(run(a.iters, a.warmup, a.skip_fused)))


if __name__ == "__main__":
    main()
