"""Times the whole-model C entry (idh_model_fwd) against HotPath on the same inputs: HotPath.forward, the C entry run eagerly, and the C entry
captured once in torch.cuda.graph on one stream (a linear graph) and replayed.

  (a) B = 32, K = 7, D = 64, BDModel with the MLP feature volume at 512 x 384 (bench.py's headline shapes)
  (b) the B = 1, D = 96 temporal loop with use_prior: frame by frame (prior_inputs of the previous frame), and as a 4-frame chain

Per variant: HIP-event device ms per frame, wall-clock frames/s over back-to-back iterations (host enqueue included, one sync at the end), and the
host's enqueue ms per frame (perf_counter around the call, no sync).  Prints one JSON object and writes it to --out.

    python tools/perf_model_entry.py --iters 50 --out profiles/model_entry/run.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _time(fn, frames, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    enq = 0.0
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        a = time.perf_counter()
        fn()
        enq += time.perf_counter() - a
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dev_ms = e0.elapsed_time(e1) / iters / frames
    return {"device_ms_per_frame": round(dev_ms, 4), "wall_frames_per_s": round(iters * frames / wall, 1),
            "enqueue_ms_per_frame": round(1e3 * enq / iters / frames, 4), "ideal_frames_per_s": round(1e3 / dev_ms, 1)}


def _graph(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def run(iters, warmup):
    from test_model_abi_gpu import _prior_inputs, _setup

    from implicit_depth_amd import model_abi as m

    res = {}
    with torch.inference_mode():
        # (a) headline shapes
        B, K, h, w = 32, 7, 384, 512
        hp, ent, cur, args = _setup(K, "mlp", "bd", False, B, h, w, P=1)
        rd = cur["rendered_depth"].contiguous()
        plan = ent.prepare(B, K, 16, h // 4, w // 4, rd.shape[1])
        out = ent(**args, rendered_depth=rd, plan=plan)
        res["a_b32_k7_d64"] = {"hotpath": _time(lambda: hp(**args, rendered_depth=rd), B, iters, warmup),
                               "c_entry": _time(lambda: ent(**args, rendered_depth=rd, plan=plan, out=out), B, iters, warmup),
                               "c_entry_graph": _time(_graph(lambda: ent(**args, rendered_depth=rd, plan=plan, out=out)), B, iters, warmup)}
        del hp, ent, args, out
        torch.cuda.empty_cache()
        # (b) temporal, D = 96: one frame per call, then a 4-frame chain per call
        K, h, w = 7, 384, 512
        hp, ent, cur, args = _setup(K, "mlp", "bd", True, 1, h, w, P=1, D=96)
        rd = cur["rendered_depth"].contiguous()
        pin = _prior_inputs(cur, 1, h, w)
        plan = ent.prepare(1, K, 16, h // 4, w // 4, 1, prior_mode=m.PRIOR_INPUTS)
        out = ent(**args, rendered_depth=rd, prior_inputs=pin, plan=plan)
        res["b_temporal_d96_frame"] = {"hotpath": _time(lambda: hp(**args, rendered_depth=rd, prior_inputs=pin), 1, iters, warmup),
                                       "c_entry": _time(lambda: ent(**args, rendered_depth=rd, prior_inputs=pin, plan=plan, out=out), 1, iters, warmup),
                                       "c_entry_graph": _time(_graph(lambda: ent(**args, rendered_depth=rd, prior_inputs=pin, plan=plan, out=out)), 1,
                                                              iters, warmup)}
        F = 4
        hp, ent, cur, args = _setup(K, "mlp", "bd", True, F, h, w, P=1, D=96)
        rd = torch.full((F, 1, h // 2, w // 2), 2.0, device="cuda")
        fc = {"world_T_cam_b44": cur["world_T_cam_b44"].contiguous(), "cam_T_world_b44": cur["cam_T_world_b44"].contiguous(),
              "K_s0_b44": cur["K_s0_b44"].contiguous(), "invK_s0_b44": cur["invK_s0_b44"].contiguous(),
              "prior_prediction": torch.rand(1, 1, h // 2, w // 2, device="cuda"), "prior_cam_T_world": torch.eye(4, device="cuda")[None].contiguous()}
        plan = ent.prepare(F, K, 16, h // 4, w // 4, 1, prior_mode=m.PRIOR_CHAIN)
        out = ent(**args, rendered_depth=rd, frame_chain=fc, plan=plan)
        res["b_temporal_d96_chain4"] = {"hotpath": _time(lambda: hp(**args, rendered_depth=rd, frame_chain=fc), F, iters, warmup),
                                        "c_entry": _time(lambda: ent(**args, rendered_depth=rd, frame_chain=fc, plan=plan, out=out), F, iters, warmup),
                                        "c_entry_graph": _time(_graph(lambda: ent(**args, rendered_depth=rd, frame_chain=fc, plan=plan, out=out)), F,
                                                               iters, warmup)}
    res["device"] = torch.cuda.get_device_name(0)
    res["iters"], res["warmup"] = iters, warmup
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = run(a.iters, a.warmup)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
