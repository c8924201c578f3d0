"""Times a B = 1 live sequence per predicting frame: ``StreamingSession.step`` (matching encoder on the current image only, source
features from the keyframe bank) against ``fused_forward(native_matching_stem=True)`` on the SAME tuples (matching encoder on all K + 1
images of every frame), at the BASELINE size: 512 x 384 images, 96 x 128 matching maps, K = 7 MLP feature volume, D = 64, 8 query planes,
synthetic weights, the stand-in image encoder on both sides.

Sequence: a camera orbiting a point 1.5 m away at 0.02 rad a frame with the keyframe distance lowered to 0.03, so that every frame is a
keyframe and, once K keyframes are stored, every frame predicts; buffer of 30.  The session runs first and records each frame's tuple; the
reference side gets its ``src_data`` dictionaries prebuilt (stacking the K images is not charged to it).

"session_ms" / "fused_forward_ms": HIP-event time over all predicting frames of one pass, divided by their number; --reps passes of each,
alternating, after one untimed pass of each; the median, with the minimum and maximum beside it.  Host work of a step (keyframe decision,
ctypes calls, launches) is inside the window: at B = 1 it is part of what a caller waits for.  "gather_ms": ``FeatureBank.gather`` alone
(one launch, ``bytes`` moved computed from shapes); "matching_encoder_ms": the native matching encoder alone on 1 image and on the K + 1
images of a tuple (events over 200 back-to-back calls each); "host_selection_ms": ``try_new_keyframe`` + ``get_best_measurement_frames``
per frame on the host's clock, no GPU involved.  Also checks that both sides give the same ``pred_0`` (scale-relative) on the last frame.
Prints one JSON line; --out also writes it.

    python tools/perf_streaming.py --frames 47 --reps 5 --out profiles/streaming/run.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class _RunOpts:
    matching_scale, min_matching_depth, max_matching_depth, use_prior = 1, 0.25, 5.0, False


class _Config:
    test_keyframe_buffer_size, test_keyframe_pose_distance, test_optimal_t_measure, test_optimal_R_measure = 30, 0.03, 0.15, 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=47)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--views", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_streaming.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from hot_helpers import holder
    from implicit_depth_amd import backbone
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.dropin import fused_forward
    from implicit_depth_amd.streaming import StreamingSession

    Hi, Wi, K, T = a.height, a.width, a.views, a.frames
    m = holder(K, "mlp", Hi // 4, Wi // 4, a.planes, with_head=False)
    m.matching_model = net.ResnetMatchingEncoder(backbone.resnet18_stem(), 16)
    m.encoder = syn.StubImageEncoder()
    m.run_opts, m.thresholder = _RunOpts(), None
    syn.fill_state_dict(m, seed=30)
    m = m.cuda().eval()

    back = np.eye(4)
    back[2, 3] = -1.5
    poses = [syn._rot_y(0.02 * t).numpy() @ back for t in range(T)]
    K1, K0 = syn.intrinsics(Wi // 4, Hi // 4).float(), syn.intrinsics(Wi // 2, Hi // 2).float()
    frames = []
    for t in range(T):
        w = torch.from_numpy(poses[t]).float()
        d = {"image_b3hw": syn.randn((1, 3, Hi, Wi), 700 + t, "img"), "K_s1_b44": K1[None], "invK_s1_b44": torch.linalg.inv(K1)[None],
             "K_s0_b44": K0[None], "invK_s0_b44": torch.linalg.inv(K0)[None], "world_T_cam_b44": w[None], "cam_T_world_b44": torch.linalg.inv(w)[None],
             "rendered_depth": syn.rendered_depth_planes(1, Hi // 2, Wi // 2, 8)}
        frames.append({k: v.cuda().contiguous() for k, v in d.items()})

    session = StreamingSession(m, buffer_size=_Config.test_keyframe_buffer_size, config=_Config)
    reference = fused_forward(m, native_matching_stem=True)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def session_pass():
        """(ms per predicting frame, tuples, last outputs) of one pass over the sequence."""
        session.reset()
        tuples, out, started, s, e = {}, None, False, ev(), ev()
        for t in range(T):
            if t == K:  # from here on every frame predicts
                torch.cuda.synchronize()
                s.record()
                started = True
            o, code = session.step(frames[t], world_T_cam=poses[t])
            assert (o is not None) == started and code == (0 if t == 0 else 1), (t, code)
            if o is not None:
                tuples[t], out = session.last_indices, o
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / (T - K), tuples, out

    _, tuples, out_s = session_pass()  # untimed: builds the plans, records the tuples
    keys = ("image_b3hw", "K_s1_b44", "invK_s1_b44", "world_T_cam_b44", "cam_T_world_b44")
    srcs = {t: {k: torch.stack([frames[i][k][0] for i in idx])[None].contiguous() for k in keys} for t, idx in tuples.items()}

    def reference_pass():
        out, s, e = None, ev(), ev()
        torch.cuda.synchronize()
        s.record()
        for t in range(K, T):
            out = reference("test", frames[t], srcs[t])
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / (T - K), out

    _, out_r = reference_pass()  # untimed
    diff = ((out_s["pred_0"].double() - out_r["pred_0"].double()).abs().max() / out_r["pred_0"].double().abs().max()).item()
    ses, ref = [], []
    for _ in range(a.reps):
        ses.append(session_pass()[0])
        ref.append(reference_pass()[0])

    bank = session.bank
    cw, cc = frames[-1]["world_T_cam_b44"], frames[-1]["cam_T_world_b44"]
    slots = [list(session.last_slots)]
    for _ in range(20):
        bank.gather(slots, cw, cc)
    torch.cuda.synchronize()
    s, e, n = ev(), ev(), 500
    s.record()
    for _ in range(n):
        bank.gather(slots, cw, cc)
    e.record()
    torch.cuda.synchronize()
    gather_ms = s.elapsed_time(e) / n
    nbytes = 2 * K * bank.H * bank.W * bank.C * 4

    # where the difference comes from: the matching encoder on 1 image and on the K + 1 of a tuple (events over back-to-back calls), and
    # the host's share of a step: the keyframe decision and selection alone, on this host's clock
    from implicit_depth_amd import keyframes
    from implicit_depth_amd.nhwc import matching_encoder_forward

    def encoder_ms(images, n=200):
        for _ in range(10):
            matching_encoder_forward(m.matching_model, images, channels_last=True)
        torch.cuda.synchronize()
        s, e = ev(), ev()
        s.record()
        for _ in range(n):
            matching_encoder_forward(m.matching_model, images, channels_last=True)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n

    with torch.inference_mode():
        enc1 = encoder_ms(frames[-1]["image_b3hw"])
        enc8 = encoder_ms(torch.cat([frames[-1]["image_b3hw"], srcs[T - 1]["image_b3hw"][0]], 0).contiguous())
    import time

    buf = keyframes.KeyframeBuffer.from_config(_Config)
    t0 = time.perf_counter()
    for t in range(T):
        if buf.try_new_keyframe(poses[t], None, index=t) == 1 and len(buf) > K:
            buf.get_best_measurement_frames(K)
    host_ms = (time.perf_counter() - t0) * 1e3 / T

    stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    res = {"session_ms": stat(ses), "fused_forward_ms": stat(ref), "speedup_median": round(statistics.median(ref) / statistics.median(ses), 4),
           "pred_0_scale_rel_diff_last_frame": diff, "gather_ms": round(gather_ms, 5), "gather_bytes": nbytes,
           "gather_gb_per_s": round(nbytes / (gather_ms * 1e-3) / 1e9, 1),
           "matching_encoder_ms": {"1_image": round(enc1, 4), f"{K + 1}_images": round(enc8, 4)}, "host_selection_ms": round(host_ms, 4),
           "shape": {"image": [Hi, Wi], "K": K, "D": a.planes, "query_planes": 8, "frames": T, "predicting_frames": T - K, "reps": a.reps,
                     "buffer_size": _Config.test_keyframe_buffer_size, "matching_channels": bank.C},
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
