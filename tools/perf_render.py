"""Times the shaded mesh render (csrc/raster_shade.hip) against the depth-only render (csrc/raster.hip) on the scenes of
tools/perf_raster.py, and one whole ``StreamingSession.composite_asset`` call:

  plane       the 1024 x 1024-vertex query plane (2 093 058 triangles), camera turned 0.05 rad from the plane's own
  plane_turn  the same plane after a 1.2 rad turn: part of it is behind the camera, the faces on the z = 0 line are queued
  scan        the synthetic scan-sized room of perf_raster.scan_mesh seen from inside (~1.0 M triangles)

each at 192 x 256 and at 480 x 640, one camera.  "depth_ms": ``raster.render_depth``; "shaded_ms": ``raster.render_shaded`` with depth +
rgba + pix_to_face (random vertex colours); "ratio" = shaded / depth: the price of the 64-bit key (twice the z-buffer bytes, a 64-bit
atomic minimum in place of a 32-bit one) plus the shade pass.  "all_outputs_ms" adds barycentrics and 3 attribute channels.

"composite_asset": a 20 x 20-cell coloured asset in a 96 x 128 session of the tests' small model (tests/test_ray_query_gpu.py), on a frame
between keyframes: "call_ms" is the whole call - two renders, the view query, the blend - and "parts_ms" the same three steps timed
alone.

All figures are HIP-event times per call over --iters back-to-back calls after --warmup: each call holds allocations, a ctypes call and
five kernel launches, so at tens of microseconds they are bounded below by the host's launch rate (an upper bound on device time, as in
perf_raster.py).  "repeat_spread": (max - min) / min of --repeats such measurements of the depth-only ``scan`` render, the run-to-run
spread ratios on this card should be read against.  Prints one JSON line; --out also writes it.

    python tools/perf_render.py --iters 50 --warmup 10 --out profiles/raster/render.json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_render.py measures on the GPU; none is visible")
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import AssetRenderer, compositing, raster
    from perf_raster import _ms, scan_mesh

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    plane_v = raster.plane_vertices(torch.eye(4, device=dev)[None], torch.tensor(2.0)).contiguous()
    plane_f = raster.plane_faces().to(dev).to(torch.int32)
    sv, sf = scan_mesh()
    sv, sf = sv.to(dev), sf.to(dev).to(torch.int32)
    meshes = {"plane": (plane_v, plane_f, 0.05), "plane_turn": (plane_v, plane_f, 1.2), "scan": (sv, sf, 0.05)}
    res = {"renders": {}}
    with torch.inference_mode():
        for name, (v, f, ry) in meshes.items():
            cam = torch.linalg.inv(syn._rot_y(ry)).float()[None].to(dev)
            col = torch.randint(0, 256, (v.shape[0], 4), dtype=torch.uint8, generator=g).to(dev)
            att = torch.randn(v.shape[0], 3, generator=g).to(dev)
            for H, W in ((192, 256), (480, 640)):
                K = syn.intrinsics(W, H).float()[None].to(dev)
                depth = lambda: raster.render_depth(v, f, cam, K, H, W)
                shaded = lambda: raster.render_shaded(v, f, cam, K, H, W, colors=col, return_faces=True)
                full = lambda: raster.render_shaded(v, f, cam, K, H, W, colors=col, attrs=att, return_faces=True, return_bary=True)
                assert torch.equal(shaded()["depth"], depth())
                d, s, u = (_ms(fn, a.iters, a.warmup) for fn in (depth, shaded, full))
                res["renders"][f"{name}_{H}x{W}"] = {"vertices": int(v.shape[0]), "faces": int(f.shape[0]), "covered": round(float((depth() > 0).float().mean()), 4),
                                                     "depth_ms": round(d, 4), "shaded_ms": round(s, 4), "ratio": round(s / d, 3), "all_outputs_ms": round(u, 4),
                                                     "key_plane_bytes": 8 * H * W}
        cam = torch.linalg.inv(syn._rot_y(0.05)).float()[None].to(dev)
        K = syn.intrinsics(256, 192).float()[None].to(dev)
        reps = [_ms(lambda: raster.render_depth(sv, sf, cam, K, 192, 256), a.iters, a.warmup) for _ in range(a.repeats)]
        res["repeat_spread"] = {"scan_192x256_depth_ms": [round(r, 4) for r in reps], "spread": round((max(reps) - min(reps)) / min(reps), 4)}

        # one whole composite_asset call on a frame between keyframes
        from implicit_depth_amd.streaming import StreamingSession
        from test_ray_query_gpu import BUFFER, IMG_H, IMG_W, _frame, _model

        poses, dists = syn.keyframe_trajectory("stream12", seed=0)
        session = StreamingSession(_model("mlp", 3), buffer_size=BUFFER)
        n = 20
        gx = np.linspace(-0.25, 0.25, n + 1)
        yy, xx = np.meshgrid(gx, gx, indexing="ij")
        verts = torch.from_numpy(np.stack([xx, yy, 0.08 * np.sin(7 * xx) * np.cos(5 * yy)], -1).reshape(-1, 3)).float()
        colors = torch.randint(0, 256, (len(verts), 4), dtype=torch.uint8, generator=g)
        asset = AssetRenderer(verts, torch.from_numpy(syn._grid_faces(n, n)), colors)
        Kimg = syn.intrinsics(IMG_W, IMG_H).float().to(dev)
        image = torch.randint(0, 256, (1, IMG_H, IMG_W, 3), dtype=torch.uint8, generator=g).to(dev)
        live = None
        for t in range(9):
            out, code = session.step(_frame(t, poses), world_T_cam=poses[t], dist_to_last_valid=dists[t])
            if out is None and session._key is not None:
                live = poses[t]
                break
        if live is None:
            raise SystemExit("the sequence has no frame between keyframes")
        call = lambda: session.composite_asset(image, asset, live, Kimg)
        parts = session.composite_asset(image, asset, live, Kimg, return_parts=True)
        h, w = compositing.MODEL_SIZE
        Kq = Kimg[None].clone()
        Kq[:, 0] *= w / IMG_W
        Kq[:, 1] *= h / IMG_H
        invKq = torch.linalg.inv(Kq)
        steps = {"two_renders": lambda: (asset.render(live, Kq, (h, w)), asset.render(live, Kimg, (IMG_H, IMG_W))),
                 "occlusion_for_view": lambda: session.occlusion_for_view(parts["asset_depth"], live, invKq, fill=-20.0),
                 "composite_mask": lambda: compositing.composite_mask(image, parts["view_pred"], virtual_rgba=parts["asset_rgba"])}
        res["composite_asset"] = {"image": [IMG_H, IMG_W], "query_size": [h, w], "asset_faces": 2 * n * n, "call_ms": round(_ms(call, a.iters, a.warmup), 4),
                                  "parts_ms": {k: round(_ms(fn, a.iters, a.warmup), 4) for k, fn in steps.items()},
                                  "asset_pixels": round(float((parts["asset_rgba"][..., 3] > 0).float().mean()), 4)}
    res["shape"] = {"iters": a.iters, "warmup": a.warmup, "repeats": a.repeats}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
