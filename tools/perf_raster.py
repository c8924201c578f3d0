"""Times the temporal evaluation's native passes (csrc/raster.hip) at the reference's shape — 192 x 256, one camera — against the one-frame
model forward measured in the same run on the same card (bench.TemporalWorkload, BASELINE config 5):

  plane      MeshDepthRasterizer render of the 1024 x 1024-vertex query plane (2 093 058 triangles), camera turned 0.05 rad from the
             plane's own: nothing is queued
  plane_turn the same plane seen after a 1.2 rad turn: part of the plane is behind the camera, the faces on the z = 0 line are queued
  scan       render of a synthetic scan-sized mesh seen from INSIDE it, as a scan is: a closed 6 x 3 x 5 m room of ~1.0 M noisy 1.6 cm
             triangles (the z = 0 plane through the camera cuts floor, ceiling and two walls: thousands of faces straddle it), a
             10 x 10-cell table top half a metre away (boxes of hundreds of pixels) and two panels that fill a quarter of the image
  vertices   update of the per-vertex predictions over 5 x 10^5 vertices (without its render, which is `scan`)
  flips      the flip count over a (30, 5 x 10^5) history

For each render the script counts, by the kernel's own rule (box of more than 64 pixel centres, or corners on both sides of z = 0), how
many faces the face pass queues for raster_large_k ("queued_large", "queued_straddling", "largest_box").

"event_ms": HIP-event time per call over --iters back-to-back calls after --warmup.  A call is two allocations, a ctypes call and five
kernel launches, so at tens of microseconds this is bounded below by the host's launch rate: an upper bound on device time, not a kernel
time.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (profiles/raster/README.md).
"interleaved_event_ms": the same call timed alone between two model forwards, which push the mesh out of the last-level cache.
"bytes" is what each pass must move, computed from shapes.  There is no parent or reference time for these passes (the reference's need
pytorch3d); the yardstick is `(plane + scan + vertices) / model forward`.  Prints one JSON line; --out also writes it.

    python tools/perf_raster.py --iters 50 --warmup 10 --out profiles/raster/run.json
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


def _wall(o, eu, ev, nu, nv, rng, noise=0.005):
    """(nu x nv)-cell wall o + s eu + t ev with normal-direction noise; returns verts, faces (local indices)."""
    import implicit_depth_amd.synthetic as syn

    t, s = np.meshgrid(np.linspace(0, 1, nv + 1), np.linspace(0, 1, nu + 1), indexing="ij")
    o, eu, ev = (np.asarray(a, np.float64) for a in (o, eu, ev))
    nrm = np.cross(eu, ev)
    nrm /= np.linalg.norm(nrm)
    p = o + s[..., None] * eu + t[..., None] * ev + noise * rng.standard_normal(s.shape)[..., None] * nrm
    return p.reshape(-1, 3), syn._grid_faces(nv, nu)


def scan_mesh(cell=0.0159, seed=0):
    """The room seen from inside (module docstring): verts (V,3) float32, faces (F,3) int64.  The camera sits at the origin."""
    rng = np.random.default_rng(seed)
    X, Y, Z0, Z1 = 3.0, 1.5, -2.5, 2.5
    n = lambda length: max(1, int(round(length / cell)))
    walls = [([-X, -Y, Z0], [2 * X, 0, 0], [0, 0, Z1 - Z0]), ([-X, Y, Z0], [2 * X, 0, 0], [0, 0, Z1 - Z0]),   # ceiling / floor (y down)
             ([-X, -Y, Z0], [0, 2 * Y, 0], [0, 0, Z1 - Z0]), ([X, -Y, Z0], [0, 2 * Y, 0], [0, 0, Z1 - Z0]),   # side walls
             ([-X, -Y, Z1], [2 * X, 0, 0], [0, 2 * Y, 0]), ([-X, -Y, Z0], [2 * X, 0, 0], [0, 2 * Y, 0])]     # front / back
    parts = [_wall(o, eu, ev, n(np.linalg.norm(eu)), n(np.linalg.norm(ev)), rng) for o, eu, ev in walls]
    parts.append(_wall([-0.3, 0.1, 0.35], [0.6, 0, 0.05], [0, 0.08, 0.5], 10, 10, rng, noise=0.0))            # table top
    parts.append(_wall([-0.45, -0.3, 0.4], [0.35, 0.0, 0.1], [0.0, 0.3, 0.0], 1, 1, rng, noise=0.0))          # near panel
    verts, faces, base = [], [], 0
    for v, f in parts:
        verts.append(v)
        faces.append(f + base)
        base += len(v)
    return torch.from_numpy(np.concatenate(verts).astype(np.float32)), torch.from_numpy(np.concatenate(faces))


def queued_faces(verts, faces, cam_T_world, K, H, W):
    """What raster_face_k queues, counted with torch by the kernel's rule (fp32, so a face within rounding of a limit may differ)."""
    T, Km = cam_T_world[0], K[0]
    p = verts @ T[:3, :3].T + T[:3, 3]
    tri = p[faces]  # (F,3,3)
    z = tri[..., 2]
    front = (z > 0).sum(1)
    straddle = (front > 0) & (front < 3)
    u = Km[0, 0] * tri[..., 0] / z + Km[0, 2]
    v = Km[1, 1] * tri[..., 1] / z + Km[1, 2]
    x0 = torch.ceil(u.amin(1) - 0.5 - 1 / 64).clamp(0, W)
    x1 = torch.floor(u.amax(1) - 0.5 + 1 / 64).clamp(-1, W - 1)
    y0 = torch.ceil(v.amin(1) - 0.5 - 1 / 64).clamp(0, H)
    y1 = torch.floor(v.amax(1) - 0.5 + 1 / 64).clamp(-1, H - 1)
    box = ((x1 - x0 + 1).clamp_min(0) * (y1 - y0 + 1).clamp_min(0))[front == 3]
    return {"faces": int(faces.shape[0]), "on_screen": int((box > 0).sum()), "queued_large": int((box > 64).sum()),
            "queued_straddling": int(straddle.sum()), "largest_box": int(box.max()) if box.numel() else 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_raster.py measures on the GPU; none is visible")
    import bench
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import raster

    dev = torch.device("cuda:0")
    H, W = 192, 256
    K = syn.intrinsics(W, H).float()[None].to(dev)
    cam = torch.linalg.inv(syn._rot_y(0.05)).float()[None].to(dev)
    cam_turn = torch.linalg.inv(syn._rot_y(1.2)).float()[None].to(dev)
    r = raster.MeshDepthRasterizer(H, W)
    r.create_plane_from_camera(torch.eye(4, device=dev)[None], distance=torch.tensor(2.0))
    sv, sf = scan_mesh()
    r.load_gt_mesh(verts=sv, faces=sf, device=dev)
    nv = 500000
    tv = r.gt_mesh[0][:nv].contiguous()
    pred = torch.rand(1, 1, H, W, device=dev)
    vis = r.render_depth(cam, K, mesh=r.gt_mesh)
    hist = syn.vertex_histories(30, nv, 1).to(dev)
    out = torch.empty(1, dtype=torch.int64, device=dev)
    from implicit_depth_amd import _lib

    wl = bench.TemporalWorkload(argparse.Namespace(batch=1, sequences=1, views=7, planes=96, height=384, width=512, volume="mlp", conv_math="fp32", mlp_math="fp32"), dev, 0)
    res = {}
    Vp, Fp = r.mesh[0].shape[0], r.mesh[1].shape[0]
    Vs, Fs = sv.shape[0], sf.shape[0]
    mesh_bytes = lambda V, F: V * 12 + F * 12 + 2 * V * 24
    passes = {
        "plane": (lambda: r(cam, K), mesh_bytes(Vp, Fp), (r.mesh, cam)),
        "plane_turn": (lambda: r(cam_turn, K), mesh_bytes(Vp, Fp), (r.mesh, cam_turn)),
        "scan": (lambda: r.render_depth(cam, K, mesh=r.gt_mesh), mesh_bytes(Vs, Fs), (r.gt_mesh, cam)),
        "vertices": (lambda: raster.vertex_predictions(tv, cam, K, pred, vis), nv * 16, None),
        "flips": (lambda: _lib.check(_lib.lib().idh_vertex_occlusion_changes_fwd(hist.data_ptr(), 30, nv, out.data_ptr(), _lib.stream_ptr()), "flips"), 30 * nv * 4, None),
    }
    with torch.inference_mode():
        for name, (fn, nbytes, mesh) in passes.items():
            res[name] = {"event_ms": round(_ms(fn, a.iters, a.warmup), 4), "bytes": nbytes}
            if mesh is not None:
                res[name].update(queued_faces(mesh[0][0], mesh[0][1], mesh[1], K, H, W))
        fwd = _ms(wl.step, a.iters, a.warmup)
        # each pass alone between model forwards: the forward's traffic evicts the mesh from the last-level cache
        for name, (fn, _, _) in passes.items():
            pairs = []
            for _ in range(a.iters):
                wl.step()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                pairs.append((e0, e1))
            torch.cuda.synchronize()
            res[name]["interleaved_event_ms"] = round(sum(x.elapsed_time(y) for x, y in pairs) / len(pairs), 4)
    res["model_forward_ms"] = round(fwd, 4)
    for key in ("event_ms", "interleaved_event_ms"):
        res["raster_over_forward_" + key] = round(sum(res[n][key] for n in ("plane", "scan", "vertices")) / fwd, 4)
    res["shape"] = {"H": H, "W": W, "vertices": nv, "T": 30, "iters": a.iters, "warmup": a.warmup}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
