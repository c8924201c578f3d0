"""Feature volume, dropping of views without a sample in the image (fv_mlp_k): per camera set, the share of (16-voxel tile,
plane, view) groups the kernel can drop - restated on the CPU - and the kernel's time with the dropping on and off.

  python tools/perf_fv_skip.py [B] [iters] [reps]

Camera sets, all at the benchmark's shape (B x 7 views, 16 channels, 96 x 128, 64 planes from 0.25 m to 5 m; features stay synthetic):
  bench      synthetic.cost_volume_inputs(seed 0): the cameras bench.py times
  identity   every source camera = the current camera: nothing can be dropped (the worst case of the dropping)
  tuple31    synthetic.frame_tuple(seed 31): the tuple tests/test_bdmodel_gpu.py feeds with the reference's BDModel goldens (g5 / g9)
  golden_g2  cost_volume_inputs with the dims of tests/golden/g2_full_k7d64.npz (the full-size feature-volume golden)
One JSON line per camera set: "on" = the default (each launch picks fv_mlp_k<KT, false> or <KT, true>), "off" = always <KT, false>, "always" = always
<KT, true>.  A library without the switch (FeatureVolumeManager.skip_empty_views) is timed once, as "on".

  IDH_LIB=<developer library> python tools/perf_fv_skip.py [B] --wave-clocks [cameras ...]

Load balance of the skipping kernel's task order (tools/fv_task_balance.py has the model): needs a library whose csrc/feature_volume.hip was
compiled with -DIDH_FV_WAVE_CLOCKS (every wave stores the 100 MHz wall clock at entry and exit and its HW_ID; in no shipped build), and
-DIDH_ABL_FV_STATIC_ORDER beside it for the static order the rotation replaced.  One launch of the kernel, forced, after three warm-up launches;
per camera set (default: bench) one JSON line: the kernel's span, the mean exit time per wave index relative to the mean over all waves, which
wave indices share a SIMD, and over the SIMDs (exit of a SIMD = exit of its last wave) busiest / mean and the mean idle tail before the kernel ends.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import implicit_depth_amd.synthetic as syn
from implicit_depth_amd import cost_volume as cv

K, C, H, W, D = 7, 16, 96, 128, 64
DMIN, DMAX = 0.25, 5.0


def plane_depths(D, dmin, dmax):
    ramp = torch.linspace(0, 1, D, dtype=torch.float64)
    return torch.exp(np.log(dmin) + np.log(dmax / dmin) * ramp)


def outside_share(src_Ks, src_extrinsics, cur_invK, H, W, depths):
    """(share of samples with four zero bilinear weights, share of (16 consecutive pixels, plane, view) groups in which all are), fp64: a sample
    has no weight when its x falls outside (-1, W) or its y outside (-1, H) after the -0.5 shift (z clamped to 1e-5), csrc/feature_volume.hip."""
    Ks, E, iK = src_Ks.double().cpu(), src_extrinsics.double().cpu(), cur_invK.double().cpu()
    B, Kv = Ks.shape[:2]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=torch.float64)])  # 3,N
    P = Ks @ E  # B,K,4,4
    q = P[:, :, :3, :3] @ iK[:, None, :3, :3] @ pix  # B,K,3,N
    cam = depths.view(1, 1, -1, 1, 1) * q[:, :, None] + P[:, :, None, :3, 3:4]  # B,K,D,3,N
    z = cam[..., 2, :].clamp_min(1e-5)
    sx, sy = cam[..., 0, :] / z - 0.5, cam[..., 1, :] / z - 0.5
    out = (sx <= -1) | (sx >= W) | (sy <= -1) | (sy >= H)  # B,K,D,N
    N = H * W
    pad = (-N) % 16
    tiles = torch.cat([out, out[..., -1:].expand(*out.shape[:-1], pad)], -1) if pad else out
    return out.double().mean().item(), tiles.reshape(*out.shape[:-1], -1, 16).all(-1).double().mean().item()


def camera_sets(B):
    base = syn.cost_volume_inputs(B, K, C, H, W, seed=0)
    sets = {"bench": base}
    ident = dict(base)
    eye = torch.eye(4).expand(B, K, 4, 4).contiguous()
    ident["src_extrinsics"], ident["src_poses"] = eye, eye.clone()
    sets["identity"] = ident
    cur, src = syn.frame_tuple(1, K, 4 * H, 4 * W, seed=31, P=3)
    t31 = dict(base)
    t31["src_extrinsics"] = (src["cam_T_world_b44"] @ cur["world_T_cam_b44"].unsqueeze(1)).expand(B, K, 4, 4).contiguous()
    t31["src_poses"] = (cur["cam_T_world_b44"].unsqueeze(1) @ src["world_T_cam_b44"]).expand(B, K, 4, 4).contiguous()
    t31["src_Ks"] = src["K_s1_b44"].expand(B, K, 4, 4).contiguous()
    t31["cur_invK"] = cur["invK_s1_b44"].expand(B, 4, 4).contiguous()
    sets["tuple31"] = t31
    g = np.load(os.path.join(ROOT, "tests", "golden", "g2_full_k7d64.npz"))
    gd = [int(v) for v in g["dims"]]
    gi = syn.cost_volume_inputs(1, gd[1], gd[2], gd[3], gd[4], gd[6], gd[7], gd[8])
    g2 = dict(base)
    for k in ("src_extrinsics", "src_poses", "src_Ks"):
        g2[k] = gi[k].expand(B, K, 4, 4).contiguous()
    g2["cur_invK"] = gi["cur_invK"].expand(B, 4, 4).contiguous()
    sets["golden_g2"] = g2
    return sets


def wave_clock_stats(clk):
    """clk: (workgroups, 8, 4) uint64 = [entry, exit, HW_ID, written] per wave (csrc/feature_volume.hip, IDH_FV_WAVE_CLOCKS); times in 10 ns ticks."""
    clk = clk[clk[:, :, 3].all(1)]  # workgroups that ran
    t0 = clk[:, :, 0].min()
    exit_t = (clk[:, :, 1] - t0).astype(np.float64)  # workgroups, 8
    hw = clk[:, :, 2].astype(np.int64)
    simd = (hw >> 4) & 3
    cu = ((hw >> 13) & 7) * 32 + ((hw >> 12) & 1) * 16 + ((hw >> 8) & 15)  # (SE, SH, CU: the XCD is not in HW_ID, a workgroup stays on one CU anyway)
    assert (cu == cu[:, :1]).all(), "a workgroup's waves on more than one CU"
    simd_exit, sharing = [], {}
    for b in range(clk.shape[0]):
        for s in range(4):
            ws = np.nonzero(simd[b] == s)[0]
            if len(ws):
                simd_exit.append(exit_t[b, ws].max())
                sharing["+".join(map(str, ws))] = sharing.get("+".join(map(str, ws)), 0) + 1
    simd_exit = np.array(simd_exit)
    end = exit_t.max()
    cu_exit = exit_t.max(1)
    in_cu = np.array([exit_t[b].max() - exit_t[b].min() for b in range(clk.shape[0])])
    return {"workgroups": int(clk.shape[0]), "kernel_span_us": round(end / 100, 1),
            "wave_index_exit_over_mean": [round(v, 4) for v in (exit_t.mean(0) / exit_t.mean()).tolist()],
            "wave_exit_first_mean_last_us": [round(exit_t.min() / 100, 1), round(exit_t.mean() / 100, 1), round(end / 100, 1)],
            "simd_exit_busiest_over_mean": round(simd_exit.max() / simd_exit.mean(), 4),
            "simd_idle_tail_mean_share": round(float((end - simd_exit).mean() / end), 4),
            "cu_exit_busiest_over_mean": round(cu_exit.max() / cu_exit.mean(), 4),
            "first_to_last_wave_within_cu_mean_us": round(in_cu.mean() / 100, 1),
            "waves_sharing_a_simd": dict(sorted(sharing.items(), key=lambda kv: -kv[1])[:8])}


def wave_clocks(B, names):
    from implicit_depth_amd import _lib

    L = _lib.lib()
    try:
        fn = L.idh_dev_fv_wave_clocks
    except AttributeError:
        raise SystemExit("--wave-clocks needs a library built with -DIDH_FV_WAVE_CLOCKS (IDH_LIB=...), see the top of this file")
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]
    dev = torch.device("cuda:0")
    m = cv.FeatureVolumeManager(H, W, D, num_source_views=K).to(dev)
    syn.fill_state_dict(m.mlp, 99, gain=1.4)
    m.skip_empty_views = "always"
    vol = torch.empty(B, H, W, D, device=dev)
    sets = camera_sets(B)
    for name in names or ["bench"]:
        d = {k: v.to(dev) for k, v in sets[name].items()}
        cur_n, src_n = cv.to_nhwc(d["cur_feats"]), cv.to_nhwc(d["src_feats"])
        st = {}
        for _ in range(4):
            m._run(cur_n.data_ptr(), src_n.data_ptr(), (B, K, C, H, W), d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"], DMIN, DMAX,
                   vol.data_ptr(), D, False, dev, scratch=st)
        torch.cuda.synchronize()
        clk = np.zeros((256, 8, 4), dtype=np.uint64)
        _lib.check(fn(clk.ctypes.data, 256), "idh_dev_fv_wave_clocks")
        print(json.dumps({"cameras": name, "B": B, **wave_clock_stats(clk)}), flush=True)


def main():
    if "--wave-clocks" in sys.argv:
        i = sys.argv.index("--wave-clocks")
        return wave_clocks(int(sys.argv[1]) if i > 1 else 32, sys.argv[i + 1:])
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    dev = torch.device("cuda:0")
    m = cv.FeatureVolumeManager(H, W, D, num_source_views=K).to(dev)
    syn.fill_state_dict(m.mlp, 99, gain=1.4)
    has_switch = "skip_empty_views" in m.__dict__
    depths = plane_depths(D, DMIN, DMAX)
    vol = torch.empty(B, H, W, D, device=dev)
    for name, inp in camera_sets(B).items():
        # the share on batch element 0 and the last one (the batch elements differ by a small translation only)
        sel = [0, B - 1]
        samp, grp = outside_share(inp["src_Ks"][sel], inp["src_extrinsics"][sel], inp["cur_invK"][sel], H, W, depths)
        d = {k: v.to(dev) for k, v in inp.items()}
        cur_n, src_n = cv.to_nhwc(d["cur_feats"]), cv.to_nhwc(d["src_feats"])
        st = {}

        def step():
            m._run(cur_n.data_ptr(), src_n.data_ptr(), (B, K, C, H, W), d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"], DMIN, DMAX,
                   vol.data_ptr(), D, False, dev, scratch=st)

        res = {"cameras": name, "B": B, "outside_samples": round(samp, 4), "outside_groups": round(grp, 4)}
        for mode in (("on", "off", "always") if has_switch else ("on",)):
            if has_switch:
                m.skip_empty_views = {"on": True, "off": False, "always": "always"}[mode]
            times = []
            for _ in range(reps):
                for _ in range(3):
                    step()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    step()
                e1.record()
                torch.cuda.synchronize()
                times.append(round(e0.elapsed_time(e1) / iters, 4))
            res[f"ms_{mode}"] = times
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
