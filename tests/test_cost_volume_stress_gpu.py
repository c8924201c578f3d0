"""Randomised geometry stress of the LDS-window kernel against the quad kernel (same arithmetic up to summation
order): random rotations up to ~1 rad about random axes, translations up to 2 m in any direction (views beside,
behind and inside the swept volume), random focal lengths / principal points, depth ranges and map sizes.  Guards the
window kernel's table logic — run skipping, window placement, per-lane global fall-back — where a wrong decision
would silently drop or corrupt samples.

Every launch here is small enough (B <= 3, maps below 70 x 150) that the launcher gives each workgroup ONE 4-plane unit: the run tree is
walked for 4-plane and single-plane nodes only.  The longer runs (8 and 16 planes sharing a window), several super-groups per workgroup, the
super-group flush and the in-kernel arg-max over several units run on the same geometry families under a forced plane split in
tests/test_cost_volume_split_gpu.py."""
import numpy as np
import pytest
import torch

import volume_geometry as vg

pytestmark = pytest.mark.gpu


def _case(rng, B, K, H, W):
    return {k: v.cuda() for k, v in vg.random_geometry(rng, B, K, H, W).items()}


@pytest.mark.parametrize("seed", range(6))
def test_window_kernel_equals_quad_kernel_on_random_geometry(seed):
    from implicit_depth_amd import _lib
    from implicit_depth_amd.cost_volume import CostVolumeManager

    rng = np.random.default_rng(1000 + seed)
    worst = 0.0
    for _ in range(12):
        B = int(rng.integers(1, 4))
        K = int(rng.integers(1, 9))
        H = int(rng.integers(12, 70))
        W = int(rng.integers(48, 150))
        D = int(rng.integers(1, 70))
        g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
        inp = _case(rng, B, K, H, W)
        inp["cur_feats"] = torch.randn(B, 16, H, W, generator=g).cuda()
        inp["src_feats"] = torch.randn(B, K, 16, H, W, generator=g).cuda()
        lo = float(rng.uniform(0.1, 1.0))
        inp["min_depth"], inp["max_depth"] = lo, lo * float(rng.uniform(2.0, 40.0))
        m = CostVolumeManager(H, W, D).cuda()
        m.kernel = _lib.CV_KERNEL_QUAD
        ref, rlow, _, _ = m(**inp)
        m.kernel = _lib.CV_KERNEL_WINDOW
        got, glow, _, _ = m(**inp)
        assert bool(torch.isfinite(got).all())
        scale = float(ref.abs().max().clamp_min(1e-6))
        err = float((got - ref).abs().max()) / scale
        worst = max(worst, err)
        assert err < 5e-6, (seed, B, K, H, W, D, err)
        assert float(((glow - rlow).abs() > 1e-5).float().mean()) < 5e-3
    assert worst < 5e-6


def _err_stats(got, ref64):
    """scale-relative error statistics of a HIP volume against the fp64 oracle.  In this geometry single samples sit exactly on an
    image border or on the z = 1e-5 clamp, where fp32 and fp64 projections legitimately pick different taps (|u| reaches 1e5 px behind
    the camera), so the bar is statistical: a logic error (dropped run, misplaced window, wrong fall-back) corrupts whole planes or tiles."""
    scale = float(ref64.abs().max().clamp_min(1e-6))
    e = (got.double().cpu() - ref64).abs().flatten() / scale
    return {"max": float(e.max()), "p999": float(torch.quantile(e[:: max(1, e.numel() // 2_000_000)], 0.999)), "mean": float(e.mean()),
            "frac_gt_1e-3": float((e > 1e-3).double().mean())}


def check_vs_fp64(got, glow, ref, rlow, tag):
    """the statistical bars of one HIP volume (and its arg-max plane) against the fp64 oracle's -> the error statistics.  One statement of the
    bars: the all-kernel check below and tests/test_cost_volume_split_gpu.py (the same geometries under a forced plane split) both call it."""
    assert bool(torch.isfinite(got).all()), tag
    st = _err_stats(got, ref)
    assert st["p999"] < 2e-4 and st["mean"] < 2e-5 and st["frac_gt_1e-3"] < 5e-4, (tag, st)
    assert float(((glow.double().cpu() - rlow).abs() > 1e-5).double().mean()) < 2e-2, (tag, "arg-max plane")
    return st


def _check_all_kernels_vs_fp64(inp, H, W, D, tag):
    from implicit_depth_amd import _lib
    from implicit_depth_amd.cost_volume import CostVolumeManager
    from oracle import cost_volume as ocv

    cpu64 = {k: (v.double().cpu() if torch.is_tensor(v) else v) for k, v in inp.items()}
    ref, rlow, _ = ocv.cost_volume_dot(cpu64["cur_feats"], cpu64["src_feats"], cpu64["src_extrinsics"], cpu64["src_Ks"], cpu64["cur_invK"],
                                       inp["min_depth"], inp["max_depth"], D)
    out = {}
    for name, code in (("quad", _lib.CV_KERNEL_QUAD), ("window", _lib.CV_KERNEL_WINDOW), ("lane", _lib.CV_KERNEL_LANE)):
        m = CostVolumeManager(H, W, D).cuda()
        m.kernel = code
        got, glow, _, _ = m(**inp)
        out[name] = check_vs_fp64(got, glow, ref, rlow, (tag, name))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_every_kernel_vs_fp64_oracle_on_random_geometry(seed):
    """the same random geometries, each of the three kernels against the INDEPENDENT fp64 restatement (oracle/cost_volume.py: explicit
    homography, hand-rolled gather) — the window-vs-quad comparison above shares the projection code, so a common-mode error would pass it"""
    rng = np.random.default_rng(1000 + seed)  # the seeds (and so the first cases) of the HIP-vs-HIP test
    for case in range(8):  # (8 of its 12 geometries per seed: the fp64 oracle on the host is what this test costs - 48 geometries in ~100 s)
        B, K = int(rng.integers(1, 4)), int(rng.integers(1, 9))
        H, W, D = int(rng.integers(12, 70)), int(rng.integers(48, 150)), int(rng.integers(1, 70))
        g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
        inp = _case(rng, B, K, H, W)
        inp["cur_feats"] = torch.randn(B, 16, H, W, generator=g).cuda()
        inp["src_feats"] = torch.randn(B, K, 16, H, W, generator=g).cuda()
        lo = float(rng.uniform(0.1, 1.0))
        inp["min_depth"], inp["max_depth"] = lo, lo * float(rng.uniform(2.0, 40.0))
        _check_all_kernels_vs_fp64(inp, H, W, D, (seed, case, B, K, H, W, D))


@pytest.mark.parametrize("seed", range(12))
def test_source_camera_plane_cuts_through_tiles(seed):
    """z crosses 0 INSIDE a tile: the source camera looks across the swept volume (rotation of 70..110 degrees about the x or y axis) and is
    placed so that its z = 0 plane passes through the centre of the current frustum at the geometric-mean depth — every 32 x 8 tile near
    the crossing holds samples in front of the camera, behind it and on the 1e-5 clamp (geometry_utils.py:86, cost_volume.py:216-217)."""
    rng = np.random.default_rng(7000 + seed)
    B, K = 1 + seed % 2, int(rng.integers(2, 8))
    H, W, D = int(rng.integers(24, 72)), int(rng.integers(64, 150)), int(rng.integers(8, 64))
    inp = _case(rng, B, K, H, W)
    lo = float(rng.uniform(0.2, 1.0))
    hi = lo * float(rng.uniform(3.0, 20.0))
    inp = {k: v.cuda() for k, v in vg.cross_source_plane(rng, {k: v.cpu() for k, v in inp.items()}, H, W, lo, hi).items()}
    g = torch.Generator().manual_seed(seed)
    inp["cur_feats"] = torch.randn(B, 16, H, W, generator=g).cuda()
    inp["src_feats"] = torch.randn(B, K, 16, H, W, generator=g).cuda()
    inp["min_depth"], inp["max_depth"] = lo, hi
    _check_all_kernels_vs_fp64(inp, H, W, D, ("z-cross", seed, B, K, H, W, D))


# (B, K, H, W, D) of the four seeds below: maps of at least 48 x 12 (the window kernel's smallest), odd sizes, one and several tiles per row
GEOMETRY_SHAPES = [(2, 3, 14, 50, 9), (3, 8, 20, 67, 21), (2, 5, 14, 50, 9), (3, 7, 20, 67, 21)]
GEOMETRY_FAMILIES = ("intrinsics", "roll_pitch")


def geometry_case(family, seed):
    """CPU inputs of one case of the test below (tests/test_volume_geometry_cpu.py checks the same cases against the mutations)"""
    B, K, H, W, D = GEOMETRY_SHAPES[seed]
    return vg.build_case(family, 100 + seed, B, K, 16, H, W)


@pytest.mark.parametrize("family", GEOMETRY_FAMILIES)
@pytest.mark.parametrize("seed", range(4))
def test_every_kernel_vs_fp64_oracle_per_view_intrinsics_and_roll_pitch(seed, family):
    """``intrinsics``: another K for every (b, k) and another current-frame K for every b - the cases above repeat one matrix, so that the
    indexing src_K + (b * K + k) * 16 / cur_invK + b * 16 of the four build_homography call sites never mattered; ``roll_pitch``: rolls of 30
    and 90 degrees and pitches of 20 degrees, a large column 1 of every homography.  Lane, quad and window kernel, the bars of the cases above.  (The eight cases: 1.0 s on the MI355X host.)"""
    B, K, H, W, D = GEOMETRY_SHAPES[seed]
    inp = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in geometry_case(family, seed).items()}
    _check_all_kernels_vs_fp64(inp, H, W, D, (family, seed, B, K, H, W, D))
