"""The TSDF pose alignment without a GPU: the fp64 reference the GPU tests compare against (tests/tsdf_align_ref.py) -
its ambiguity masks, its Jacobian, its convergence on the committed scenes, the degenerate plane - and everything idh_tsdf_align_fwd and
the Python layer refuse, which is decided on the host before any launch."""
import ctypes

import numpy as np
import pytest

import tsdf_align_ref as AR
import tsdf_ref as R

ALL_ROW_CASES = [(*c, False) for c in AR.ROW_CASES] + [("room24x32", False, 1, False, 0.0, True), ("room30x44", True, 2, True, 0.01, True)]


def test_ambiguous_share_stays_under_the_cap():
    worst = 0.0
    for case in ALL_ROW_CASES:
        ref = AR.row_reference(*case)
        sel = int(ref["selected"].sum())
        share = ref["ambiguous"].sum() / sel
        worst = max(worst, share)
        assert share <= AR.CAP, (case, share)
        assert ref["valid"].sum() >= (6 if case[-1] else 0.3 * sel), (case, int(ref["valid"].sum()), sel)  # the cases test something
        assert not (ref["valid"] & ~ref["selected"]).any()
    # the issue's count: pixels within EPS_VOX of a cell face are at most 2 of 1320
    for name in ("room24x32", "room30x44"):
        ref = AR.row_reference(name, False, 1, False, 0.0)
        assert (ref["face"] < AR.EPS_VOX).sum() <= 2
    print("largest ambiguous share", worst)


def _moved(pose, xi):
    P = np.asarray(pose, np.float64).copy()
    P[:3, :3], P[:3, 3] = AR.update(P[:3, :3], P[:3, 3], np.asarray(xi, np.float64))
    return P


@pytest.mark.parametrize("name,box", [("room24x32", False), ("room30x44", True)])
def test_jacobian_is_the_derivative_of_the_residual(name, box):
    c = AR.row_inputs(name, box, False)
    args = (c["values"], c["origin"], c["voxel_size"], c["trunc_voxels"], c["depth"], c["invK"])
    pose = c["start"].astype(np.float64)
    base = AR.rows(*args, pose, exact_pose=True)
    use = base["valid"] & (base["face"] >= 0.05)
    assert use.sum() > 200
    step = 1e-6  # metres / radians: 2e-5 voxels, far inside the 0.05-voxel margin; r is a cubic polynomial of the increment within a cell
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = step
        hi, lo = AR.rows(*args, _moved(pose, xi), exact_pose=True), AR.rows(*args, _moved(pose, -xi), exact_pose=True)
        assert (hi["valid"] & lo["valid"])[use].all()
        fd = (hi["r"] - lo["r"])[use] / (2 * step)
        J = base["J"][..., k][use]
        assert np.abs(fd - J).max() <= 1e-7 * (1 + np.abs(J).max()), (k, np.abs(fd - J).max())


def _fit(name, pert, iters):
    c = AR.case(name, False)
    start = AR.perturb(c["pose"], *pert)
    out = AR.align(c["values"], c["origin"], c["voxel_size"], c["trunc_voxels"], c["depth"], c["invK"], start, iters=iters)
    return c, start, out


@pytest.mark.parametrize("name,pert,iters", [("room24x32", AR.PERTURBATION_A, 8), ("room24x32", AR.PERTURBATION_B, 8), ("room30x44", AR.PERTURBATION_A, 10)])
def test_reference_converges(name, pert, iters):
    c, start, out = _fit(name, pert, iters)
    assert out["statuses"] == [0] * iters
    t0, r0 = AR.pose_error(start, c["pose"])
    t1, r1 = AR.pose_error(out["world_T_cam"], c["pose"])
    print(name, "start", t0, np.degrees(r0), "end", t1, np.degrees(r1), "last step", out["steps"][-1], "ratios", out["ratios"].min())
    assert out["ratios"].min() >= 0.1  # well conditioned: min_pivot_ratio = 1e-6 is far away
    assert t1 < 2e-3 and np.degrees(r1) < 0.25  # millimetres and a fraction of a degree from 2.7 cm / 1 degree (5.8 cm / 2 degrees)
    if pert is AR.PERTURBATION_A:
        assert t1 <= t0 / 10 and r1 <= r0 / 4


def test_plane_is_degenerate():
    c = AR.plane_case()
    ref = AR.rows(c["values"], c["origin"], c["voxel_size"], c["trunc_voxels"], c["depth"], c["invK"], c["pose"])
    assert ref["valid"].sum() >= 64 and (ref["J"][..., 0] == 0).all() and (ref["J"][..., 2] != 0)[ref["valid"]].all()
    out = AR.align(c["values"], c["origin"], c["voxel_size"], c["trunc_voxels"], c["depth"], c["invK"], c["pose"], iters=3)
    assert out["statuses"] == [2, 3, 3] and out["ratios"][0] == 0.0
    assert np.array_equal(out["world_T_cam"], c["pose"].astype(np.float64))
    # and too few pixels is status 1
    holes = np.zeros_like(c["depth"])
    out = AR.align(c["values"], c["origin"], c["voxel_size"], c["trunc_voxels"], holes, c["invK"], c["pose"], iters=2)
    assert out["statuses"] == [1, 3]


EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4


def _library():
    import os

    from implicit_depth_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib, _lib.lib()


def _good_args(_lib, L, h=24, w=32, stride=1, iters=4):
    """Arguments that pass every check; the pointers are never dereferenced on the host."""
    a = _lib.TsdfAlignArgs()
    v = a.volume
    v.values, v.block_flags, v.block_flag_bytes = 0x10000, 0x20000, L.idh_tsdf_block_flag_bytes(20, 28, 36)
    v.voxel_size, v.trunc_voxels, v.Nz, v.Ny, v.Nx = 0.05, 3.0, 20, 28, 36
    a.depth_11hw, a.invK_44, a.world_T_cam_in_44, a.world_T_cam_out_44, a.records_i40 = 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
    a.workspace, a.workspace_bytes = 0x80000, L.idh_tsdf_align_workspace_bytes(h, w, stride, iters)
    a.damping, a.min_step, a.min_pivot_ratio, a.huber = 0.0, 0.0, 1e-6, 0.0
    a.h, a.w, a.iters, a.stride, a.min_count, a.max_workgroups = h, w, iters, stride, 64, 0
    return a


def test_workspace_bytes():
    _lib, L = _library()
    f = L.idh_tsdf_align_workspace_bytes
    assert f(24, 32, 1, 8) == 8 * (16 + 32 * 4) and f(30, 44, 1, 1) == 8 * (16 + 32 * 6) and f(30, 44, 3, 64) == 8 * (16 + 32)
    assert f(5, 7, 1, 1) == 8 * 48 and f(17, 16, 1, 1) == 8 * (16 + 64) and f(33, 33, 2, 1) == 8 * (16 + 32 * 4)
    for bad in ((0, 32, 1, 8), (24, 0, 1, 8), (24, 32, 0, 8), (24, 32, 1, 0), (24, 32, 1, 65), (65536, 32768, 1, 8), (-1, 32, 1, 8)):
        assert f(*bad) == 0, bad
    assert f(46340, 46340, 1, 1) > 0  # just below 2^31 pixels


def test_entry_point_refuses_on_the_host():
    _lib, L = _library()
    h = ctypes.CDLL(_lib.LIB_PATH)
    h.idh_sizeof_tsdf_align_args.restype = ctypes.c_size_t
    assert ctypes.sizeof(_lib.TsdfAlignArgs) == h.idh_sizeof_tsdf_align_args() == _lib.TsdfAlignArgs().struct_size
    assert "idh_tsdf_align_fwd" in _lib.declared_symbols() and "idh_tsdf_align_workspace_bytes" in _lib.declared_symbols()
    fwd = lambda a: L.idh_tsdf_align_fwd(ctypes.byref(a), None)
    assert L.idh_tsdf_align_fwd(None, None) == EINVAL
    nan, inf = float("nan"), float("inf")
    edits = [("struct_size", ctypes.sizeof(_lib.TsdfAlignArgs) - 1, EINVAL), ("h", 0, EINVAL), ("w", -3, EINVAL), ("iters", 0, EINVAL),
             ("iters", 65, EINVAL), ("stride", 0, EINVAL), ("min_count", 5, EINVAL), ("max_workgroups", -1, EINVAL), ("huber", nan, EINVAL),
             ("huber", inf, EINVAL), ("damping", -1e-3, EINVAL), ("damping", nan, EINVAL), ("damping", inf, EINVAL), ("min_step", -1.0, EINVAL),
             ("min_step", nan, EINVAL), ("min_step", inf, EINVAL), ("min_pivot_ratio", 1.0, EINVAL), ("min_pivot_ratio", -1e-9, EINVAL),
             ("min_pivot_ratio", nan, EINVAL), ("depth_11hw", None, EINVAL), ("invK_44", None, EINVAL), ("world_T_cam_in_44", None, EINVAL),
             ("world_T_cam_out_44", None, EINVAL), ("records_i40", None, EINVAL), ("workspace", 0x80004, EINVAL), ("rows_hw8", 0x90008, EINVAL),
             ("workspace", None, EWORKSPACE), ("workspace_bytes", 8 * (16 + 32 * 4) - 1, EWORKSPACE), ("workspace_bytes", -1, EWORKSPACE)]
    for field, value, code in edits:
        a = _good_args(_lib, L)
        setattr(a, field, value)
        assert fwd(a) == code, (field, value)
    vol_edits = [("struct_size", 8, EINVAL), ("Nx", 1, EINVAL), ("voxel_size", 0.0, EINVAL), ("trunc_voxels", inf, EINVAL), ("values", None, EINVAL),
                 ("block_flags", None, EWORKSPACE), ("block_flag_bytes", 1, EWORKSPACE)]
    for field, value, code in vol_edits:
        a = _good_args(_lib, L)
        setattr(a.volume, field, value)
        assert fwd(a) == code, ("volume", field, value)
    a = _good_args(_lib, L)
    a.volume.Nz, a.volume.Ny, a.volume.Nx = 2048, 1024, 1024
    assert fwd(a) == EUNSUPPORTED
    a = _good_args(_lib, L)
    a.h, a.w, a.workspace_bytes = 65536, 32768, 2 ** 40
    assert fwd(a) == EUNSUPPORTED
    # a workspace sized for a coarser stride is short for stride 1
    a = _good_args(_lib, L)
    a.workspace_bytes = L.idh_tsdf_align_workspace_bytes(24, 32, 2, 4)
    assert fwd(a) == EWORKSPACE


def test_python_layer_refuses():
    import torch

    from implicit_depth_amd import _lib, fusion

    d = torch.ones(1, 1, 6, 8)
    eye = torch.eye(4)
    with pytest.raises(_lib.IdhError, match="requires grad"):
        fusion.align_depth(None, d.clone().requires_grad_(), eye, eye)
    with pytest.raises(_lib.IdhError, match="requires grad"):
        fusion.align_depth(None, d, eye, eye.clone().requires_grad_())
    with pytest.raises(_lib.IdhError, match=r"\(1,1,h,w\)"):
        fusion.align_depth(None, torch.ones(2, 1, 6, 8), eye, eye)
    with pytest.raises(_lib.IdhError, match="weight"):
        fusion.align_depth(None, d, eye, eye, weight_11hw=torch.ones(1, 1, 6, 7))
    for schedule in ((), ((0, 3),), ((1, 0),), ((1, 65),)):
        with pytest.raises(_lib.IdhError, match="schedule"):
            fusion.align_depth(None, d, eye, eye, schedule=schedule)
    with pytest.raises(_lib.IdhError, match="schedule"):
        fusion.align_depth(None, d, eye, eye, iters=0)
    with pytest.raises(_lib.IdhError, match="CPU tensor"):
        fusion.align_depth(None, d, eye, eye)


def test_alignment_summary():
    from implicit_depth_amd import _lib, fusion

    rec = np.zeros((4, 40))
    rec[0, 27:32] = (4.0, 100, 0, 0.02, 0.01)
    rec[1, 27:32] = (1.0, 100, 0, 0.001, 0.002)
    rec[2:, 29] = 3
    s = fusion.alignment_summary(rec)
    assert s == {"status": 0, "count": 100, "rms": 0.1, "iterations": 2, "stopped": True, "translation": 0.021, "rotation": 0.012}
    rec[1, 28:30] = (3, 1)
    assert fusion.alignment_summary(rec)["status"] == 1
    with pytest.raises(_lib.IdhError):
        fusion.alignment_summary(rec[2:])
