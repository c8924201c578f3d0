"""TSDF colour without a GPU (include/idh_fusion.h): the fp64 reference of tests/tsdf_color_ref.py stays under the
ambiguity cap and holds the cases it is there for; the ctypes mirrors match the library; every error code of the three entry points
returns before a launch; the new kernels compile for gfx950 without scratch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import tsdf_color_ref as CR
import tsdf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4


@pytest.mark.parametrize("scene", sorted(R.SCENES))
@pytest.mark.parametrize("cam", CR.COLOR_CAMERAS)
def test_reference_stays_under_the_cap_and_holds_its_cases(scene, cam):
    r = CR.scene_integrated(scene, cam)
    base = R.scene_integrated(scene)
    assert np.array_equal(r["T"], base["T"]) and np.array_equal(r["W"], base["W"]) and np.array_equal(r["touched"], base["touched"])
    touched, coloured = int(r["touched"].sum()), int(r["coloured"].sum())
    amb = int((r["touched"] & r["ambiguous"]).sum())
    print(f"{scene} {cam}: {touched} touched, {coloured} coloured, {amb} ambiguous among the touched ({amb / touched:.4%}), "
          f"{r['band_outside']} band updates off the frame, {int(r['free_only'].sum())} voxels of free space only")
    assert amb <= CR.CAP * touched and int(r["ambiguous"].sum()) <= CR.CAP * r["touched"].size
    assert 0 < coloured < touched
    assert (r["coloured"] <= r["touched"]).all()
    assert r["free_only"].sum() > 100 and (r["Wc"][r["free_only"]] == 0).all() and (r["C"][r["free_only"]] == 0).all()
    assert (r["Wc"] <= r["W"]).all() and r["Wc"].max() == R.SCENES[scene][5]
    assert (r["Wc"][~r["coloured"]] == 0).all() and (r["Wc"][r["coloured"]] >= 1).all()
    assert r["C"].min() >= 0 and r["C"].max() <= 255
    if cam == "odd":
        assert r["band_outside"] > 50  # part of the band falls outside the unrelated camera's frame
        assert (r["band"] & ~r["coloured"]).sum() > 0  # and some band voxels no frame covers at all
    else:
        assert r["band_outside"] == 0 or cam == "double"  # (the doubled camera sees exactly the map's view up to rounding)


def test_reference_weight_cap_and_depth_only_maps():
    r = CR.scene_integrated("room24x32", "same", None, 2.0)
    assert r["Wc"].max() == 2 and set(np.unique(r["Wc"])) == {0.0, 1.0, 2.0} and (r["Wc"] <= r["W"]).all()
    # depth-only maps on a coloured volume leave the colours alone
    dims, v, origin, depth, K, E = R.scene_inputs("room24x32")
    full = CR.scene_integrated("room24x32", "same")
    colors = np.concatenate([full["C"].astype(np.float32), full["Wc"][..., None]], -1)
    values = np.stack([full["T"].astype(np.float32), full["W"]], -1)
    again = CR.integrate(values, colors, depth, K, E, None, None, origin, v)
    assert np.array_equal(again["C"], colors[..., :3].astype(np.float64)) and np.array_equal(again["Wc"], colors[..., 3])
    assert (again["W"] >= full["W"]).all() and again["W"].max() == 6


def test_sizeof_mirrors_and_symbols():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert L.idh_sizeof_tsdf_integrate_color_args() == C.sizeof(_lib.TsdfIntegrateColorArgs)
    assert L.idh_sizeof_tsdf_raycast_color_args() == C.sizeof(_lib.TsdfRaycastColorArgs)
    assert L.idh_sizeof_tsdf_mesh_colors_args() == C.sizeof(_lib.TsdfMeshColorsArgs)
    assert C.sizeof(_lib.TsdfIntegrateColorArgs) > C.sizeof(_lib.TsdfIntegrateArgs) and C.sizeof(_lib.TsdfRaycastColorArgs) > C.sizeof(_lib.TsdfRaycastArgs)
    # the plain fields sit where they sit in the plain structs
    for plain, col in ((_lib.TsdfIntegrateArgs, _lib.TsdfIntegrateColorArgs), (_lib.TsdfRaycastArgs, _lib.TsdfRaycastColorArgs)):
        for name, _ in plain._fields_:
            assert getattr(plain, name).offset == getattr(col, name).offset, name
    header = open(os.path.join(ROOT, "include", "idh_fusion.h")).read()
    for name in ("idh_tsdf_integrate_color_fwd", "idh_tsdf_raycast_color_fwd", "idh_tsdf_mesh_colors_fwd"):
        assert callable(getattr(L, name)) and name in _lib.declared_symbols() and f"int {name}(" in header


def _vol():
    from implicit_depth_amd import _lib

    x = _lib.TsdfVolume()
    x.values, x.block_flags, x.block_flag_bytes = 0x1000, 0x2000, 1 << 20
    x.voxel_size, x.trunc_voxels, x.Nz, x.Ny, x.Nx = 0.04, 3.0, 20, 28, 36
    return x


def _good(kind):
    """Argument structs that pass every check, on fake non-null pointers: nothing below reaches a launch."""
    from implicit_depth_amd import _lib

    if kind == "integrate":
        a = _lib.TsdfIntegrateColorArgs()
        a.volume, a.depth_m1hw, a.K_m44, a.cam_T_world_m44, a.max_weight, a.M, a.h, a.w = _vol(), 0x3000, 0x4000, 0x5000, 64.0, 2, 24, 32
        a.colors_zyx4, a.color_mhw3, a.color_K_m44, a.hc, a.wc = 0x7000, 0x8000, 0x9000, 48, 64
    elif kind == "raycast":
        a = _lib.TsdfRaycastColorArgs()
        a.volume, a.world_T_cam_b44, a.invK_b44, a.depth_b1hw, a.flags_bhw = _vol(), 0x3000, 0x4000, 0x5000, 0x6000
        a.near, a.step_voxels, a.empty_depth, a.max_steps, a.skip, a.B, a.H, a.W = 0.25, 1.0, -1.0, 100, 1, 1, 24, 32
        a.colors_zyx4, a.rgba_bhw4 = 0x7000, 0x8000
    else:
        a = _lib.TsdfMeshColorsArgs()
        a.mesh.volume, a.mesh.workspace, a.mesh.workspace_bytes, a.mesh.vert_capacity = _vol(), 0xa000, 1 << 30, 100
        a.colors_zyx4, a.rgba_v4 = 0x7000, 0x8000
    return a


def _volume_of(a):
    return a.mesh.volume if hasattr(a, "mesh") else a.volume


def _set(obj, **kw):
    for k, x in kw.items():
        setattr(obj, k, x)


def _origin_nan(v):
    v.origin[1] = float("nan")


VOLUME_CASES = [(dict(struct_size=8), EINVAL), (dict(Nz=1), EINVAL), (dict(Ny=0), EINVAL), (dict(Nx=-4), EINVAL), (dict(voxel_size=0.0), EINVAL),
                (dict(voxel_size=float("inf")), EINVAL), (dict(trunc_voxels=float("nan")), EINVAL), (dict(trunc_voxels=-1.0), EINVAL),
                (_origin_nan, EINVAL), (dict(values=None), EINVAL), (dict(Nz=2048, Ny=1024, Nx=1024, block_flag_bytes=1 << 40), EUNSUPPORTED),
                (dict(Nz=65536, Ny=2, Nx=2), EUNSUPPORTED), (dict(Nz=2, Ny=262141, Nx=2), EUNSUPPORTED), (dict(block_flags=None), EWORKSPACE),
                (dict(block_flag_bytes=59), EWORKSPACE), (dict(block_flag_bytes=-1), EWORKSPACE)]

ARG_CASES = {
    "integrate": [(kw, EINVAL) for kw in (  # (112: the size of the plain idh_tsdf_integrate_args)
        dict(struct_size=16), dict(struct_size=112), dict(M=0), dict(h=0), dict(w=-1), dict(max_weight=0.5),
        dict(max_weight=float("inf")), dict(max_weight=float("nan")), dict(depth_m1hw=None), dict(K_m44=None), dict(cam_T_world_m44=None),
        dict(colors_zyx4=None), dict(color_mhw3=None), dict(color_K_m44=None), dict(hc=0), dict(wc=-3), dict(colors_zyx4=0x7008))]
    + [(dict(M=17), EUNSUPPORTED), (dict(M=16, h=1 << 14, w=1 << 13), EUNSUPPORTED), (dict(M=16, hc=1 << 14, wc=1 << 13), EUNSUPPORTED),
       (dict(M=2, hc=1 << 15, wc=1 << 15), EUNSUPPORTED)],
    "raycast": [(kw, EINVAL) for kw in (
        dict(struct_size=16), dict(B=0), dict(H=0), dict(W=-2), dict(max_steps=0), dict(step_voxels=0.0), dict(step_voxels=1.5),
        dict(step_voxels=float("nan")), dict(near=-0.1), dict(near=float("inf")), dict(empty_depth=float("nan")), dict(world_T_cam_b44=None),
        dict(invK_b44=None), dict(depth_b1hw=None), dict(flags_bhw=None), dict(colors_zyx4=None), dict(rgba_bhw4=None), dict(colors_zyx4=0x7004))]
    + [(dict(B=129), EUNSUPPORTED), (dict(B=128, H=4096, W=4096), EUNSUPPORTED), (dict(max_steps=65537), EUNSUPPORTED)],
    "mesh": [(kw, EINVAL) for kw in (dict(struct_size=16), dict(colors_zyx4=None), dict(rgba_v4=None), dict(colors_zyx4=0x7004))],
}
MESH_INNER_CASES = [(dict(struct_size=16), EINVAL), (dict(min_weight=-1.0), EINVAL), (dict(min_weight=float("nan")), EINVAL),
                    (dict(vert_capacity=-1), EINVAL), (dict(workspace=None), EWORKSPACE), (dict(workspace_bytes=100), EWORKSPACE),
                    (dict(workspace_bytes=-1), EWORKSPACE), (dict(workspace=0xa008), EINVAL)]


@pytest.mark.parametrize("kind", ["integrate", "raycast", "mesh"])
def test_error_codes_before_any_launch(kind):
    from implicit_depth_amd import _lib

    L = _lib.lib()
    fn = {"integrate": L.idh_tsdf_integrate_color_fwd, "raycast": L.idh_tsdf_raycast_color_fwd, "mesh": L.idh_tsdf_mesh_colors_fwd}[kind]
    assert fn(None, None) == EINVAL
    for edit, code in VOLUME_CASES:
        a = _good(kind)
        edit(_volume_of(a)) if callable(edit) else _set(_volume_of(a), **edit)
        assert fn(C.byref(a), None) == code, (kind, edit, code)
    for kw, code in ARG_CASES[kind]:
        a = _good(kind)
        _set(a, **kw)
        assert fn(C.byref(a), None) == code, (kind, kw, code)
    if kind == "mesh":
        for kw, code in MESH_INNER_CASES:
            a = _good(kind)
            _set(a.mesh, **kw)
            assert fn(C.byref(a), None) == code, (kind, kw, code)
        a = _good(kind)  # more than 2^28 voxels
        _set(a.mesh.volume, Nz=1024, Ny=1024, Nx=512, block_flag_bytes=1 << 40)
        assert fn(C.byref(a), None) == EUNSUPPORTED
        a = _good(kind)  # the plain mesh outputs are not read: null is fine, and a capacity of zero returns before the launch
        _set(a.mesh, vert_capacity=0, verts_v3=None, faces_f3=None, totals=None)
        assert fn(C.byref(a), None) == 0


def test_new_kernels_use_no_scratch():
    """The colour integrate and the mesh colours compile for gfx950 without scratch; the colour ray casts use no more than their plain
    counterparts (tools/kernel_resources.py, as test_abi.py runs it)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    csrc = os.path.join(ROOT, "implicit-depth_amd", "csrc")
    rows = {r["Name"]: int(r.get("ScratchSize [bytes/lane]", 0)) for src in ("tsdf.hip", "tsdf_mesh.hip") for r in kr.resources(os.path.join(csrc, src))}
    print(rows)
    for name in ("tsdf_integrate_k<IntegrateColorArgs>", "tsdf_integrate_k<IntegrateArgs>", "mesh_colors_k", "mesh_emit_k"):
        assert name in rows and rows[name] == 0, (name, sorted(rows))
    for skip in ("true", "false"):
        for normals in ("true", "false"):
            plain, col = f"tsdf_raycast_k<{skip}, {normals}, RaycastArgs>", f"tsdf_raycast_k<{skip}, {normals}, RaycastColorArgs>"
            assert plain in rows and col in rows, sorted(rows)
            assert rows[col] <= rows[plain], (col, rows[col], rows[plain])
