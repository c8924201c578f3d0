"""Surface normals from depth without a GPU: the fp64 restatement of the contract (tests/normals_ref.py) against the torch fp32 composition
that kornia executes, the properties of the contract (planes, constants, zeros, the footprint of a NaN), and the host side of the C ABI
(include/idh_geometry.h): the symbols are bound and every IDH_EINVAL case returns before a launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import normals_ref as NR

EPS32 = float(np.finfo(np.float32).eps)


def rounding_bound(depth, invK, k, s):
    """What fp32 rounding may do to a normal of this input, pixel by pixel.  The points carry a few roundings of size eps * |p| each (the
    blur sums, the back-projection, the nine-tap sums: 16 eps |p| taken together), a gradient therefore an absolute error
    dg <= 16 eps max|p| over its 3x3 window; the cross product moves by at most 2 |g| dg and the unit normal by that over |cross|."""
    d = np.asarray(depth, dtype=np.float64)[:, 0]
    pts = NR.backproject64(NR.blur64(d, k, s), np.asarray(invK))
    rows, cols = NR._taps(d.shape[1], d.shape[2])
    nb = [pts[:, :, rows[i]][:, :, :, cols[j]] for i in range(3) for j in range(3)]
    gx = sum(NR.SOBEL_X.reshape(-1)[t] * nb[t] for t in range(9))
    gy = sum(NR.SOBEL_Y.reshape(-1)[t] * nb[t] for t in range(9))
    cross = np.sqrt((np.cross(gx, gy, axis=1) ** 2).sum(1))
    g = np.maximum(np.abs(gx).max(1), np.abs(gy).max(1))
    pmax = np.max([np.abs(t).max(1) for t in nb], 0)
    return float((2 * g * 16 * EPS32 * pmax / cross).max())


@pytest.mark.parametrize("k", NR.KS)
@pytest.mark.parametrize("shape", [(13, 19), (24, 32), (70, 130)])
def test_restatement_agrees_with_the_fp32_composition(shape, k):
    H, W = shape
    depth, invK = NR.field(2, H, W), NR.inv_intrinsics(2, H, W)
    assert NR.conditioning(depth, invK, k, 2.0) >= 0.04  # no pixel of the field is ill-conditioned: every pixel is compared
    ref, _, _ = NR.dense(depth, invK, k, 2.0)
    err, bound = NR.max_err(NR.composition(depth, invK, k, 2.0), ref), rounding_bound(depth, invK, k, 2.0)
    print(f"{H}x{W} k={k}: composition vs fp64 {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    assert np.abs(np.sqrt((ref ** 2).sum(1)) - 1).max() < 1e-12


@pytest.mark.parametrize("shape", [(4, 5, 7), (3, 3, 3), (2, 2, 3), (1, 1, 1)])
def test_restatement_at_the_smallest_shapes_reflect_allows(shape):
    H, W, k = shape
    depth, invK = NR.field(2, H, W) if H > 1 else torch.full((2, 1, 1, 1), 2.0), NR.inv_intrinsics(2, H, W)
    ref, _, _ = NR.dense(depth, invK, k, 2.0)
    comp = NR.composition(depth, invK, k, 2.0)
    if H == 1:  # one pixel: every tap is that pixel, both gradients vanish
        assert (ref == 0).all() and bool((comp == 0).all())
    else:
        assert NR.max_err(comp, ref) <= rounding_bound(depth, invK, k, 2.0)


def test_a_tilted_plane_gives_its_normal_at_every_pixel_borders_included():
    """k = 1: replicate padding turns the border differences into one-sided ones, which stay in the plane."""
    H, W = 24, 32
    invK = NR.inv_intrinsics(1, H, W)
    n = np.array([0.3, -0.2, 1.0])
    n /= np.linalg.norm(n)
    y, x = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    ray = np.einsum("ij,jhw->ihw", invK[0, :3, :3].double().numpy(), np.stack([x, y, np.ones_like(x)]))
    z = 2.0 / (n[:, None, None] * ray).sum(0)  # the plane n . X = 2
    ref, _, dot = NR.dense(z[None, None], invK, 1, 2.0)
    want = np.broadcast_to(n[None, :, None, None], ref.shape)
    assert np.abs(ref - want).max() < 1e-10
    depth = torch.from_numpy(z[None, None].astype(np.float32))  # rounding the depth alone moves a point off the plane by eps * z
    assert (dot > 0).all()  # the reference's normal points away from the camera
    err = NR.max_err(NR.composition(depth, invK, 1, 2.0), want)
    print(f"plane {H}x{W}: fp32 composition max component error {err:.3g}")
    assert err <= rounding_bound(depth, invK, 1, 2.0)
    flipped, _, _ = NR.dense(z[None, None], invK, 1, 2.0, orient=True)
    assert np.abs(flipped + want).max() < 1e-10


@pytest.mark.parametrize("k", NR.KS)
def test_constant_and_zero_depths(k):
    invK = NR.inv_intrinsics(2, 9, 11)
    for fn in (lambda d: NR.dense(d, invK, k, 2.0)[0], lambda d: NR.composition(d, invK, k, 2.0).double().numpy()):
        n = fn(torch.full((2, 1, 9, 11), 1.75))
        assert np.abs(n - np.array([0.0, 0.0, 1.0])[None, :, None, None]).max() < 1e-5
        assert (fn(torch.zeros(2, 1, 9, 11)) == 0).all()  # exactly (0, 0, 0)


@pytest.mark.parametrize("k", NR.KS)
def test_a_nan_makes_exactly_its_footprint_non_finite(k):
    H, W, y0, x0 = 24, 32, 11, 17
    depth, invK = NR.field(1, H, W), NR.inv_intrinsics(1, H, W)
    depth[0, 0, y0, x0] = float("nan")
    r = k // 2 + 1
    want = np.zeros((H, W), dtype=bool)
    want[y0 - r:y0 + r + 1, x0 - r:x0 + r + 1] = True  # (2 (k // 2) + 3)^2 pixels: the blur radius plus the Sobel ring, the centre included
    for n in (NR.dense(depth, invK, k, 2.0)[0], NR.composition(depth, invK, k, 2.0).numpy()):
        bad = ~np.isfinite(n[0])
        assert (bad == want[None]).all()


def test_validity_is_the_footprint_of_the_flags():
    """An isolated hole invalidates its footprint; at a border the two index maps fold the footprint back into the image."""
    H, W, k = 20, 24, 5
    depth, invK = NR.field(1, H, W), NR.inv_intrinsics(1, H, W)
    flags = np.full((1, 1, H, W), 3, dtype=np.uint8)
    flags[0, 0, 10, 12] = 7
    n, valid, _ = NR.dense(depth, invK, k, 2.0, flags=flags)
    want = np.ones((H, W), dtype=np.uint8)
    want[7:14, 9:16] = 0
    assert (valid[0, 0] == want).all() and (n[0][:, want == 0] == 0).all() and (np.abs(n[0][:, want == 1]).sum(0) > 0.9).all()
    # a depth that carries a NaN where the flags say so never reaches a valid normal
    depth[0, 0, 10, 12] = float("nan")
    assert np.isfinite(NR.dense(depth, invK, k, 2.0, flags=flags)[0]).all()
    flags[:] = 3
    flags[0, 0, 0, 0] = 0  # corner: reflect reads it from rows / columns 0 .. 2, replicate one further
    _, valid, _ = NR.dense(depth, invK, k, 2.0, flags=flags)
    want[:] = 1
    want[:4, :4] = 0
    assert (valid[0, 0] == want).all()


def test_patch_form_is_the_dense_form_at_interior_pixels():
    H, W = 9, 12
    depth, invK = NR.field(2, H, W), NR.inv_intrinsics(2, H, W)
    ref, _, _ = NR.dense(depth, invK, 1, 2.0)
    pts = torch.from_numpy(NR.backproject64(depth[:, 0].double().numpy(), invK.numpy()))
    got, _, _ = NR.patch(NR.patches_of(pts))
    assert np.array_equal(got.reshape(2, H - 2, W - 2, 3), ref[:, :, 1:-1, 1:-1].transpose(0, 2, 3, 1))


# ---- the C ABI, host side --------------------------------------------------------------------------------------------------------------
NAMES = ("idh_depth_normals_fwd", "idh_patch_normals_fwd", "idh_sizeof_normals_args", "idh_sizeof_patch_normals_args")


def test_header_symbols_are_bound():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.declared_symbols() and hasattr(L, name)
    assert L.idh_sizeof_normals_args() == C.sizeof(_lib.NormalsArgs) == _lib.NormalsArgs().struct_size
    assert L.idh_sizeof_patch_normals_args() == C.sizeof(_lib.PatchNormalsArgs) == _lib.PatchNormalsArgs().struct_size


FAKE = 0x10000  # a non-null pointer that is never dereferenced: every call below returns before a launch


def _dense_args(**kw):
    from implicit_depth_amd import _lib

    a = _lib.NormalsArgs()
    a.depth_b1hw, a.invK_b44, a.normals_b3hw = FAKE, FAKE, FAKE
    a.smoothing_std, a.kernel_size, a.need, a.B, a.H, a.W = 2.0, 5, 3, 2, 13, 19
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _patch_args(**kw):
    from implicit_depth_amd import _lib

    a = _lib.PatchNormalsArgs()
    a.points_bn93, a.normals_bn3, a.need, a.B, a.N = FAKE, FAKE, 3, 2, 10
    for k, v in kw.items():
        setattr(a, k, v)
    return a


DENSE_EINVAL = [dict(depth_b1hw=None), dict(invK_b44=None), dict(normals_b3hw=None), dict(struct_size=8),
                dict(kernel_size=0), dict(kernel_size=2), dict(kernel_size=4), dict(kernel_size=9), dict(kernel_size=-1),
                dict(smoothing_std=0.0), dict(smoothing_std=-1.0), dict(smoothing_std=float("nan")),
                dict(kernel_size=7, H=3), dict(kernel_size=7, W=3), dict(kernel_size=3, H=1), dict(kernel_size=1, H=0), dict(kernel_size=1, W=0),
                dict(H=-4), dict(B=-1), dict(flags_b1hw=FAKE), dict(B=0, kernel_size=6), dict(B=0, depth_b1hw=None)]
PATCH_EINVAL = [dict(points_bn93=None), dict(normals_bn3=None), dict(struct_size=8), dict(B=-1), dict(N=-1), dict(flags_bn9=FAKE),
                dict(orient=1), dict(N=0, normals_bn3=None)]


def test_every_einval_case_returns_before_a_launch():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert L.idh_depth_normals_fwd(None, None) == -1 and L.idh_patch_normals_fwd(None, None) == -1
    for kw in DENSE_EINVAL:
        assert L.idh_depth_normals_fwd(_dense_args(**kw), None) == -1, kw
    for kw in PATCH_EINVAL:
        assert L.idh_patch_normals_fwd(_patch_args(**kw), None) == -1, kw
    # B == 0 and N == 0 succeed without a launch (no GPU is touched here), with and without the options
    assert L.idh_depth_normals_fwd(_dense_args(B=0), None) == 0
    assert L.idh_depth_normals_fwd(_dense_args(B=0, flags_b1hw=FAKE, valid_b1hw=FAKE, world_R_cam_b33=FAKE, orient=1, kernel_size=7, H=4, W=5), None) == 0
    assert L.idh_patch_normals_fwd(_patch_args(B=0), None) == 0 and L.idh_patch_normals_fwd(_patch_args(N=0), None) == 0
    assert L.idh_patch_normals_fwd(_patch_args(N=0, orient=1, cam_centre_b3=FAKE, flags_bn9=FAKE, valid_bn=FAKE), None) == 0


def test_python_surface_refuses_cpu_tensors_and_bad_sizes():
    from implicit_depth_amd import dropin, geometry
    from implicit_depth_amd._lib import IdhError

    depth, invK = NR.field(1, 8, 8), NR.inv_intrinsics(1, 8, 8)
    gen = geometry.NormalGenerator(8, 8)
    assert (gen.kernel_size, gen.std) == (5, 2.0) and list(gen.state_dict()) == ["backproject.pix_coords_13N"]
    with pytest.raises(IdhError, match="CPU"):
        gen(depth, invK)
    with pytest.raises(IdhError, match="CPU"):
        geometry.depth_normals(depth, invK)
    with pytest.raises(IdhError, match="CPU"):
        geometry.patch_normals(torch.zeros(1, 2, 9, 3))
    with pytest.raises(IdhError, match="smoothing_kernel_size"):
        geometry.NormalGenerator(8, 8, smoothing_kernel_size=4)
    # convert(native_normals=True) swaps a reference-shaped compute_normals for the native module, and only with the flag
    import hot_helpers

    class RefNormals(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.height, self.width, self.kernel_size, self.std = 6, 10, 3, 1.5
            self.backproject = geometry.BackprojectDepth(6, 10)

    m = hot_helpers.holder(2, "dot", 4, 4, 4, decoder="depth", with_mlp=False)
    m.compute_normals = ref = RefNormals()
    assert dropin.convert(m).compute_normals is ref
    new = dropin.convert(m, native_normals=True).compute_normals
    assert isinstance(new, geometry.NormalGenerator) and (new.height, new.width, new.kernel_size, new.std) == (6, 10, 3, 1.5)
    assert list(new.state_dict()) == list(ref.state_dict()) and dropin.convert(m, native_normals=True).compute_normals is new
