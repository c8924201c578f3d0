"""Surface normals from depth on the GPU: depth_normals_k / patch_normals_k (csrc/normals.hip) through geometry.depth_normals /
patch_normals / NormalGenerator against the fp64 restatement of the contract (tests/normals_ref.py).  The accuracy bound is not a constant:
it is FACTOR = 4 times the error of the torch fp32 composition - what kornia executes - against fp64 on the same input, with a floor of a
few fp32 ulps of 1.0.  The metric is the largest absolute component difference; every pixel is compared.

Measured on an MI355X (composition, kernel) per shape: DESIGN.md §4.18."""
import numpy as np
import pytest
import torch

import normals_ref as NR

pytestmark = pytest.mark.gpu
STD = 2.0
# (B, H, W, k): 13x19 is no multiple of the 64x8 tile and lies within a halo of a border everywhere; 4x5 / 3x3 are the smallest shapes
# reflect allows for k = 7 / 3; 48x64 is whole tiles; 70x130 has several tiles in both directions and ragged edges
CASES = ([(2, 13, 19, k) for k in NR.KS] + [(2, 4, 5, 7), (2, 3, 3, 3)] + [(2, 48, 64, k) for k in NR.KS] + [(3, 70, 130, k) for k in NR.KS])
_REF = {}


def _ref(B, H, W, k):
    """Input, fp64 restatement and the composition's own error, computed once per case and shared."""
    key = (B, H, W, k)
    if key not in _REF:
        depth, invK = NR.field(B, H, W), NR.inv_intrinsics(B, H, W)
        ref, _, dot = NR.dense(depth, invK, k, STD)
        _REF[key] = (depth, invK, ref, dot, NR.max_err(NR.composition(depth, invK, k, STD), ref))
    return _REF[key]


def _bound(comp_err):
    return max(NR.FACTOR * comp_err, NR.FLOOR)


def _normals(depth, invK, **kw):
    from implicit_depth_amd import geometry

    n, valid = geometry.depth_normals(depth.cuda(), invK.cuda(), **kw)
    torch.cuda.synchronize()
    return n.cpu().numpy(), (None if valid is None else valid.cpu().numpy())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}_{}x{}_k{}".format(*c))
def test_dense_kernel_against_fp64(case):
    B, H, W, k = case
    depth, invK, ref, _, comp = _ref(*case)
    got, valid = _normals(depth, invK, kernel_size=k, std=STD)
    assert valid is None and got.shape == (B, 3, H, W)
    err = NR.max_err(got, ref)
    print(f"{H}x{W} B={B} k={k}: composition {comp:.3g}, kernel {err:.3g} (bound {_bound(comp):.3g})")
    assert err <= _bound(comp)
    if k == 5 and (H, W) == (13, 19):  # the module is the same launch; an empty batch is a no-op
        from implicit_depth_amd import geometry

        gen = geometry.NormalGenerator(H, W, k, STD).cuda()
        assert np.array_equal(gen(depth.cuda(), invK.cuda()).cpu().numpy(), got)
        empty, _ = geometry.depth_normals(depth.cuda()[:0], invK.cuda()[:0], kernel_size=k)
        assert tuple(empty.shape) == (0, 3, H, W)


@pytest.mark.parametrize("k", NR.KS)
def test_zeros_and_the_finite_mask(k):
    """Zeros map to exact zeros; with one NaN, one +inf and a block of zeros in the input the non-finite pattern is the restatement's."""
    B, H, W = 2, 48, 70
    invK = NR.inv_intrinsics(B, H, W)
    got, _ = _normals(torch.zeros(B, 1, H, W), invK, kernel_size=k)
    assert (got == 0).all()
    depth = NR.field(B, H, W)
    depth[0, 0, 7, 63] = float("nan")   # on a tile seam in both directions
    depth[1, 0, 30, 5] = float("inf")
    depth[0, 0, 0, W - 1] = float("inf")  # a corner: the border maps fold the footprint
    depth[:, 0, 20:36, 20:40] = 0.0
    ref, _, _ = NR.dense(depth, invK, k, STD)
    got, _ = _normals(depth, invK, kernel_size=k, std=STD)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)) and not np.isfinite(ref).all()
    zero = (ref == 0).all(1)
    assert zero[:, 24:32, 24:36].all() and (got.transpose(0, 2, 3, 1)[zero] == 0).all()


def _holes(B, H, W):
    flags = np.full((B, 1, H, W), 3, dtype=np.uint8)
    for b, y, x, v in ((0, 5, 9, 7), (0, H // 2, W // 2, 1), (1, 0, 0, 0), (1, H - 1, W - 1, 2), (0, 7, min(63, W - 2), 5), (1, min(8, H - 2), min(64, W - 1), 6),
                       (B - 1, H - 3, 3, 4)):
        flags[b, 0, y, x] = v
    return flags


@pytest.mark.parametrize("case", [(2, 70, 130, 5), (2, 70, 130, 1), (2, 13, 19, 7), (3, 24, 66, 3)], ids=lambda c: "B{}_{}x{}_k{}".format(*c))
def test_validity_map_rotation_and_orientation(case):
    """Flags with isolated holes, holes at two corners and at a tile seam; the depth holds garbage there.  valid equals the restatement's,
    invalid pixels are exact zeros, and with rotation and orientation on the valid normals match the restatement: the rotation adds
    three products and two sums of numbers <= 1 to each component, FLOOR covers them."""
    B, H, W, k = case
    depth, invK, _, _, comp = _ref(*case) if case in CASES else (NR.field(B, H, W), NR.inv_intrinsics(B, H, W), None, None, None)
    if comp is None:
        comp = NR.max_err(NR.composition(depth, invK, k, STD), NR.dense(depth, invK, k, STD)[0])
    flags = _holes(B, H, W)
    dirty = depth.clone()
    dirty[torch.from_numpy(flags != 3)] = float("nan")
    rot = NR.rotations(B)
    ref, valid_ref, dot = NR.dense(dirty, invK, k, STD, world_R_cam=rot, orient=True, flags=flags)
    ok = valid_ref[:, 0] == 1
    assert 0 < ok.sum() < ok.size and np.abs(dot[ok]).min() > 1e-3  # no valid pixel's orientation hangs on rounding
    got, valid = _normals(dirty, invK, kernel_size=k, std=STD, world_R_cam=rot.cuda(), orient=True, flags=torch.from_numpy(flags).cuda())
    assert valid.dtype == np.uint8 and np.array_equal(valid, valid_ref)
    assert (got.transpose(0, 2, 3, 1)[~ok] == 0).all() and np.isfinite(got).all()
    err = NR.max_err(got, ref)
    print(f"{H}x{W} B={B} k={k} rotated + oriented: kernel {err:.3g} (bound {NR.FACTOR * comp + NR.FLOOR:.3g}); valid {ok.mean():.3f}")
    assert err <= NR.FACTOR * comp + NR.FLOOR
    # orientation alone, in camera space: n . p <= 0 at every valid pixel, and the flip is the only difference to the plain launch
    cam, _ = _normals(dirty, invK, kernel_size=k, std=STD, orient=True, flags=torch.from_numpy(flags).cuda())
    pts = NR.backproject64(NR.blur64(np.nan_to_num(dirty[:, 0].double().numpy()), k, STD), invK.numpy())
    assert ((cam * pts).sum(1)[ok] < 0).all()
    plain, _ = _normals(dirty, invK, kernel_size=k, std=STD, flags=torch.from_numpy(flags).cuda())
    flip = np.where((dot > 0)[:, None], -plain, plain)
    assert np.array_equal(flip.transpose(0, 2, 3, 1)[ok], cam.transpose(0, 2, 3, 1)[ok])
    other, valid_other = _normals(dirty, invK, kernel_size=k, std=STD, flags=torch.from_numpy(flags).cuda(), need=7)
    assert valid_other.sum() == 0 and (other == 0).all()


def test_patch_kernel_against_fp64_and_options():
    from implicit_depth_amd import geometry

    B, N = 2, 300  # more than one workgroup, no multiple of one
    rng = np.random.default_rng(11)
    base = rng.uniform(-1, 1, (B, N, 1, 3)) * 2 + np.array([0, 0, 4.0])
    du, dv = rng.standard_normal((B, N, 1, 3)) * 0.05, rng.standard_normal((B, N, 1, 3)) * 0.05
    i, j = np.meshgrid(np.arange(-1, 2), np.arange(-1, 2), indexing="ij")
    pts = base + j.reshape(1, 1, 9, 1) * du + i.reshape(1, 1, 9, 1) * dv + rng.standard_normal((B, N, 9, 3)) * 1e-3
    pts = torch.from_numpy(pts.astype(np.float32))
    centre = torch.from_numpy(rng.standard_normal((B, 3)).astype(np.float32) * 0.1)
    flags = np.full((B, N, 9), 3, dtype=np.uint8)
    flags[0, 5, 4], flags[1, 299, 0], flags[1, 17, 8] = 1, 7, 0
    ref, _, _ = NR.patch(pts.numpy())
    got, valid = geometry.patch_normals(pts.cuda())
    assert valid is None
    # the same chain of roundings as the dense form after its points: the nine-tap sums, cross, norm.  Per component 16 eps |p| / |g| ...
    p = pts.double().numpy()
    gx = sum(NR.SOBEL_X.reshape(-1)[t] * p[:, :, t] for t in range(9))
    gy = sum(NR.SOBEL_Y.reshape(-1)[t] * p[:, :, t] for t in range(9))
    g = np.maximum(np.abs(gx).max(-1), np.abs(gy).max(-1))
    bound = (2 * g * 16 * np.finfo(np.float32).eps * np.abs(p).max((-1, -2)) / np.sqrt((np.cross(gx, gy) ** 2).sum(-1)))
    err = np.abs(got.cpu().numpy() - ref).max(-1)
    print(f"patch normals: worst error / bound {np.max(err / bound):.3g}, max error {err.max():.3g}")
    assert (err <= bound).all()
    ref_o, valid_ref, dot = NR.patch(pts.numpy(), cam_centre=centre.numpy(), orient=True, flags=flags)
    sure = np.abs(dot) > 1e-3
    got_o, valid = geometry.patch_normals(pts.cuda(), cam_centre=centre.cuda(), orient=True, flags=torch.from_numpy(flags).cuda())
    assert np.array_equal(valid.cpu().numpy(), valid_ref) and valid_ref.sum() == B * N - 3
    assert (got_o.cpu().numpy()[valid_ref == 0] == 0).all()
    assert sure.mean() > 0.95 and (np.abs(got_o.cpu().numpy() - ref_o).max(-1)[sure] <= bound[sure]).all()
    assert np.array_equal(np.abs(got_o.cpu().numpy())[valid_ref == 1], np.abs(got.cpu().numpy())[valid_ref == 1])  # only the sign may differ
    empty, _ = geometry.patch_normals(pts.cuda()[:, :0])
    assert tuple(empty.shape) == (B, 0, 3)


@pytest.mark.parametrize("shape", [(13, 19), (70, 130)])
def test_dense_and_patch_kernels_share_their_bits(shape):
    """depth_normals(k = 1) at interior pixels equals patch_normals on the 3x3 patches of the same back-projected points, formed in torch with
    the expression order of step 2: one device function serves both."""
    from implicit_depth_amd import geometry

    H, W = shape
    depth, invK = NR.field(2, H, W).cuda(), NR.inv_intrinsics(2, H, W).cuda()
    dense, _ = geometry.depth_normals(depth, invK, kernel_size=1)
    patches = NR.patches_of(NR.points32(depth, invK))
    sparse, _ = geometry.patch_normals(patches)
    a = dense[:, :, 1:-1, 1:-1].permute(0, 2, 3, 1).reshape(2, -1, 3).contiguous()
    assert torch.equal(a.view(torch.int32), sparse.view(torch.int32))
    # ... and with the orientation rule: the dense form looks from the origin of the camera frame
    dense_o, _ = geometry.depth_normals(depth, invK, kernel_size=1, orient=True)
    sparse_o, _ = geometry.patch_normals(patches, cam_centre=torch.zeros(2, 3, device="cuda"), orient=True)
    a = dense_o[:, :, 1:-1, 1:-1].permute(0, 2, 3, 1).reshape(2, -1, 3).contiguous()
    assert torch.equal(a.view(torch.int32), sparse_o.view(torch.int32)) and not torch.equal(dense_o, dense)
