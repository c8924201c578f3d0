"""Mesh extraction from the TSDF volume on the GPU (include/idh_fusion.h, csrc/tsdf_mesh.hip, fusion.extract_mesh) against the numpy
statement of tests/mesh_ref.py run on the same float32 volume: faces and vertex counts exactly, positions within the bound the header's
arithmetic allows; the bit-level promises (determinism, block skipping, capacities); closed forms."""
import numpy as np
import pytest
import torch

import mesh_ref as M
import tsdf_ref as R

pytestmark = pytest.mark.gpu

# the scan works on chunks of 1024 voxels (256 threads x 4): a volume of more than 1024 x 1024 voxels has more first-level partial sums
# than one workgroup scans in one pass, so a second level is built.  104^3 = 1 124 864 voxels -> 1099 first-level sums.
SCAN_CHUNK = 1024
TWO_LEVEL_DIMS = (104, 104, 104)


def _cuda(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _volume(values, origin, v):
    from implicit_depth_amd import fusion

    return fusion.TSDFVolume.from_values(_cuda(values), v, origin)


def _check(values, origin, v, min_weight=0.0, what="", **kw):
    """Extract on the GPU and in numpy from the same float32 values; faces and counts exact, positions and weights within bounds."""
    from implicit_depth_amd import fusion

    got = fusion.extract_mesh(_volume(values, origin, v), min_weight=min_weight, return_weights=True, **kw)
    ref = M.extract(values, origin, v, min_weight=min_weight)
    assert got["verts"].dtype == torch.float32 and got["faces"].dtype == torch.int32 and got["weights"].dtype == torch.float32
    assert tuple(got["verts"].shape) == (len(ref["verts"]), 3) and tuple(got["weights"].shape) == (len(ref["verts"]),)
    assert tuple(got["faces"].shape) == (len(ref["faces"]), 3)
    assert np.array_equal(got["faces"].cpu().numpy(), ref["faces"])
    bound = M.position_bound(np.asarray(origin, np.float32), np.float32(v), values.shape[:3])
    err = np.abs(got["verts"].cpu().numpy().astype(np.float64) - ref["verts"]).max() if len(ref["verts"]) else 0.0
    werr = (np.abs(got["weights"].cpu().numpy().astype(np.float64) - ref["weights"]) / np.maximum(np.abs(ref["weights"]), 1e-30)).max() if len(ref["verts"]) else 0.0
    print(f"{what}: V = {len(ref['verts'])}, F = {len(ref['faces'])}, max position error {err:.3e} (bound {bound:.3e}), max relative weight error {werr:.2e}")
    assert err <= bound
    assert werr <= 1e-6
    return got, ref


def test_all_256_cases():
    values = M.case_volume()
    got, ref = _check(values, (0.1, -0.2, 0.3), 0.04, what="all cases")
    assert len(ref["faces"]) > 7000 and ref["emitted"][1, 1, 1::4].sum() == 254  # every brick's inner cell but those of cases 0 and 255


@pytest.fixture(scope="module")
def fused():
    """The GPU's fused float32 volumes of the two committed scenes, on the host."""
    from implicit_depth_amd import fusion

    out = {}
    for name in sorted(R.SCENES):
        dims, v, origin, depth, K, E = R.scene_inputs(name)
        vol = fusion.TSDFVolume(dims, v, origin)
        vol.integrate(_cuda(depth), _cuda(K), _cuda(E))
        out[name] = (vol, vol.values.cpu().numpy())
    return out


@pytest.mark.parametrize("name", sorted(R.SCENES))
@pytest.mark.parametrize("min_weight", [0.0, 1.0])
def test_fused_scenes(fused, name, min_weight):
    vol, values = fused[name]
    dims, v, origin = R.SCENES[name][:3]
    got, ref = _check(values, origin, v, min_weight=min_weight, what=f"{name} min_weight={min_weight}")
    assert len(ref["faces"]) > 300
    if min_weight:
        assert len(ref["faces"]) < len(M.extract(values, origin, v)["faces"])  # cells seen once are gone
        assert got["weights"].min() > 1.0
    # the volume integrate left (its own flags, not rebuilt ones) gives the same tensors, through the method too
    again = vol.extract_mesh(min_weight=min_weight, return_weights=True)
    assert all(torch.equal(again[k], got[k]) for k in ("verts", "faces", "weights"))
    assert M.vertices_on_crossed_edges(got["verts"].cpu().numpy(), values, origin, v).all()


def test_tails_x_crosses_wave_boundaries_and_no_dim_is_a_multiple_of_8():
    dims = (23, 37, 131)
    values = M.sphere_volume(dims, (70.3, 17.6, 11.2), 9.4)
    got, ref = _check(values, (-2.0, 0.5, 1.0), 0.03, what="sphere in (23, 37, 131)")
    V = len(ref["verts"])
    assert ref["verts"][:, 0].min() < -2.0 + 0.03 * 63 < -2.0 + 0.03 * 65 < ref["verts"][:, 0].max()  # x = 64 lies inside the sphere
    keys, counts, rcounts = M.directed_edges(got["faces"].cpu().numpy(), V)
    assert (counts == 1).all() and (rcounts == 1).all() and M.euler_characteristic(ref["faces"], V) == 2
    vols = M.signed_volumes(got["verts"].cpu().numpy(), got["faces"].cpu().numpy())
    assert len(vols) == 1 and 0.97 < sum(vols.values()) / (4 / 3 * np.pi * (9.4 * 0.03) ** 3) < 1
    # a surface that touches the last voxel of every axis: a slab of inside voxels along each high face
    values = np.ones((*dims, 2), np.float32)
    values[-1, :, :, 0] = values[:, -1, :, 0] = values[:, :, -1, 0] = -0.25
    values[0, 0, 0, 0] = -1.0
    _check(values, (0.0, 0.0, 0.0), 1.0, what="high faces")


def test_scan_with_two_levels_of_partial_sums():
    from implicit_depth_amd import _lib

    dims = TWO_LEVEL_DIMS
    n = dims[0] * dims[1] * dims[2]
    assert -(-n // SCAN_CHUNK) > SCAN_CHUNK
    assert _lib.lib().idh_tsdf_mesh_workspace_bytes(*dims) == 8 * n + 8 * (-(-n // SCAN_CHUNK)) + 8 * 2
    # one small sphere in the middle, one in the last slices: behind the 1024th first-level sum (z >= 97)
    values = M.sphere_volume(dims, (60.3, 50.2, 40.1), 5.2)
    late = M.sphere_volume(dims, (31.4, 72.3, 99.2), 3.3)
    values[..., 0] = np.minimum(values[..., 0], late[..., 0])
    got, ref = _check(values, (-1.0, -1.0, 0.5), 0.02, what="two spheres in 104^3")
    assert (ref["cell"] // (dims[1] * dims[2]) >= 97).sum() > 50 and (ref["cell"] // (dims[1] * dims[2]) < 50).sum() > 50
    vols = M.signed_volumes(got["verts"].cpu().numpy(), got["faces"].cpu().numpy())
    assert len(vols) == 2 and min(vols.values()) > 0


def test_bits_determinism_block_skipping_and_an_empty_volume():
    from implicit_depth_amd import fusion

    # a sphere known only near it: most blocks stay unflagged
    dims = (23, 37, 131)
    values = M.sphere_volume(dims, (70.3, 17.6, 11.2), 6.4, trunc=2.0)
    values[..., 1] = (np.abs(values[..., 0]) < 1).astype(np.float32) * 3
    vol = _volume(values, (0.0, 0.0, 0.0), 0.05)
    assert 0 < int(vol.block_flags.sum()) < vol.block_flags.numel() // 2
    a = fusion.extract_mesh(vol, return_weights=True, use_block_flags=True)
    b = fusion.extract_mesh(vol, return_weights=True, use_block_flags=True)
    c = fusion.extract_mesh(vol, return_weights=True, use_block_flags=False)
    assert a["faces"].shape[0] > 300
    for k in ("verts", "faces", "weights"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    assert np.array_equal(a["faces"].cpu().numpy(), M.extract(values, (0, 0, 0), 0.05)["faces"])
    # a single flagged block, in the far corner
    dims = (20, 20, 20)
    values = M.sphere_volume(dims, (18.2, 17.9, 18.1), 1.2)
    values[..., 1] = 0
    values[17:, 17:, 17:, 1] = 2
    vol = _volume(values, (0.0, 0.0, 0.0), 0.05)
    flags = vol.block_flags.cpu().numpy().reshape(3, 3, 3)
    assert flags.sum() == 1 and flags[2, 2, 2] == 1
    on, off = fusion.extract_mesh(vol, use_block_flags=True), fusion.extract_mesh(vol, use_block_flags=False)
    assert on["faces"].shape[0] > 8 and torch.equal(on["verts"], off["verts"]) and torch.equal(on["faces"], off["faces"])
    assert np.array_equal(on["faces"].cpu().numpy(), M.extract(values, (0, 0, 0), 0.05)["faces"])
    # an empty volume, and one that is known but has no crossing
    for vol in (fusion.TSDFVolume((9, 12, 70), 0.05, (0, 0, 0)), _volume(np.ones((9, 12, 70, 2), np.float32), (0, 0, 0), 0.05)):
        for flag in (True, False):
            e = fusion.extract_mesh(vol, return_weights=True, use_block_flags=flag)
            assert tuple(e["verts"].shape) == (0, 3) and tuple(e["faces"].shape) == (0, 3) and tuple(e["weights"].shape) == (0,)
            assert e["verts"].dtype == torch.float32 and e["faces"].dtype == torch.int32 and e["verts"].is_cuda


def test_emit_writes_nothing_beyond_the_capacities():
    from implicit_depth_amd import fusion

    values = M.sphere_volume((20, 20, 20), (9.3, 10.1, 8.7), 6.3)
    vol = _volume(values, (0.0, 0.0, 0.0), 0.05)
    full = fusion.extract_mesh(vol, return_weights=True)
    V, F = full["verts"].shape[0], full["faces"].shape[0]
    workspace, totals = fusion.mesh_count(vol)
    assert totals.tolist() == [V, F]
    extra = 5
    for vcap, fcap in ((V - 1, F - 1), (V // 2, 7), (0, F), (V, 0)):
        verts = torch.full((V + extra, 3), -777.0, device="cuda")
        weights = torch.full((V + extra,), -777.0, device="cuda")
        faces = torch.full((F + extra, 3), -5, device="cuda", dtype=torch.int32)
        fusion.mesh_emit(vol, workspace, verts, faces, weights, vert_capacity=vcap, face_capacity=fcap)
        assert torch.equal(verts[:vcap], full["verts"][:vcap]) and torch.equal(weights[:vcap], full["weights"][:vcap])
        assert torch.equal(faces[:fcap], full["faces"][:fcap])
        assert (verts[vcap:] == -777.0).all() and (weights[vcap:] == -777.0).all() and (faces[fcap:] == -5).all()


def _plane_field(dims):
    """T = 0.75 - x / 64 - y / 128 - z / 16 at the voxels: dyadic coefficients, so the float32 values are the linear field exactly."""
    zz, yy, xx = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in dims), indexing="ij")
    values = np.ones((*dims, 2), np.float32)
    values[..., 0] = 0.75 - xx / 64 - yy / 128 - zz / 16
    return values, np.array([-1 / 64, -1 / 128, -1 / 16]), 0.75


def test_oblique_plane_vertices_render_and_ray_cast_agree_with_the_closed_form():
    from implicit_depth_amd import fusion, raster

    dims, v, origin = (24, 28, 32), 0.05, np.array([-0.8, -0.7, 1.0], np.float32)
    values, grad, c0 = _plane_field(dims)
    vol = _volume(values, origin, v)
    mesh = fusion.extract_mesh(vol)
    verts = mesh["verts"].cpu().numpy().astype(np.float64)
    assert len(verts) > 1000
    bound = M.position_bound(origin, np.float32(v), dims)
    v64, o64 = float(np.float32(v)), origin.astype(np.float64)
    g = (verts - o64) / v64
    res = np.abs(g @ grad + c0)
    print(f"plane: {len(verts)} vertices, max residual {res.max():.3e} voxel-units of T (bound {np.abs(grad).sum() * bound / v64:.3e})")
    assert res.max() <= np.abs(grad).sum() * bound / v64
    # the closed form in a live camera: the ray t + s R q, q = invK (j + 0.5, i + 0.5, 1), meets T = 0 at depth s
    E = R._f32(R._pose(0.05, -0.03, 0.04, (0.02, -0.01, 0.0)))
    K = R._f32(R._pinhole(40.0, 40.0, 22.3, 14.6))
    iK = R._f32(np.linalg.inv(K.astype(np.float64)))
    H, W = 30, 44
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    q = np.stack([jj + 0.5, ii + 0.5, np.ones((H, W))], -1) @ iK.astype(np.float64)[:3, :3].T
    d = q @ E.astype(np.float64)[:3, :3].T
    t = E.astype(np.float64)[:3, 3]
    s = -(((t - o64) / v64) @ grad + c0) / ((d / v64) @ grad)
    hit = (t + s[..., None] * d - o64) / v64
    interior = ((hit > 2.5) & (hit < np.array(dims[::-1]) - 3.5)).all(-1) & (s > 0.4)
    want = s * q[..., 2]
    assert interior.sum() > 0.3 * H * W
    cam_T_world = R._f32(np.linalg.inv(E.astype(np.float64)))
    rendered = raster.render_depth(mesh["verts"], mesh["faces"], _cuda(cam_T_world)[None], _cuda(K)[None], H, W)[0, 0].cpu().numpy().astype(np.float64)
    cast = fusion.raycast_volume(vol, _cuda(E), _cuda(iK), (H, W), near=0.3, max_steps=60)
    depth = cast["depth"][0, 0].cpu().numpy().astype(np.float64)
    assert ((cast["flags"][0].cpu().numpy() & R.HIT) > 0)[interior].all() and (rendered[interior] > 0).all()  # no hole in either
    rel_mesh, rel_cast = (np.abs(rendered - want) / want)[interior].max(), (np.abs(depth - want) / want)[interior].max()
    print(f"plane: {interior.sum()} interior pixels, mesh render {rel_mesh:.2e}, ray cast {rel_cast:.2e} from the closed form")
    assert rel_mesh < 1e-4 and rel_cast < 1e-4


def test_sphere_with_an_unknown_block_has_its_boundary_exactly_at_the_unknown_cells():
    dims = (20, 20, 20)
    values = M.sphere_volume(dims, (9.3, 10.1, 8.7), 6.3)
    values[:8, :8, :8, 1] = 0
    got, ref = _check(values, (0.0, 0.0, 0.0), 0.05, what="sphere with a hole")
    faces, V = got["faces"].cpu().numpy().astype(np.int64), len(ref["verts"])
    keys, counts, rcounts = M.directed_edges(faces, V)
    assert (counts == 1).all() and (rcounts <= 1).all()  # no edge more than once each way
    boundary = set(keys[rcounts == 0].tolist())
    assert len(boundary) > 10
    # from the reference's bookkeeping: a face edge whose two vertices lie in one cube face of the face's cell is open iff the cell
    # across that cube face is not known (an in-face fan diagonal, closed inside its own cell, is not)
    Nz, Ny, Nx = dims
    known = np.zeros((Nz + 1, Ny + 1, Nx + 1), bool)  # known[z + 1, y + 1, x + 1]; False outside the grid of cells
    known[1:Nz, 1:Ny, 1:Nx] = ref["known"]
    cell = np.stack([ref["cell"] % Nx, (ref["cell"] // Nx) % Ny, ref["cell"] // (Nx * Ny)], 1)  # (F, 3) as (x, y, z)
    own = np.stack([ref["owner"] % Nx, (ref["owner"] // Nx) % Ny, ref["owner"] // (Nx * Ny)], 1)
    same_cell = set()
    for k in range(3):
        same_cell |= set((ref["cell"] * V * V + faces[:, k] * V + faces[:, (k + 1) % 3]).tolist())
    expected = set()
    for k in range(3):
        a, b = faces[:, k], faces[:, (k + 1) % 3]
        la, lb = own[a] - cell, own[b] - cell  # the owners' corners of the cell, in {0, 1}^3
        assert la.min() >= 0 and la.max() <= 1
        for axis in range(3):
            shared = (ref["axis"][a] != axis) & (ref["axis"][b] != axis) & (la[:, axis] == lb[:, axis])
            nb = cell.copy()
            nb[:, axis] += 2 * la[:, axis] - 1
            open_ = shared & ~known[nb[:, 2] + 1, nb[:, 1] + 1, nb[:, 0] + 1]
            closed_inside = np.array([(c * V * V + y * V + x) in same_cell for c, x, y in zip(ref["cell"].tolist(), a.tolist(), b.tolist())])
            expected |= set((a * V + b)[open_ & ~closed_inside].tolist())
    assert boundary == expected
