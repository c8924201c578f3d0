"""Surface normals in a live sequence: StreamingSession.normals_for_view / raycast_view_normals are, bit for bit, the session's own depth
queries followed by geometry.depth_normals / patch_normals, single- and multi-key; dropin.convert(native_normals=True) puts the fused
kernel behind a DepthModel's compute_normals.  The smallest model the streaming tests use (tests/test_ray_query_gpu.py)."""
import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import normals_ref as NR
from test_ray_query_gpu import _frame, _model, BUFFER
from test_view_search_gpu import _thresholder

pytestmark = pytest.mark.gpu
H, W = 30, 40
_SESSIONS = {}


def _session(query_keyframes):
    """A session stepped through seven frames of the pan the other streaming tests use: the camera has moved, at least three predictions
    were made, and on the last frame step() returned None.  Built once per ring size and shared; the queries do not change it."""
    if query_keyframes not in _SESSIONS:
        from implicit_depth_amd.streaming import StreamingSession

        poses, dists = syn.keyframe_trajectory("stream12", seed=0)
        s = StreamingSession(_model("mlp", 3), buffer_size=BUFFER, query_keyframes=query_keyframes)
        predicted = 0
        for t in range(7):
            out, _ = s.step(_frame(t, poses), world_T_cam=poses[t], dist_to_last_valid=dists[t])
            predicted += out is not None
        assert out is None and predicted >= 2
        invK = torch.linalg.inv(syn.intrinsics(W, H)).float()
        invK[:2, :3] *= 2.0  # a lens half as long as the keyframe's: the border of the live image looks past the keyframe's
        _SESSIONS[query_keyframes] = (s, poses[6], invK.cuda())
    return _SESSIONS[query_keyframes]


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), what


@pytest.mark.parametrize("first_hit", [None, dict(samples=9, refine=4)], ids=["search", "first_hit"])
@pytest.mark.parametrize("query_keyframes", [1, 2])
def test_normals_for_view_is_the_depth_query_plus_the_kernel(query_keyframes, first_hit):
    from implicit_depth_amd import geometry

    s, live, invK = _session(query_keyframes)
    th, fill = _thresholder(), 6.0
    got = s.normals_for_view(live, invK, (H, W), thresholder=th, fill=fill, smoothing_kernel_size=3, smoothing_kernel_std=1.5, first_hit=first_hit)
    if first_hit is None:
        want, pre = s.depth_for_view(live, invK, (H, W), thresholder=th, fill=fill), "view_search"
    else:
        want, pre = s.first_hit_for_view(live, invK, (H, W), thresholder=th, fill=fill, **first_hit), "view_march"
    assert set(got) == set(want) | {"view_normals", "view_normals_valid"} and (pre + "_key" in got) == (query_keyframes > 1)
    for k, v in want.items():
        _same(got[k], v, k)
    T = torch.from_numpy(live.astype(np.float32)).cuda()[None]
    n, valid = geometry.depth_normals(want[pre + "_depths"], invK[None], kernel_size=3, std=1.5, world_R_cam=T[:, :3, :3], orient=True,
                                      flags=want[pre + "_flags"], need=3)
    _same(got["view_normals"], n, "view_normals")
    _same(got["view_normals_valid"], valid, "view_normals_valid")
    assert tuple(n.shape) == (1, 3, H, W) and tuple(valid.shape) == (1, 1, H, W) and valid.dtype == torch.uint8
    ok = valid[0, 0].bool()
    share = ok.float().mean().item()
    print(f"query_keyframes={query_keyframes} {pre}: valid normals {share:.3f}, flags == 3 {(want[pre + '_flags'] == 3).float().mean().item():.3f}")
    assert 0.0 < share < 1.0  # some of both: the wide lens looks past the keyframe's image
    length = n[0].norm(dim=0)
    assert bool(((length[ok] - 1).abs() < 1e-5).all()) and bool((n[0][:, ~ok] == 0).all())
    # world-space normals face the live camera: n . (point - camera centre) <= 0, up to the rounding of the rotation
    view = want[pre + "_points"][0, 0].permute(2, 0, 1) - T[0, :3, 3].view(3, 1, 1)
    assert bool(((view * n[0]).sum(0)[ok] <= 1e-5 * view.norm(dim=0)[ok]).all())
    # the defaults are the reference NormalGenerator's: kernel size 5, std 2.0
    dflt = s.normals_for_view(live, invK, (H, W), thresholder=th, fill=fill, first_hit=first_hit)
    n5, _ = geometry.depth_normals(want[pre + "_depths"], invK[None], kernel_size=5, std=2.0, world_R_cam=T[:, :3, :3], orient=True,
                                   flags=want[pre + "_flags"], need=3)
    _same(dflt["view_normals"], n5, "view_normals (defaults)")


@pytest.mark.parametrize("query_keyframes", [1, 2])
def test_raycast_view_normals_is_one_raycast_of_nine_rays_plus_the_patch_kernel(query_keyframes):
    from implicit_depth_amd import geometry
    from implicit_depth_amd._lib import IdhError
    from implicit_depth_amd.streaming import patch_rays

    s, live, invK = _session(query_keyframes)
    th, fill, step = _thresholder(), 6.0, 1.5
    g = torch.Generator().manual_seed(5)
    rays = (torch.rand(1, 37, 2, generator=g) * torch.tensor([W - 8.0, H - 8.0]) + 4.0).cuda()
    got = s.raycast_view_normals(rays, live, invK, step=step, thresholder=th, fill=fill)
    nine = patch_rays(rays, step)
    assert tuple(nine.shape) == (1, 9 * 37, 2) and torch.equal(nine.view(1, 37, 9, 2)[:, :, 4], rays)
    off = (nine.view(1, 37, 9, 2) - rays[:, :, None]).cpu()
    assert torch.allclose(off[0, 0], torch.tensor([[x, y] for y in (-step, 0, step) for x in (-step, 0, step)]), atol=1e-5)
    all9 = s.raycast_view(nine, live, invK, thresholder=th, fill=fill)
    T = torch.from_numpy(live.astype(np.float32)).cuda()[None]
    n, valid = geometry.patch_normals(all9["view_search_points"].view(1, 37, 9, 3), cam_centre=T[:, :3, 3], orient=True,
                                      flags=all9["view_search_flags"].view(1, 37, 9), need=3)
    _same(got["view_normals"], n, "view_normals")
    _same(got["view_normals_valid"], valid, "view_normals_valid")
    assert tuple(n.shape) == (1, 37, 3) and tuple(valid.shape) == (1, 37)
    centre = s.raycast_view(rays, live, invK, thresholder=th, fill=fill)
    assert set(got) == set(centre) | {"view_normals", "view_normals_valid"}
    for k, v in centre.items():  # the centre ray's depth, point, flags (and key) are raycast_view's on the original rays
        _same(got[k], v, k)
    ok = valid[0].bool()
    print(f"query_keyframes={query_keyframes}: {int(ok.sum())} of 37 hit tests have a normal")
    assert bool(ok.any()) and bool((n[0][~ok] == 0).all()) and bool(((n[0][ok].norm(dim=-1) - 1).abs() < 1e-5).all())
    view = centre["view_search_points"][0] - T[0, :3, 3]
    assert bool(((view * n[0]).sum(-1)[ok] <= 1e-5 * view.norm(dim=-1)[ok]).all())
    with pytest.raises(IdhError, match="rays"):
        s.raycast_view_normals(rays[0], live, invK)


def test_converted_depth_model_computes_normals_natively():
    """A DepthModel-shaped module: convert(native_normals=True) replaces compute_normals by the native module of the same height, width,
    size and std, whose output on a predicted depth is the contract's; without the flag the module is untouched."""
    import hot_helpers
    from implicit_depth_amd import dropin, geometry

    h, w, k, std = 48, 64, 5, 2.0

    class RefNormals(torch.nn.Module):  # the attributes of the reference's NormalGenerator (utils/geometry_utils.py:104-110)
        def __init__(self):
            super().__init__()
            self.height, self.width, self.kernel_size, self.std = h, w, k, std
            self.backproject = geometry.BackprojectDepth(h, w)

        def forward(self, depth_b1hw, invK_b44):
            raise RuntimeError("kornia is not installed")

    m = hot_helpers.holder(2, "dot", 12, 16, 8, decoder="depth", with_mlp=False)
    m.compute_normals = ref_module = RefNormals()
    m = m.cuda()
    assert dropin.convert(m).compute_normals is ref_module
    dropin.convert(m, native_normals=True)
    assert isinstance(m.compute_normals, geometry.NormalGenerator) and list(m.compute_normals.state_dict()) == list(ref_module.state_dict())
    assert m.compute_normals.backproject.pix_coords_13N.is_cuda
    depth, invK = NR.field(2, h, w), NR.inv_intrinsics(2, h, w)
    got = m.compute_normals(depth.cuda(), invK.cuda())  # depth_model.py:565-570
    ref, _, _ = NR.dense(depth, invK, k, std)
    comp = NR.max_err(NR.composition(depth, invK, k, std), ref)
    assert tuple(got.shape) == (2, 3, h, w) and NR.max_err(got.cpu().numpy(), ref) <= max(NR.FACTOR * comp, NR.FLOOR)
