"""fv_mlp_k<KT, true> drops, per 16-voxel tile and plane, the source views in which no voxel has a non-zero bilinear weight (csrc/feature_volume.hip,
DESIGN 4.3): its outputs must be bit-identical to those of fv_mlp_k<KT, false>, which processes every view (FeatureVolumeManager.skip_empty_views = "always" /
False -> idh_volume_opts.fv_keep_empty_views 2 / 1), so must those of the default, where each launch picks one of the two kernels, and all must
agree with the fp64 oracle at the bar of tests/test_feature_volume_gpu.py."""
import functools
import math

import pytest
import torch

import implicit_depth_amd.synthetic as syn
from conftest import TOL, rel_err
from oracle import cost_volume as ocv

B, C, D = 2, 16, 6
DMIN, DMAX = 0.25, 5.0
# three 16-pixel tiles per row; rows of 40: every other row starts in the middle of a tile, so tiles span two rows; 7 x 23 = 161 pixels: a ragged
# last tile, whose 15 clamped stand-in voxels take part in the ballot
MAPS = [(8, 48), (12, 40), (7, 23)]
VIEWS = [7, 8, 3]  # KT = 7, 8 and the run-time variant KT = 0 of fv_mlp_k<KT, false | true>
CAMERAS = ["identity", "sideways", "turned_away", "all_outside"]


def _poses(kind, K):
    """cur_T_src per view (4x4 fp64)."""
    out = []
    for k in range(K):
        T = torch.eye(4, dtype=torch.float64)
        if kind == "sideways":
            # pure translation along x, growing with the view: a point at depth d moves by fx * t / d = 0.903 W t / d pixels, so view k is
            # wholly outside for d <= 0.903 t_k, and leaves the image in the middle of a row on the planes behind that
            T[0, 3] = 0.4 * (k + 1)
        elif kind == "turned_away":
            T[0, 3] = 0.05 * (k + 1)
            if k == 1 % K:
                T = syn._rot_y(math.pi)  # at the current camera's place, looking the other way: every point is behind it (z clamp)
        elif kind == "all_outside":
            T[0, 3] = 100.0 + k
        out.append(T)
    return torch.stack(out)


def _outside_groups(inp, H, W):
    """Share of (16 consecutive pixels of the flattened map, plane, view) groups in which every sample has four zero bilinear weights, fp64 on the
    CPU: x outside (-1, W) or y outside (-1, H) after the -0.5 shift, z clamped to 1e-5 (prologue() of fv_mlp_k)."""
    Ks, E, iK = inp["src_Ks"].double(), inp["src_extrinsics"].double(), inp["cur_invK"].double()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=torch.float64)])
    depths = torch.exp(math.log(DMIN) + math.log(DMAX / DMIN) * torch.linspace(0, 1, D, dtype=torch.float64))
    P = Ks @ E
    q = P[:, :, :3, :3] @ iK[:, None, :3, :3] @ pix
    cam = depths.view(1, 1, -1, 1, 1) * q[:, :, None] + P[:, :, None, :3, 3:4]
    z = cam[..., 2, :].clamp_min(1e-5)
    sx, sy = cam[..., 0, :] / z - 0.5, cam[..., 1, :] / z - 0.5
    out = (sx <= -1) | (sx >= W) | (sy <= -1) | (sy >= H)
    pad = (-H * W) % 16
    if pad:
        out = torch.cat([out, out[..., -1:].expand(*out.shape[:-1], pad)], -1)
    return out.reshape(*out.shape[:-1], -1, 16).all(-1).double().mean().item()


@functools.lru_cache(maxsize=None)
def _case(H, W, K, kind):
    """Inputs, MLP weights and the fp64 oracle of one case (computed once, shared by the tests, never modified)."""
    from implicit_depth_amd.cost_volume import FeatureVolumeManager

    inp = syn.cost_volume_inputs(B, K, C, H, W, seed=3 + K)
    poses = _poses(kind, K).expand(B, K, 4, 4).contiguous()
    inp["src_poses"] = poses.float()
    inp["src_extrinsics"] = torch.linalg.inv(poses).float()
    m = FeatureVolumeManager(H, W, D, mlp_channels=[202, 128, 128, 1], num_source_views=K, matching_dim_size=C)
    syn.fill_state_dict(m.mlp, seed=50 + K, gain=1.4)
    w = {k: v.double() for k, v in m.mlp.state_dict().items()}
    d = {k: v.double() for k, v in inp.items()}
    ref = ocv.feature_volume(d["cur_feats"], d["src_feats"], d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"], DMIN, DMAX, D, w,
                             return_mask=True)
    return inp, m, ref


@pytest.mark.parametrize("shape", MAPS)
@pytest.mark.parametrize("K", VIEWS)
def test_cameras_cover_the_paths(shape, K):
    """A condition on the inputs (no GPU): nothing can be dropped with identity poses, everything with every view outside, and the sideways
    translation leaves between 20 % and 80 % of the (tile, plane, view) groups wholly outside, next to partially covered ones."""
    H, W = shape
    share = {kind: _outside_groups(_case(H, W, K, kind)[0], H, W) for kind in CAMERAS}
    assert share["identity"] == 0.0
    assert share["all_outside"] == 1.0
    assert 0.2 <= share["sideways"] <= 0.8, share
    assert 0.0 < share["turned_away"] < 1.0, share


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CAMERAS)
@pytest.mark.parametrize("shape", MAPS)
@pytest.mark.parametrize("K", VIEWS)
def test_dropping_views_changes_no_bit_and_matches_oracle(K, shape, kind):
    H, W = shape
    inp, m, (ref, rlow, _, rmask) = _case(H, W, K, kind)
    m = m.cuda()
    d = {k: v.cuda() for k, v in inp.items()}
    outs = {}
    for skip in ("always", True, False):
        m.skip_empty_views = skip
        fv, low, planes, mask = m(**d, return_mask=True)
        outs[skip] = (fv.cpu(), low.cpu(), mask.cpu())
        assert m(**d)[3] is None
    m.skip_empty_views = True
    for mode in ("always", True):
        for on, off in zip(outs[mode], outs[False]):
            assert torch.equal(on, off)
    for fv, low, mask in outs.values():
        assert rel_err(fv, ref) < TOL
        assert (mask != rmask).float().mean().item() < 2e-3
        assert ((low.double() - rlow).abs() > 1e-5).float().mean().item() < 5e-3
