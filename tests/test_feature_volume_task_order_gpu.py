"""fv_mlp_k<KT, true> hands its tasks to the waves in a rotated order (csrc/feature_volume.hip: fv_skip_task; the order itself:
tests/test_fv_task_map_cpu.py).  The order must not change a bit of any output: the kernel forced (idh_volume_opts.fv_keep_empty_views = 2)
against fv_mlp_k<KT, false> forced (= 1), which keeps the static order - volume, lowest_cost and mask bit-identical - on shapes with several rounds, a
partial last round, a grid below 256 workgroups, more than one plane group, and NHWC stores.  The cameras are synthetic.cost_volume_inputs':
their intrinsics scale with the image, so at every size some (tile, plane, view) groups are dropped and others kept (asserted on the CPU)."""
import ctypes
import functools
import math

import pytest
import torch

import implicit_depth_amd.synthetic as syn
from conftest import TOL, rel_err
from implicit_depth_amd import _lib
from oracle import cost_volume as ocv

C = 16
DMIN, DMAX = 0.25, 5.0
# (B, K, H, W, D)
RAGGED = (3, 7, 96, 128, 8)     # fv_mlp_k<7, true>: more than one round of 2048 tasks, the last one partial
SMALL = (2, 8, 10, 24, 5)       # fv_mlp_k<8, true>: 15 tiles per image, one partial round on 4 workgroups, the last of them with 6 of 8 tasks
RUNTIME_K = (12, 4, 48, 64, 16)  # fv_mlp_k<0, true>: several rounds
NHWC = (2, 7, 24, 40, 8)        # NHWC stores (12 channels per pixel for 8 planes), mask on


def _tasks(shape):
    """(ntasks, grid, groups) of a launch, from the functions the launch calls."""
    B, K, H, W, D = shape
    L = _lib.lib()
    g, dp = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(L.idh_feature_volume_plane_groups(B, H, W, D, ctypes.byref(g), ctypes.byref(dp)), "idh_feature_volume_plane_groups")
    ntasks = B * ((H * W + 15) // 16) * g.value
    return ntasks, L.idh_feature_volume_grid(ntasks), g.value


def _outside_groups(inp, H, W, D):
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
def _case(shape):
    """Inputs and MLP of one case (computed once, shared by the tests, never modified)."""
    from implicit_depth_amd.cost_volume import FeatureVolumeManager

    B, K, H, W, D = shape
    inp = syn.cost_volume_inputs(B, K, C, H, W, seed=11 + K)
    m = FeatureVolumeManager(H, W, D, mlp_channels=[16 * (K + 1) + 10 * K + 4, 128, 128, 1], num_source_views=K, matching_dim_size=C)
    syn.fill_state_dict(m.mlp, seed=70 + K, gain=1.4)
    w = {k: v.detach().cpu().double() for k, v in m.mlp.state_dict().items()}  # (taken here: the tests move the module to the GPU in place)
    return inp, m, w


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    B, K, H, W, D = shape
    inp, _, w = _case(shape)
    d = {k: v.double() for k, v in inp.items()}
    return ocv.feature_volume(d["cur_feats"], d["src_feats"], d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"], DMIN, DMAX, D, w,
                              return_mask=True)


@pytest.mark.parametrize("shape", [RAGGED, SMALL, RUNTIME_K, NHWC])
def test_cases_drop_some_groups_and_keep_others(shape):
    """A condition on the inputs (no GPU): task costs differ within each case."""
    B, K, H, W, D = shape
    share = _outside_groups(_case(shape)[0], H, W, D)
    assert 0.05 < share < 0.95, share


def test_cases_have_the_rounds_they_are_here_for():
    """A condition on the launches (no GPU), from idh_feature_volume_plane_groups and idh_feature_volume_grid."""
    n, grid, _ = _tasks(RAGGED)
    assert grid == 256 and n > grid * 8 and n % (grid * 8) != 0  # more than one round, and the last one is not full
    n, grid, G = _tasks(SMALL)
    assert (n, grid, G) == (30, 4, 1)  # one round; the last workgroup holds 6 of its 8 tasks
    n, grid, _ = _tasks(RUNTIME_K)
    assert grid == 256 and n >= 3 * grid * 8
    n, grid, G = _tasks(NHWC)
    assert (n, grid, G) == (240, 30, 2)  # two plane groups per tile, a grid that is no multiple of 8 (the XCD remap's uneven split)


def _both(shape, return_mask=True):
    inp, m, _ = _case(shape)
    m = m.cuda()
    d = {k: v.cuda() for k, v in inp.items()}
    outs = {}
    try:
        for mode in ("always", False):
            m.skip_empty_views = mode
            fv, low, planes, mask = m(**d, return_mask=return_mask)
            outs[mode] = (fv.cpu(), low.cpu(), mask.cpu())
    finally:
        m.skip_empty_views = True
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [RAGGED, SMALL, RUNTIME_K])
def test_rotated_order_changes_no_bit(shape):
    outs = _both(shape)
    for rot, static in zip(outs["always"], outs[False]):
        assert torch.equal(rot, static)
    assert torch.isfinite(outs["always"][0]).all()


@pytest.mark.gpu
def test_rotated_order_matches_oracle():
    """The first case against the fp64 oracle, at the bar of tests/test_feature_volume_gpu.py / test_feature_volume_skip_gpu.py."""
    ref, rlow, _, rmask = _oracle(RAGGED)
    fv, low, mask = _both(RAGGED)["always"]
    assert rel_err(fv, ref) < TOL
    assert (mask != rmask).float().mean().item() < 2e-3
    assert ((low.double() - rlow).abs() > 1e-5).float().mean().item() < 5e-3


@pytest.mark.gpu
def test_rotated_order_nhwc_and_mask():
    """NHWC output (vol_nhwc_cs = 12 > D = 8: the CVEncoder's input layout) with the mask on: the whole buffer, padding channels included."""
    from implicit_depth_amd import cost_volume as cv

    B, K, H, W, D = NHWC
    cs = 12
    inp, m, _ = _case(NHWC)
    m = m.cuda()
    d = {k: v.cuda() for k, v in inp.items()}
    cur_n, src_n = cv.to_nhwc(d["cur_feats"]), cv.to_nhwc(d["src_feats"])
    outs = {}
    try:
        for mode in ("always", False):
            m.skip_empty_views = mode
            vol = torch.full((B, H, W, cs), -7.0, device="cuda")
            low, _, mask = m._run(cur_n.data_ptr(), src_n.data_ptr(), (B, K, C, H, W), d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"],
                                  DMIN, DMAX, vol.data_ptr(), cs, True, vol.device, scratch={})
            torch.cuda.synchronize()
            outs[mode] = (vol.cpu(), low.cpu(), mask.cpu())
    finally:
        m.skip_empty_views = True
    for rot, static in zip(outs["always"], outs[False]):
        assert torch.equal(rot, static)
    vol = outs["always"][0]
    assert torch.isfinite(vol).all() and (vol[..., :D] != -7.0).all() and (vol[..., D:] == -7.0).all()
