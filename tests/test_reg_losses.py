"""DepthModel's validation losses without a GPU (include/idh_geometry.h: idh_reg_val_losses_fwd): the torch fp32
composition of tests/reg_losses_ref.py against golden G18 (the reference's own compute_losses on the restated kornia functions), the
fp64 restatement against the composition, the properties of the fixture the GPU tests rely on, and the host side of the C ABI: the symbols
are bound and every IDH_EINVAL / IDH_EWORKSPACE case returns before a launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import mv_consistency_ref as MV
import reg_losses_ref as R
from conftest import load_golden

EPS32 = float(np.finfo(np.float32).eps)
CASES = [("scannet", "all"), ("scannet", "s0"), ("hypersim", "all"), ("hypersim", "s0")]


def _case(dataset, sname, g=None):
    g = load_golden("g18_reg_losses") if g is None else g
    B, H, W, K = (int(v) for v in g["shape"])
    return R.inputs(B, H, W, K, scales=(0, 1, 2, 3) if sname == "all" else (0,)), g[f"{dataset}_{sname}"]


@pytest.mark.parametrize("dataset,sname", CASES)
def test_composition_reproduces_the_reference_golden_exactly(dataset, sname):
    (cur, src, outputs), gold = _case(dataset, sname)
    got = R.compute_losses32(cur, src, outputs, dataset == "hypersim")
    assert np.array_equal(np.array([float(got[k]) for k in R.KEYS], dtype=np.float32), gold)
    assert np.isfinite(gold).all() and gold.dtype == np.float32


@pytest.mark.parametrize("dataset,sname", CASES)
def test_fp64_restatement_agrees_with_the_composition(dataset, sname):
    """Each value is an O(1) mean of a few hundred to a few thousand fp32 terms of one sign, summed pairwise by torch: 8 eps relative covers
    the rounding of the terms, of the sum and of the fp32 cocktail."""
    (cur, src, outputs), gold = _case(dataset, sname)
    ref, counts = R.losses64(cur, src, outputs, dataset == "hypersim")
    for k, v in zip(R.KEYS, gold):
        print(f"{dataset} {sname} {k}: fp32 {v:.9g} fp64 {ref[k]:.12g}")
        assert abs(float(v) - ref[k]) <= 8 * EPS32 * abs(ref[k]), k
    if dataset == "hypersim":
        assert ref["grad_loss"] == 0 and ref["normals_loss"] == 0 and ref["mv_loss"] == 0 and ref["loss"] == ref["ms_loss"]
        assert counts["normals"] == 0 and counts["grad_s0"] == 0
    else:
        assert all(counts[k] > 0 for k in R.COUNT_KEYS) and counts["mask_b_limit"] < counts["mask_b"]


@pytest.mark.parametrize("shape", [(2, 24, 32), (1, 21, 27), (3, 40, 72)], ids=lambda s: "x".join(map(str, s)))
def test_fixture_properties(shape):
    """What the GPU tests take for granted: no predicted depth within rounding of the 0.1 threshold, no multi-view projection within
    rounding of a tap border or a gate threshold, NaNs in the ground truth and in both normal maps, finite gradients at every level."""
    B, h, w = shape
    cur, src, outputs = R.inputs(B, h, w, 2, scales=(0,) if h % 8 else (0, 1, 2, 3))
    pred, gt = outputs["depth_pred_s0_b1hw"], cur["depth_b1hw"]
    assert not ((pred > 0.09) & (pred < 0.11)).any() and (pred == R.STRIP).any() and torch.isfinite(pred).all()
    assert torch.isnan(gt).any() and (cur["mask_b_b1hw"] & ~torch.isfinite(gt)).sum() == 0
    assert (torch.isfinite(gt) & ~cur["mask_b_b1hw"]).any()
    assert torch.isnan(cur["normals_b3hw"]).any() and torch.isnan(outputs["normals_pred_b3hw"]).any()
    chk = MV.check(pred, cur["invK_s0_b44"], cur["world_T_cam_b44"], src["depth_b1hw"], src["K_s0_b44"], src["cam_T_world_b44"], gate_depth=gt)
    assert not chk["ambiguous_pixel"].any() and (chk["loss_count"] > 0).all() and np.isfinite(chk["loss"])
    sizes = R.pyramid_sizes(h, w)
    levels = R.grad_levels64(gt, pred)
    for (hl, wl), (mean, n) in zip(sizes, levels):
        assert 0 < n < 2 * B * hl * wl and np.isfinite(mean)
    if shape == (1, 21, 27):
        assert sizes == [(21, 27), (11, 14), (6, 7), (3, 4)]


def test_restated_kornia_functions():
    """blur_pool2d: output size ceil(H/2) x ceil(W/2), a constant image keeps its value away from the zero padding and loses the padded
    share at it, one NaN poisons exactly the outputs whose 3x3 window holds it; spatial_gradient: a ramp has gradient (1, 0) up to the
    replicated border, where it halves, and one NaN makes its whole 3x3 neighbourhood NaN in both components - zero taps included."""
    x = torch.full((1, 1, 7, 9), 2.0)
    b = R.blur_pool32(x)
    assert b.shape == (1, 1, 4, 5) and torch.equal(b[0, 0, 1:3, 1:4], torch.full((2, 3), 2.0))
    assert b[0, 0, 0, 0] == 2.0 * 9 / 16 and b[0, 0, 3, 2] == 2.0 * 12 / 16  # row 7 is padding for an odd H
    assert np.array_equal(R.blur_pool64(x[:, 0].double().numpy()), b[:, 0].double().numpy())
    x[0, 0, 3, 4] = float("nan")
    assert torch.isnan(R.blur_pool32(x))[0, 0].nonzero().tolist() == [[1, 2], [2, 2]]  # rows 2Y-1 .. 2Y+1 hold 3 for Y = 1, 2; columns for X = 2
    assert np.array_equal(np.isnan(R.blur_pool64(x[:, 0].double().numpy())), torch.isnan(R.blur_pool32(x))[:, 0].numpy())
    ramp = torch.arange(9.0).expand(1, 1, 7, 9).contiguous()
    g = R.spatial_gradient32(ramp)
    assert torch.equal(g[0, 0, 0, :, 1:-1], torch.ones(7, 7)) and torch.equal(g[0, 0, 0, :, 0], torch.full((7,), 0.5)) and (g[0, 0, 1] == 0).all()
    ramp[0, 0, 3, 4] = float("inf")
    bad = ~torch.isfinite(R.spatial_gradient32(ramp))[0, 0]
    want = torch.zeros(7, 9, dtype=torch.bool)
    want[2:5, 3:6] = True
    assert torch.equal(bad[0], want) and torch.equal(bad[1], want)
    gx, gy = R.spatial_gradient64(ramp[:, 0].double().numpy())
    assert np.array_equal(~np.isfinite(gx[0]), want.numpy()) and np.array_equal(~np.isfinite(gy[0]), want.numpy())


def test_means_of_nothing_are_nan_in_both_forms():
    cur, src, outputs = R.inputs(2, 24, 32, 2)
    cur["mask_b_b1hw"] = torch.zeros_like(cur["mask_b_b1hw"])
    comp, (ref, counts) = R.compute_losses32(cur, src, outputs), R.losses64(cur, src, outputs)
    for k in ("ms_loss", "abs_loss", "si_loss", "inv_abs_loss", "log_l1_loss", "loss"):
        assert np.isnan(float(comp[k])) and np.isnan(ref[k]), k
    assert counts["mask_b"] == 0 and np.isfinite(ref["grad_loss"]) and np.isfinite(float(comp["normals_loss"]))
    cur, src, outputs = R.inputs(2, 24, 32, 2)
    cur["depth_b1hw"] = torch.full_like(cur["depth_b1hw"], float("nan"))
    assert np.isnan(float(R.grad_loss32(cur["depth_b1hw"], outputs["depth_pred_s0_b1hw"])))
    assert all(n == 0 and np.isnan(m) for m, n in R.grad_levels64(cur["depth_b1hw"], outputs["depth_pred_s0_b1hw"]))


# ---- the C ABI, host side --------------------------------------------------------------------------------------------------------------
NAMES = ("idh_reg_val_losses_fwd", "idh_reg_val_losses_workspace_bytes", "idh_sizeof_reg_val_losses_args")
FAKE = 0x10000  # a non-null, 8-byte aligned pointer that is never dereferenced: every call below returns before a launch


def test_header_symbols_are_bound():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.declared_symbols() and hasattr(L, name)
    assert L.idh_sizeof_reg_val_losses_args() == C.sizeof(_lib.RegValLossesArgs) == _lib.RegValLossesArgs().struct_size


def _align(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("shape", [(2, 24, 32), (1, 21, 27), (3, 40, 72), (32, 192, 256), (1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_workspace_size_formula(shape):
    """Levels 1 .. 3 of both pyramids as doubles, each map rounded up to 256 bytes, then per level the tile records: 16 doubles per 32 x 32
    tile of level 0, 2 per tile above."""
    from implicit_depth_amd import _lib

    B, h, w = shape
    sizes = R.pyramid_sizes(h, w)
    want = sum(2 * _align(8 * B * hl * wl) for hl, wl in sizes[1:])
    want += sum(_align(8 * (2 if l else 16) * B * -(-hl // 32) * -(-wl // 32)) for l, (hl, wl) in enumerate(sizes))
    L = _lib.lib()
    assert L.idh_reg_val_losses_workspace_bytes(B, h, w) == want
    for bad in ((0, h, w), (B, 0, w), (B, h, -1)):
        assert L.idh_reg_val_losses_workspace_bytes(*bad) == 0


def _args(**kw):
    from implicit_depth_amd import _lib

    a = _lib.RegValLossesArgs()
    a.depth_gt_b1hw = a.depth_pred_b1hw = a.mask_b_b1hw = a.normals_gt_b3hw = a.normals_pred_b3hw = a.out16 = a.workspace = FAKE
    a.B, a.h, a.w, a.si_lambda = 2, 24, 32, 0.85
    a.workspace_bytes = _lib.lib().idh_reg_val_losses_workspace_bytes(2, 24, 32)
    scales = kw.pop("scales", {0: (24, 32), 1: (12, 16), 2: (6, 8), 3: (3, 4)})
    for i, (sh, sw) in scales.items():
        a.log_depth_pred_s[i], a.scale_h[i], a.scale_w[i] = FAKE, sh, sw
    for k, v in kw.items():
        setattr(a, k, v)
    return a


GRAD, POINT, NORMALS = 1, 2, 4
EINVAL = [dict(struct_size=8), dict(out16=None), dict(B=-1), dict(h=0), dict(w=0), dict(h=-3), dict(max_workgroups=-1), dict(num_scales=5),
          dict(num_scales=-1), dict(terms=8), dict(terms=-1), dict(si_lambda=float("nan")), dict(depth_gt_b1hw=None), dict(depth_pred_b1hw=None),
          dict(mask_b_b1hw=None), dict(normals_gt_b3hw=None), dict(normals_pred_b3hw=None), dict(scales={}), dict(scales={1: (12, 16)}),
          dict(scales={0: (24, 32), 1: (0, 16)}), dict(scales={0: (24, 32), 2: (6, -8)}), dict(scales={0: (24, 32), 1: (10, 16)}),
          dict(scales={0: (24, 32), 3: (3, 5)}), dict(scales={0: (48, 64)}), dict(scales={0: (16, 32)}), dict(out16=FAKE + 4),
          dict(workspace=FAKE + 4), dict(terms=GRAD, depth_gt_b1hw=None), dict(terms=NORMALS, normals_pred_b3hw=None),
          dict(terms=POINT, hypersim=1, mask_b_b1hw=None), dict(B=0, out16=None), dict(B=0, scales={})]
EWORKSPACE = [dict(workspace=None), dict(workspace_bytes=0), dict(workspace=None, workspace_bytes=0)]


def test_every_einval_and_eworkspace_case_returns_before_a_launch():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert L.idh_reg_val_losses_fwd(None, None) == -1
    for kw in EINVAL:
        assert L.idh_reg_val_losses_fwd(_args(**kw), None) == -1, kw
    code = {L.idh_reg_val_losses_fwd(_args(**kw), None) for kw in EWORKSPACE}
    short = _args()
    short.workspace_bytes -= 1
    code.add(L.idh_reg_val_losses_fwd(short, None))
    assert len(code) == 1 and code != {0} and code != {-1}
    assert b"workspace" in L.idh_error_string(code.pop()).lower()
    # B == 0 succeeds without a launch (no GPU is touched here) and needs no workspace; what the terms leave out may be NULL
    assert L.idh_reg_val_losses_fwd(_args(B=0), None) == 0
    assert L.idh_reg_val_losses_fwd(_args(B=0, workspace=None, workspace_bytes=0), None) == 0
    assert L.idh_reg_val_losses_fwd(_args(B=0, hypersim=1, normals_gt_b3hw=None, normals_pred_b3hw=None, mv_loss=None), None) == 0
    assert L.idh_reg_val_losses_fwd(_args(B=0, terms=GRAD, mask_b_b1hw=None, normals_gt_b3hw=None, scales={}), None) == 0
    assert L.idh_reg_val_losses_fwd(_args(B=0, terms=NORMALS, depth_gt_b1hw=None, depth_pred_b1hw=None, mask_b_b1hw=None, scales={}), None) == 0


def test_python_surface_refuses_what_it_cannot_run():
    from implicit_depth_amd import dropin, evaluation, geometry, losses
    from implicit_depth_amd._lib import IdhError

    cur, src, outputs = R.inputs(2, 24, 32, 2)
    with pytest.raises(IdhError, match="CPU"):
        evaluation.reg_val_losses(outputs, cur, hypersim=True)
    with pytest.raises(IdhError, match="CPU"):
        losses.MSGradientLoss()(cur["depth_b1hw"], outputs["depth_pred_s0_b1hw"])
    with pytest.raises(IdhError, match="CPU"):
        losses.NormalsLoss()(cur["normals_b3hw"], outputs["normals_pred_b3hw"])
    with pytest.raises(IdhError, match="Could not find a valid scale to compute si loss!"):
        evaluation.reg_val_losses({k: v for k, v in outputs.items() if not k.startswith("log_")}, cur, src)
    with pytest.raises(IdhError, match="src_data"):
        evaluation.reg_val_losses(outputs, cur)
    with pytest.raises(IdhError, match="compute_normals=True"):
        evaluation.reg_val_losses({k: v for k, v in outputs.items() if k != "normals_pred_b3hw"}, cur, src)
    with pytest.raises(IdhError, match="num_scales"):
        losses.MSGradientLoss(5)
    with pytest.raises(IdhError, match="num_scales"):
        losses.MSGradientLoss(0)
    assert losses.MVDepthLoss is geometry.MVDepthLoss and losses.MSGradientLoss().num_scales == 4

    class Ref(torch.nn.Module):
        num_scales, height, width = 3, 24, 32

    import hot_helpers

    m = hot_helpers.holder(2, "dot", 4, 4, 4, decoder="depth", with_mlp=False)
    assert dropin.convert(m, native_losses=True) is m and not hasattr(m, "grad_loss")  # a model without the attributes is left alone
    m.grad_loss, m.normals_loss, m.mv_depth_loss = refs = (Ref(), Ref(), Ref())
    dropin.convert(m)
    assert (m.grad_loss, m.normals_loss, m.mv_depth_loss) == refs  # only with the flag
    dropin.convert(m, native_losses=True)
    new = (m.grad_loss, m.normals_loss, m.mv_depth_loss)
    assert isinstance(new[0], losses.MSGradientLoss) and isinstance(new[1], losses.NormalsLoss) and isinstance(new[2], losses.MVDepthLoss)
    assert new[0].num_scales == 3 and (new[2].height, new[2].width) == (24, 32)
    dropin.convert(m, native_losses=True)
    assert (m.grad_loss, m.normals_loss, m.mv_depth_loss) == new  # idempotent
