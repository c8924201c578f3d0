"""evaluation.reg_val_losses, losses.MSGradientLoss / NormalsLoss and dropin.convert(native_losses=True) on the GPU (csrc/reg_losses.hip,
DESIGN.md §4.28) against tests/reg_losses_ref.py and golden G18.

Every value is held to two bounds: rtol 2e-6 of the golden (the reference's own fp32 result of an O(1) mean, itself within ~1e-6 relative
of the exact value; the bound tests/test_edge_mask_gpu.py uses for bd_val_losses), and FACTOR x the error of the torch fp32 composition
against the fp64 restatement (floor: FLOOR x the value's size).  The counts behind the means are integers and must be exact.  The shapes:
24x32 is one tile per image with a partial tile at every level above 0; 21x27 has an odd size at every level (the `ceil` sizes and the
zero-padded last row and column of the blur); 40x72 has 2 x 3 tiles of 32 x 32 at level 0 and 1 x 2 at level 1, the last of each
direction partial."""
import sys

import numpy as np
import pytest
import torch

import reg_losses_ref as R
from conftest import load_golden
from normals_ref import FACTOR, FLOOR

pytestmark = pytest.mark.gpu

ALL = (0, 1, 2, 3)
_cache = {}


def _case(B, h, w, scales=ALL, hypersim=False):
    """Inputs, the fp64 values and counts, and the fp32 composition's values of a case, computed once and left unchanged."""
    key = (B, h, w, scales, hypersim)
    if key not in _cache:
        cur, src, outputs = R.inputs(B, h, w, 2, scales=scales)
        ref, counts = R.losses64(cur, src, outputs, hypersim)
        comp = {k: float(v) for k, v in R.compute_losses32(cur, src, outputs, hypersim).items()}
        _cache[key] = (cur, src, outputs, ref, counts, comp)
    return _cache[key]


def _cuda(d):
    return None if d is None else {k: v.cuda() for k, v in d.items()}


def _run(cur, src, outputs, **kw):
    from implicit_depth_amd import evaluation

    out = evaluation.reg_val_losses(_cuda(outputs), _cuda(cur), _cuda(src), return_counts=True, **kw)
    assert sorted(k for k in out if k != "counts") == sorted(R.KEYS) and tuple(out["counts"]) == R.COUNT_KEYS
    assert all(out[k].dim() == 0 and out[k].dtype == torch.float32 and out[k].is_cuda for k in R.KEYS)
    return {k: out[k].cpu() for k in R.KEYS}, {k: int(v) for k, v in out["counts"].items()}


def _bits(vals):
    return [vals[k].view(torch.int32).item() for k in R.KEYS]


def _check(got, ref, comp, what):
    for k in R.KEYS:
        v, r, c = got[k].item(), ref[k], comp[k]
        if np.isnan(r):
            assert np.isnan(v) and np.isnan(c), (what, k)
            continue
        err_k, err_c = abs(v - r), abs(c - r)
        print(f"{what} {k}: {v:.9g} error {err_k:.3e} (composition {err_c:.3e})")
        assert err_k <= max(FACTOR * err_c, FLOOR * abs(r)), (what, k, v, r)


@pytest.mark.parametrize("dataset,scales", [("scannet", ALL), ("scannet", (0,)), ("hypersim", ALL), ("hypersim", (0,))],
                         ids=["scannet-all", "scannet-s0", "hypersim-all", "hypersim-s0"])
def test_reg_val_losses_golden_fp64_and_counts(dataset, scales):
    g = load_golden("g18_reg_losses")
    B, H, W, K = (int(v) for v in g["shape"])
    hyp = dataset == "hypersim"
    cur, src, outputs, ref, counts, comp = _case(B, H, W, scales, hyp)
    got, n = _run(cur, src, outputs, hypersim=hyp)
    gold = g[f"{dataset}_{'all' if scales == ALL else 's0'}"]
    vals = np.array([got[k].item() for k in R.KEYS], dtype=np.float32)
    np.testing.assert_allclose(vals, gold, rtol=2e-6, atol=0)
    _check(got, ref, comp, f"{dataset} {scales}")
    assert n == counts
    if hyp:  # the reference's literal zeros, and the cocktail is ms_loss alone
        assert got["grad_loss"].item() == 0 and got["normals_loss"].item() == 0 and got["mv_loss"].item() == 0
        assert torch.equal(got["loss"].view(torch.int32), got["ms_loss"].view(torch.int32))
        bare_cur = {k: v for k, v in cur.items() if k in ("depth_b1hw", "mask_b_b1hw")}
        bare_out = {k: v for k, v in outputs.items() if k != "normals_pred_b3hw"}
        again, n2 = _run(bare_cur, None, bare_out, hypersim=True)
        assert _bits(again) == _bits(got) and n2 == n


def test_odd_sizes_and_a_single_scale():
    B, h, w = 1, 21, 27
    assert R.pyramid_sizes(h, w) == [(21, 27), (11, 14), (6, 7), (3, 4)]
    cur, src, outputs, ref, counts, comp = _case(B, h, w, (0,))
    got, n = _run(cur, src, outputs)
    _check(got, ref, comp, "21x27")
    assert n == counts and all(n[f"grad_s{i}"] > 0 for i in range(4))
    assert torch.equal(got["ms_loss"].view(torch.int32), got["log_l1_loss"].view(torch.int32))  # scale 0 alone: the same mean


def test_several_tiles_and_every_grid_give_the_same_bits():
    B, h, w = 3, 40, 72
    cur, src, outputs, ref, counts, comp = _case(B, h, w)
    base, n = _run(cur, src, outputs)
    _check(base, ref, comp, "40x72")
    assert n == counts
    for mw in (0, 1, 3):
        other, n2 = _run(cur, src, outputs, max_workgroups=mw)
        assert _bits(other) == _bits(base) and n2 == n, mw


def test_edge_semantics():
    from implicit_depth_amd import _lib, evaluation

    cur, src, outputs, ref, counts, _ = _case(2, 24, 32)
    # an empty mask_b: the five masked means are the mean of nothing
    c = dict(cur, mask_b_b1hw=torch.zeros_like(cur["mask_b_b1hw"]))
    got, n = _run(c, src, outputs)
    assert all(torch.isnan(got[k]) for k in ("ms_loss", "abs_loss", "si_loss", "inv_abs_loss", "log_l1_loss", "loss"))
    assert n["mask_b"] == 0 and n["mask_b_limit"] == 0 and torch.isfinite(got["grad_loss"]) and torch.isfinite(got["normals_loss"])
    # a ground truth without a finite value: no gradient counts at any level
    c = dict(cur, depth_b1hw=torch.full_like(cur["depth_b1hw"], float("nan")))
    got, n = _run(c, src, outputs)
    assert torch.isnan(got["grad_loss"]) and [n[f"grad_s{i}"] for i in range(4)] == [0, 0, 0, 0]
    # one NaN of the prediction where the ground truth's gradient is finite
    o = dict(outputs, depth_pred_s0_b1hw=outputs["depth_pred_s0_b1hw"].clone())
    o["depth_pred_s0_b1hw"][0, 0, 10, 20] = float("nan")
    assert torch.isfinite(cur["depth_b1hw"][0, 0, 8:13, 18:23]).all()
    got, n = _run(cur, src, o)
    assert not torch.isfinite(got["grad_loss"]) and n["grad_s0"] == counts["grad_s0"]
    # what cannot be computed raises
    with pytest.raises(_lib.IdhError, match="Could not find a valid scale to compute si loss!"):
        _run(cur, src, {k: v for k, v in outputs.items() if not k.startswith("log_")})
    with pytest.raises(_lib.IdhError, match="log_depth_pred_s1_b1hw"):
        _run(cur, src, dict(outputs, log_depth_pred_s1_b1hw=torch.zeros(2, 1, 10, 16)))
    with pytest.raises(_lib.IdhError, match="mask_b_b1hw"):
        _run(dict(cur, mask_b_b1hw=cur["mask_b_b1hw"][:, :, :-1]), src, outputs)
    o = _cuda(outputs)
    o["depth_pred_s0_b1hw"].requires_grad_(True)
    with pytest.raises(_lib.IdhError, match="forward only"):
        evaluation.reg_val_losses(o, _cuda(cur), _cuda(src))
    with torch.no_grad():
        assert torch.isfinite(evaluation.reg_val_losses(o, _cuda(cur), _cuda(src))["loss"])
    with pytest.raises(_lib.IdhError, match="src_data"):
        _run(cur, None, outputs)


def test_loss_modules_alone_and_fewer_scales():
    from implicit_depth_amd import losses

    cur, src, outputs, ref, _, _ = _case(3, 40, 72)
    got, _ = _run(cur, src, outputs)
    gt, pred = cur["depth_b1hw"].cuda(), outputs["depth_pred_s0_b1hw"].cuda()
    g = losses.MSGradientLoss()(gt, pred)
    nl = losses.NormalsLoss()(cur["normals_b3hw"].cuda(), outputs["normals_pred_b3hw"].cuda())
    mv = losses.MVDepthLoss(40, 72)(pred, gt, src["depth_b1hw"].cuda(), cur["invK_s0_b44"].cuda(), src["K_s0_b44"].cuda(),
                                    cur["world_T_cam_b44"].cuda(), src["cam_T_world_b44"].cuda())
    for name, v in (("grad_loss", g), ("normals_loss", nl), ("mv_loss", mv)):
        assert v.dim() == 0 and v.dtype == torch.float32 and torch.equal(v.cpu().view(torch.int32), got[name].view(torch.int32)), name
    levels = R.grad_levels64(cur["depth_b1hw"], outputs["depth_pred_s0_b1hw"])
    for num_scales in (1, 2, 3):
        want = sum(m for m, _ in levels[:num_scales])
        comp = float(R.grad_loss32(cur["depth_b1hw"], outputs["depth_pred_s0_b1hw"], num_scales))
        v = losses.MSGradientLoss(num_scales)(gt, pred).item()
        print(f"num_scales={num_scales}: {v:.9g} error {abs(v - want):.3e} (composition {abs(comp - want):.3e})")
        assert abs(v - want) <= max(FACTOR * abs(comp - want), FLOOR * abs(want))


def test_compute_normals_option():
    from implicit_depth_amd import _lib, evaluation, geometry

    cur, src, outputs, _, _, _ = _case(2, 24, 32)
    c, s, o = _cuda(cur), _cuda(src), _cuda(outputs)
    c["normals_b3hw"] = geometry.depth_normals(c["depth_b1hw"], c["invK_s0_b44"])[0]
    o["normals_pred_b3hw"] = geometry.depth_normals(o["depth_pred_s0_b1hw"], c["invK_s0_b44"])[0]
    want = evaluation.reg_val_losses(o, c, s)
    bare_c, bare_o = {k: v for k, v in c.items() if k != "normals_b3hw"}, {k: v for k, v in o.items() if k != "normals_pred_b3hw"}
    got = evaluation.reg_val_losses(bare_o, bare_c, s, compute_normals=True)
    assert "normals_b3hw" not in bare_c and "normals_pred_b3hw" not in bare_o
    for k in R.KEYS:
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
    assert torch.isfinite(got["normals_loss"])
    for oo, cc in ((bare_o, c), (o, bare_c)):
        with pytest.raises(_lib.IdhError, match="compute_normals=True"):
            evaluation.reg_val_losses(oo, cc, s)


class _RefLoss(torch.nn.Module):
    """What convert reads of the reference's loss modules (losses.py:78-81, :144-148)."""
    num_scales, height, width = 4, 24, 32


def test_convert_native_losses_on_the_depth_model_stand_in():
    """The three loss attributes of a DepthModel-shaped module are replaced by the native modules, a second call changes nothing, nothing of
    the reference or of kornia is imported, and the statements of compute_losses that call them (depth_model.py:501, :512, :517-525) give
    the entries of reg_val_losses bit for bit."""
    from implicit_depth_amd import dropin, losses
    from test_bdmodel_gpu import _standin_model

    m = _standin_model(2, "mlp", decoder="depth")
    plain = dropin.convert(m, native_losses=True)
    assert plain is m and not hasattr(m, "grad_loss")
    m.grad_loss, m.normals_loss, m.mv_depth_loss = _RefLoss(), _RefLoss(), _RefLoss()
    before = set(sys.modules)
    dropin.convert(m, native_losses=True)
    new = (m.grad_loss, m.normals_loss, m.mv_depth_loss)
    assert isinstance(new[0], losses.MSGradientLoss) and isinstance(new[1], losses.NormalsLoss) and isinstance(new[2], losses.MVDepthLoss)
    dropin.convert(m, native_losses=True)
    assert (m.grad_loss, m.normals_loss, m.mv_depth_loss) == new
    m.cuda()
    cur, src, outputs, _, _, _ = _case(2, 24, 32)
    want, _ = _run(cur, src, outputs)
    c, s, o = _cuda(cur), _cuda(src), _cuda(outputs)
    with torch.no_grad():
        grad = m.grad_loss(c["depth_b1hw"], o["depth_pred_s0_b1hw"])
        nrm = m.normals_loss(c["normals_b3hw"], o["normals_pred_b3hw"])
        mv = m.mv_depth_loss(depth_pred_b1hw=o["depth_pred_s0_b1hw"], cur_depth_b1hw=c["depth_b1hw"], src_depth_bk1hw=s["depth_b1hw"],
                             cur_invK_b44=c["invK_s0_b44"], src_K_bk44=s["K_s0_b44"], cur_world_T_cam_b44=c["world_T_cam_b44"],
                             src_cam_T_world_bk44=s["cam_T_world_b44"])
        loss = want["ms_loss"].cuda() + 1.0 * grad + 1.0 * nrm + 0.2 * mv
    assert not any(name.startswith("utils") or name.startswith("kornia") for name in set(sys.modules) - before)
    for name, v in (("grad_loss", grad), ("normals_loss", nrm), ("mv_loss", mv), ("loss", loss)):
        assert torch.equal(v.cpu().view(torch.int32), want[name].view(torch.int32)), name
