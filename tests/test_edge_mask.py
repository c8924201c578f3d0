"""Device-free checks of the edge mask and the validation losses: tests/edge_mask_ref.py against golden G17 - the
reference's own get_edge_mask and compute_binary_losses, tests/golden/gen_golden_edge.py - the contract's statements about non-finite
values, the argument validation of the two C entry points, and the text of the drop-in's error."""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_mask_ref as E
from conftest import load_golden
from normals_ref import field


def _unpack(g, key):
    B, H, W = (int(v) for v in g["shape"])
    return np.unpackbits(g[key])[:B * H * W].reshape(B, 1, H, W).astype(bool)


@pytest.mark.parametrize("name", ["plain", "patch"])
def test_reference_forms_reproduce_the_golden_masks(name):
    """The torch composition gives the reference's masks bit for bit (same Sobel, the reference's quantile / compare / max-pool); the fp64
    restatement differs from them only at pixels inside the band around its threshold, and its own dilation is the reference's."""
    g = load_golden("g17_edge")
    B, H, W = (int(v) for v in g["shape"])
    depth = field(B, H, W)
    if name == "patch":
        depth = E.with_zero_patch(depth)
    for dil in (True, False):
        m, _, _ = E.composition(depth, 0.95, dil)
        assert np.array_equal(m.numpy().astype(bool), _unpack(g, f"{name}_mask_dilate{int(dil)}")), (name, dil)
    ds, _, _ = E.composition(depth, 0.975, False)  # the dataset's variant: torch.quantile of the non-NaN values == nanquantile
    assert np.array_equal(ds.numpy().astype(bool), _unpack(g, f"{name}_dataset_mask"))
    for q, key in ((0.95, f"{name}_mask_dilate0"), (0.975, f"{name}_dataset_mask")):
        m64, _, thr64, band = E.mask64(depth, q)
        ref = _unpack(g, key)
        assert np.isfinite(thr64).all()
        assert not ((m64 != ref) & ~band).any(), (name, q)
        assert band.reshape(B, -1).mean(1).max() <= E.BAND_CAP, (name, q, band.sum())
        if q == 0.95 and not (m64 != ref).any():
            assert np.array_equal(E.dilate(m64), _unpack(g, f"{name}_mask_dilate1"))
    assert _unpack(g, f"{name}_mask_dilate1").sum() > _unpack(g, f"{name}_mask_dilate0").sum() > 0


def test_zero_patch_gives_the_contracts_nan_and_inf_sets():
    """A 6x6 patch of zero depth: 60 NaN and 4 inf pixels per image (an inf under a zero tap is a NaN; only the four pixels whose sole inf
    neighbour is a diagonal corner are +inf), in the composition and in the fp64 restatement alike."""
    depth = E.with_zero_patch(field(2, 24, 32))
    _, S, thr = E.composition(depth)
    S64 = E.sobel64(depth)
    for s in (S.numpy(), S64):
        assert np.isnan(s).reshape(2, -1).sum(1).tolist() == [60, 60]
        assert np.isposinf(s).reshape(2, -1).sum(1).tolist() == [4, 4]
    assert np.array_equal(np.isnan(S.numpy()), np.isnan(S64)) and np.array_equal(np.isinf(S.numpy()), np.isinf(S64))
    assert torch.isfinite(thr).all()  # 4 inf of 708 values stay above the 0.95 quantile
    # more than 1 - q of the values at inf: both order statistics are inf and at::lerp's inf - inf is a NaN
    many = E.with_scattered_zeros(field(1, 24, 32), 0.10)
    _, S, thr = E.composition(many)
    assert torch.isinf(S).sum() > 0.05 * (~torch.isnan(S)).sum() and not torch.isfinite(thr).any()
    assert np.array_equal(np.isnan(E.quantile64(E.sobel64(many), 0.95)), torch.isnan(thr).numpy())


def test_reference_forms_reproduce_the_golden_losses():
    """losses32 is compute_binary_losses restated: it must give the reference's numbers; losses64 the same within fp32 summation error
    (a mean of ~4000 terms of size <= 8: pairwise fp32 summation stays within a few ulps of the result, 2e-6 relative is generous)."""
    g = load_golden("g17_edge")
    pred, rendered, depth = E.loss_inputs(2, 3, 24, 32)
    edge = torch.from_numpy(_unpack(g, "loss_edge_mask").astype(np.float32))
    assert np.array_equal(E.composition(depth)[0].numpy(), edge.numpy())
    cases = {"edge": edge, "noedge": None, "emptyreg": torch.zeros_like(edge)}
    for cname, em in cases.items():
        for wgt in (0.0, 0.5):
            gold = g[f"loss_{cname}_w{wgt}"]
            bl, rl, total = E.losses32(pred, rendered, depth, em, wgt)
            got = np.array([bl.item(), rl.item(), total.item()], dtype=np.float32)
            assert np.array_equal(np.isnan(got), np.isnan(gold)), (cname, wgt, got, gold)
            np.testing.assert_allclose(got, gold, rtol=2e-7, atol=0, equal_nan=True)
            nm, nr, *ref = E.losses64(pred, rendered, depth, em, wgt)
            np.testing.assert_allclose(np.array(ref), gold.astype(np.float64), rtol=2e-6, atol=0, equal_nan=True)
            if cname == "edge":
                assert [nm, nr] == g["loss_counts"].tolist()
            if cname == "emptyreg":
                assert nr == 0 and np.isnan(gold[1]) and (np.isnan(gold[2]) if wgt > 0 else gold[2] == gold[0])
    assert 0 < g["loss_counts"][1] < g["loss_counts"][0]
    # an empty mask: the reference's edge case, a total of 0 and no per-scale entries
    bl, rl, total = E.losses32(pred, torch.zeros_like(rendered), depth, edge, 0.5)
    assert bl is None and rl is None and total.item() == 0.0
    assert E.losses64(pred, torch.zeros_like(rendered), depth, edge, 0.5)[4] == 0.0


def test_entry_points_validate_their_arguments_without_a_device():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert C.sizeof(_lib.EdgeMaskArgs) == L.idh_sizeof_edge_mask_args() and C.sizeof(_lib.BdValLossesArgs) == L.idh_sizeof_bd_val_losses_args()
    assert L.idh_edge_mask_workspace_bytes(2, 24, 32) >= 4 * 2 * 24 * 32 + 4 * 2 and L.idh_edge_mask_workspace_bytes(0, 24, 32) == 0
    assert L.idh_bd_val_losses_workspace_bytes(2, 3, 24, 32) == 32 * 3 and L.idh_bd_val_losses_workspace_bytes(2, 0, 24, 32) == 0

    def edge(**kw):
        a = _lib.EdgeMaskArgs()
        a.depth_b1hw, a.mask_b1hw, a.workspace, a.workspace_bytes = 0x1000, 0x2000, 0x3000, 1 << 20  # never dereferenced: every case fails first
        a.q, a.dilate, a.B, a.H, a.W = 0.95, 1, 2, 24, 32
        for k, v in kw.items():
            setattr(a, k, v)
        return L.idh_edge_mask_fwd(a, None)

    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -4, -2
    assert L.idh_edge_mask_fwd(None, None) == EINVAL
    for bad in (dict(H=0), dict(W=0), dict(W=-3), dict(B=-1), dict(q=-0.01), dict(q=1.5), dict(q=float("nan")), dict(depth_b1hw=None),
                dict(mask_b1hw=None), dict(struct_size=8), dict(workspace=0x3001)):
        assert edge(**bad) == EINVAL, bad
    assert edge(workspace=None) == EWORKSPACE and edge(workspace_bytes=1024) == EWORKSPACE
    assert edge(H=4097, W=4097) == EUNSUPPORTED
    assert edge(B=0) == 0  # nothing to launch
    assert b"invalid" in L.idh_error_string(EINVAL).lower()

    def loss(**kw):
        a = _lib.BdValLossesArgs()
        a.pred_bdhw, a.rendered_bdhw, a.depth_b1hw, a.out5, a.workspace, a.workspace_bytes = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 1 << 20
        a.bd_regularisation_weight, a.positive_weight, a.B, a.D, a.h, a.w = 0.5, 1.0, 2, 3, 24, 32
        for k, v in kw.items():
            setattr(a, k, v)
        return L.idh_bd_val_losses_fwd(a, None)

    assert L.idh_bd_val_losses_fwd(None, None) == EINVAL
    for bad in (dict(B=0), dict(D=0), dict(h=0), dict(w=-1), dict(pred_bdhw=None), dict(rendered_bdhw=None), dict(depth_b1hw=None), dict(out5=None),
                dict(max_workgroups=-1), dict(bd_regularisation_weight=float("nan")), dict(positive_weight=float("nan")), dict(out5=0x4004),
                dict(workspace=0x5004), dict(struct_size=8)):
        assert loss(**bad) == EINVAL, bad
    assert loss(workspace=None) == EWORKSPACE and loss(workspace_bytes=64) == EWORKSPACE
    assert loss(B=1024, D=64, h=192, w=256) == EUNSUPPORTED


def test_python_wrappers_refuse_what_the_kernels_cannot_take():
    from implicit_depth_amd import _lib, evaluation, geometry

    d = field(1, 5, 7)
    with pytest.raises(_lib.IdhError, match="no CPU fallback"):
        geometry.edge_mask(d)
    with pytest.raises(_lib.IdhError, match="no CPU fallback"):
        evaluation.bd_val_losses({"pred_0": torch.zeros(1, 2, 5, 7)}, {"rendered_depth": torch.zeros(1, 2, 5, 7), "depth_b1hw": d}, 0.5, False)


def test_drop_in_error_names_the_native_flag(monkeypatch):
    """Without the reference on the import path the drop-in's error must say how to get the mask natively."""
    import sys

    from implicit_depth_amd import _lib, dropin

    monkeypatch.setitem(sys.modules, "utils", None)  # `import utils...` raises ImportError whatever else is installed
    with pytest.raises(_lib.IdhError) as e:
        dropin._reference_get_edge_mask()
    msg = str(e.value)
    assert "native_edge_mask=True" in msg and "geometry.edge_mask" in msg and "bd_edge_regularision" in msg
    assert "unset the option for pure inference" in msg  # today's advice stays
