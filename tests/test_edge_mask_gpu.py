"""geometry.edge_mask, evaluation.bd_val_losses and dropin.fused_forward(native_edge_mask=True) on the GPU (csrc/edge_mask.hip, DESIGN.md
§4.27) against tests/edge_mask_ref.py and golden G17.

The mask checks form a chain, each stage against torch applied on the CPU to the kernel's own previous stage, so that fp32 summation order
cannot fail a test: (a) the Sobel map against the composition's NaN / inf sets and the fp64 contract, (b) the threshold against the order
statistics and torch.nanquantile of the kernel's map, (c) the undilated mask against `map > threshold`, (d) the dilated mask against
F.max_pool2d of (c), (e) the undilated mask against the fp64 contract outside a narrow band around its threshold, (f) two runs bit for bit.
(e) is applied to the smooth-plus-step field with and without a zero patch at the sizes of 768 pixels and more, where 0.5 % of an image
is several pixels; at 5x7 a single order statistic on the threshold (q = 0 or 1 put one there by construction) is 2.9 % of the image."""
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_mask_ref as E
from conftest import load_golden
from normals_ref import FACTOR, FLOOR, field

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 7), (3, 24, 32), (2, 37, 53), (2, 192, 256)]
CASES = ["field", "patch", "allnan", "const", "zeros10"]
QS = (0.95, 0.975, 0.0, 1.0)
_inputs, _cpu_refs = {}, {}


def _depth(case, shape):
    """The input of a case, built once."""
    key = (case, shape)
    if key not in _inputs:
        d = field(*shape)
        if case == "patch":
            d = E.with_zero_patch(d)
        elif case == "allnan":  # image 0 is NaN everywhere: n = 0 there
            d[0] = float("nan")
        elif case == "const":  # every value of S ties
            d = torch.full_like(d, 2.5)
        elif case == "zeros10":  # more than 1 - q of the values of S are inf
            d = E.with_scattered_zeros(d, 0.10)
        _inputs[key] = d
    return _inputs[key]


def _refs(case, shape):
    """Composition map (fp32, CPU) and fp64 map of a case, computed once and left unchanged."""
    key = (case, shape)
    if key not in _cpu_refs:
        d = _depth(case, shape)
        _cpu_refs[key] = (E.sobel32(1 / d).numpy(), E.sobel64(d))
    return _cpu_refs[key]


def _ulp_close(a, b):
    """Same class when non-finite, else within one fp32 ulp of b."""
    a, b = np.float32(a), np.float32(b)
    if not np.isfinite(b) or not np.isfinite(a):
        return (np.isnan(a) and np.isnan(b)) or (np.isinf(a) and np.isinf(b) and np.sign(a) == np.sign(b))
    return abs(np.float64(a) - np.float64(b)) <= np.float64(np.spacing(np.abs(b)))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_mask_chain(shape, case):
    from implicit_depth_amd import geometry

    B, H, W = shape
    depth = _depth(case, shape)
    S32, S64 = _refs(case, shape)
    dev = depth.cuda()
    for q in QS:
        md, S, thr = geometry.edge_mask(dev, q, True, return_sobel=True, return_threshold=True)
        mu, S2, thr2 = geometry.edge_mask(dev, q, False, return_sobel=True, return_threshold=True)
        mb = geometry.edge_mask(dev, q, False, as_bool=True)
        assert md.shape == (B, 1, H, W) and md.dtype == torch.float32 and mb.dtype == torch.bool and thr.shape == (B,)
        md, mu, mb, S, S2, thr, thr2 = (t.cpu() for t in (md, mu, mb, S, S2, thr, thr2))
        what = f"{case} {shape} q={q}"
        # (f) determinism: the map and the threshold do not depend on the run (nor on the mask's options)
        assert torch.equal(S.view(torch.int32), S2.view(torch.int32)) and torch.equal(thr.view(torch.int32), thr2.view(torch.int32)), what
        assert torch.equal(mb, mu.bool()), what
        # (a) the Sobel map
        Sn = S.numpy()
        assert np.array_equal(np.isnan(Sn), np.isnan(S32)) and np.array_equal(np.isinf(Sn), np.isinf(S32)), what
        assert not (Sn[np.isinf(Sn)] < 0).any()
        fin = np.isfinite(S64)
        assert np.array_equal(fin, np.isfinite(Sn)), what
        if fin.any():
            err_c = np.abs(S32.astype(np.float64) - S64)[fin].max()
            err_k = np.abs(Sn.astype(np.float64) - S64)[fin].max()
            print(f"{what}: Sobel error {err_k:.3e} (composition {err_c:.3e})")
            assert err_k <= max(FACTOR * err_c, FLOOR), what
        # (b) the threshold against the kernel's own map
        tq = torch.nanquantile(S.flatten(1), q, 1)
        for b in range(B):
            n, lo, hi, w, v_lo, v_hi = E.order_statistics(Sn[b], q)
            t = thr[b].item()
            if n == 0:
                assert np.isnan(t), what
                continue
            if np.isfinite(v_lo) and np.isfinite(v_hi):
                assert v_lo <= t <= v_hi, (what, b, v_lo, t, v_hi)
            assert _ulp_close(t, tq[b].item()), (what, b, t, tq[b].item())
        # (c) and (d): the masks against torch on the kernel's own map and threshold
        mu_ref = (S > thr.reshape(-1, 1, 1, 1)).float()
        assert torch.equal(mu, mu_ref), what
        assert torch.equal(md, F.max_pool2d(mu, 5, 1, 2)), what
        if case == "const":
            assert mu.sum() == 0 and md.sum() == 0 and torch.isfinite(thr).all()
        if case == "allnan":
            assert md[0].sum() == 0 and torch.isnan(thr[0])
        if case == "zeros10" and q == 0.95:
            assert not torch.isfinite(thr).any(), what  # the class torch gives was checked in (b)
        # (e) end to end against the fp64 contract
        if case in ("field", "patch") and H * W >= 768:
            m64, _, thr64, band = E.mask64(depth, q, S64)
            assert band.reshape(B, -1).mean(1).max() <= E.BAND_CAP, (what, band.reshape(B, -1).sum(1))
            bad = (mu.numpy().astype(bool) != m64) & ~band
            assert not bad.any(), (what, int(bad.sum()))


def test_edge_mask_matches_the_reference_golden_and_the_dataset_form():
    """Golden G17 (the reference's own get_edge_mask on the restated Sobel): the kernel's masks may differ from it only where the undilated
    masks differ inside the band, i.e. nowhere on these two inputs unless a pixel sits in the band."""
    from implicit_depth_amd import geometry

    g = load_golden("g17_edge")
    B, H, W = (int(v) for v in g["shape"])
    unpack = lambda key: np.unpackbits(g[key])[:B * H * W].reshape(B, 1, H, W).astype(bool)
    for name in ("plain", "patch"):
        depth = field(B, H, W)
        if name == "patch":
            depth = E.with_zero_patch(depth)
        for q, dil, key in ((0.95, False, f"{name}_mask_dilate0"), (0.95, True, f"{name}_mask_dilate1"), (0.975, False, f"{name}_dataset_mask")):
            got = geometry.edge_mask(depth.cuda(), q, dil).cpu().numpy().astype(bool)
            _, _, _, band = E.mask64(depth, q)
            band = E.dilate(band) if dil else band
            assert not ((got != unpack(key)) & ~band).any(), (name, q, dil)
        # the dataset's call: a (1,H,W) map, bool out
        one = geometry.edge_mask(depth[0].cuda(), 0.975, False, as_bool=True)
        assert one.shape == (1, H, W) and one.dtype == torch.bool
        assert torch.equal(one.cpu(), geometry.edge_mask(depth[:1].cuda(), 0.975, False, as_bool=True)[0].cpu())


def _losses(pred, rendered, depth, edge, wgt, **kw):
    from implicit_depth_amd import evaluation

    cur = {"rendered_depth": rendered.cuda(), "depth_b1hw": depth.cuda()}
    if edge is not None:
        cur["edge_mask"] = edge.cuda()
    out = evaluation.bd_val_losses({"pred_0": pred.cuda()}, cur, wgt, edge is not None, return_counts=True, **kw)
    assert all(out[k].dim() == 0 and out[k].dtype == torch.float32 for k in ("binary_loss/0", "reg_loss/0", "binary_loss", "loss"))
    return {k: v.cpu() for k, v in out.items()}


def _check_losses(pred, rendered, depth, edge, wgt, what):
    """Counts exact; each value within FACTOR x the error of the torch fp32 composition against fp64 (floor: FLOOR x the value's size)."""
    got = _losses(pred, rendered, depth, edge, wgt)
    nm, nr, *ref = E.losses64(pred, rendered, depth, edge, wgt)
    comp = E.losses32(pred, rendered, depth, edge, wgt)
    assert got["counts"].tolist() == [nm, nr], what
    for key, r, c in zip(("binary_loss/0", "reg_loss/0", "binary_loss"), ref, comp):
        v = got[key].item()
        if np.isnan(r):
            assert np.isnan(v) and np.isnan(c.item()), (what, key)
            continue
        err_k, err_c = abs(v - r), abs(c.item() - r)
        print(f"{what} {key}: {v:.9g} error {err_k:.3e} (composition {err_c:.3e})")
        assert err_k <= max(FACTOR * err_c, FLOOR * max(1.0, abs(r))), (what, key, v, r)
    assert torch.equal(got["loss"].view(torch.int32), got["binary_loss"].view(torch.int32))  # (bits: the total may be a NaN)
    return got


def test_bd_val_losses_golden_fp64_counts_and_empty_cases():
    g = load_golden("g17_edge")
    B, H, W = (int(v) for v in g["shape"])
    pred, rendered, depth = E.loss_inputs(B, 3, H, W)
    edge = torch.from_numpy(np.unpackbits(g["loss_edge_mask"])[:B * H * W].reshape(B, 1, H, W).astype(np.float32))
    for cname, em in {"edge": edge, "noedge": None, "emptyreg": torch.zeros_like(edge)}.items():
        for wgt in (0.0, 0.5):
            got = _check_losses(pred, rendered, depth, em, wgt, f"{cname} w={wgt}")
            gold = g[f"loss_{cname}_w{wgt}"]
            vals = np.array([got[k].item() for k in ("binary_loss/0", "reg_loss/0", "binary_loss")], dtype=np.float32)
            # the golden is the reference's fp32 result: a mean of ~4000 fp32 terms, itself within ~1e-6 relative of the exact value
            np.testing.assert_allclose(vals, gold, rtol=2e-6, atol=0, equal_nan=True)
            if cname == "edge":
                assert got["counts"].tolist() == g["loss_counts"].tolist()
            if cname == "emptyreg":  # the mean of nothing
                assert got["counts"][1] == 0 and np.isnan(vals[1]) and (np.isnan(vals[2]) if wgt > 0 else vals[2] == vals[0])
    # an empty mask: a total of 0 (the per-scale entries, which the reference does not create, are NaN)
    got = _losses(pred, torch.zeros_like(rendered), depth, edge, 0.5)
    assert got["counts"].tolist() == [0, 0] and got["binary_loss"].item() == 0.0 and got["loss"].item() == 0.0
    assert torch.isnan(got["binary_loss/0"]) and torch.isnan(got["reg_loss/0"])
    # the weighting of compute_losses and a positive weight other than 1
    from implicit_depth_amd import evaluation

    cur = {"rendered_depth": rendered.cuda(), "depth_b1hw": depth.cuda(), "edge_mask": edge.cuda()}
    o = evaluation.bd_val_losses({"pred_0": pred.cuda()}, cur, 0.5, True, 2.0, positive_weight=3.0)
    assert o["loss"].item() == 2.0 * o["binary_loss"].item()
    ref = E.losses64(pred, rendered, depth, edge, 0.5, 3.0)
    comp = E.losses32(pred, rendered, depth, edge, 0.5, 3.0)
    assert abs(o["binary_loss/0"].item() - ref[2]) <= max(FACTOR * abs(comp[0].item() - ref[2]), FLOOR * abs(ref[2]))


@pytest.mark.parametrize("shape", [(2, 3, 24, 32), (3, 5, 37, 53)], ids=lambda s: "x".join(map(str, s)))
def test_bd_val_losses_do_not_depend_on_the_grid(shape):
    """Several chunks of 2048 elements (3 and 15, the last one partial): one workgroup, three, and the default grid give the same bits,
    and so do two runs; the values hold against fp64."""
    B, D, h, w = shape
    pred, rendered, depth = E.loss_inputs(B, D, h, w)
    edge = E.composition(depth)[0]
    base = _check_losses(pred, rendered, depth, edge, 0.5, f"{shape}")
    for mw in (0, 1, 3):
        other = _losses(pred, rendered, depth, edge, 0.5, max_workgroups=mw)
        for k in base:
            assert torch.equal(base[k].view(torch.int32) if base[k].dtype == torch.float32 else base[k],
                               other[k].view(torch.int32) if other[k].dtype == torch.float32 else other[k]), (k, mw)


class _Opts:
    matching_scale = 1
    min_matching_depth = 0.25
    max_matching_depth = 5.0
    use_prior = False
    bd_edge_regularision = True
    bd_regularisation_weight = 0.5


def test_fused_forward_fills_the_edge_mask_natively():
    """A BDModel drop-in with bd_edge_regularision on and no reference on the import path: with native_edge_mask the forward fills
    cur_data["edge_mask"] with geometry.edge_mask of the ground-truth depth, imports nothing of the reference, and leaves every output as
    the run without the option has it; the validation losses then run on the result.  Without the flag the same call still raises."""
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import _lib, evaluation, geometry
    from implicit_depth_amd.dropin import fused_forward
    from test_bdmodel_gpu import _standin_model

    K = 7
    m = _standin_model(K, "mlp")
    syn.fill_state_dict(m, seed=30)
    m.cuda().eval()
    cur, src = syn.frame_tuple(2, K, 96, 128, seed=31, P=3)
    cur = {k: v.cuda() for k, v in cur.items()}
    src = {k: v.cuda() for k, v in src.items()}
    h, w = cur["rendered_depth"].shape[-2:]
    cur["depth_b1hw"] = E.with_zero_patch(field(2, h, w)).cuda()
    before = set(sys.modules)
    with torch.no_grad():
        plain = fused_forward(m)("test", dict(cur), src)  # the option off (the stand-in's run_opts do not carry it)
        m.run_opts = _Opts()
        cur_n = dict(cur)
        out = fused_forward(m, native_edge_mask=True)("test", cur_n, src)
    assert "edge_mask" in cur_n and "edge_mask" not in cur
    assert not any(name.startswith("utils") or name.startswith("kornia") for name in set(sys.modules) - before)
    want = geometry.edge_mask(cur["depth_b1hw"])
    assert torch.equal(cur_n["edge_mask"], want) and 0 < want.sum() < want.numel()
    assert sorted(out) == sorted(plain)
    compared = 0
    for k in out:
        if out[k] is None:
            assert plain[k] is None, k
            continue
        assert torch.equal(out[k], plain[k]), k
        compared += 1
    assert compared >= 1 and "pred_0" in out
    losses = evaluation.bd_val_losses(out, cur_n, m.run_opts.bd_regularisation_weight, m.run_opts.bd_edge_regularision)
    ref = E.losses64(out["pred_0"].cpu(), cur["rendered_depth"].cpu(), cur["depth_b1hw"].cpu(), want.cpu(), 0.5)
    assert abs(losses["loss"].item() - ref[4]) <= 2e-6 * abs(ref[4])  # an fp32 result of an O(1) mean
    with pytest.raises(_lib.IdhError, match="native_edge_mask=True"):
        fused_forward(m)("test", dict(cur), src)
