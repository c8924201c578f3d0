"""Fused per-frame test evaluation (csrc/eval_frame.hip, implicit-depth_amd/evaluation.py) against the reference's evaluation
loops replayed on CPU (golden G14, tests/golden/gen_golden_eval.py) and against a CPU torch composition written here.

Counting rule: valid and target counts are exact.  The pred / inter counts of a (frame, tag, plane) may differ from the
reference's by at most the number of valid pixels whose interpolated prediction lies within 2e-6 of its threshold (relative
1e-6 of the query for the regressed compare): another fp32 implementation may decide those either way.  Where that number is 0
the counts, and so the scores, are exact."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import implicit_depth_amd.synthetic as syn
from conftest import load_golden

pytestmark = pytest.mark.gpu

THR_MARGIN, REG_MARGIN = 2e-6, 1e-6
PLANES = torch.tensor([1.5 + 0.5 * i for i in range(8)])


def _case(g, name):
    c = json.loads(str(g[f"{name}__case"]))
    outputs, cur = syn.eval_frame_case(*c["shape"])
    return c, outputs, cur


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def _thresholder(g):
    from implicit_depth_amd.metrics import Thresholder

    return Thresholder(torch.as_tensor(g["thr_planes"]), torch.as_tensor(g["thr_values"]))


def assert_counts(got, ref, amb, what=""):
    """(B, 3, P, 2 + 2T) counts under the counting rule of the module docstring."""
    got, ref, amb = np.asarray(got, np.int64), np.asarray(ref, np.int64), np.asarray(amb, np.int64)
    assert got.shape == ref.shape, what
    np.testing.assert_array_equal(got[..., :2], ref[..., :2], err_msg=f"{what}: valid / target counts")
    dev = np.abs(got[..., 2:] - ref[..., 2:]).max(-1)
    assert (dev <= amb).all(), (what, dev.max(), amb[dev > amb])
    assert (dev[amb == 0] == 0).all()


def _score_index(ev, B, P, T, names, temporal):
    """key -> (tag, d, t, j) through the same dict builder the product uses."""
    idx = torch.arange(3 * P * T * 3, dtype=torch.float64).view(1, 3, P, T, 3).expand(B, 3, P, T, 3)
    return {k: np.unravel_index(int(v[0]), (3, P, T, 3)) for k, v in ev._tag_scores(idx, names, temporal).items()}


# ---- masks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bd_thr", "bd_thr_mult_odd"])
def test_masks_equal_the_reference_bit_for_bit(name):
    from implicit_depth_amd.evaluation import eval_masks, get_boundary_mask, get_surface_mask

    g = load_golden("g14_eval_frame")
    _, _, cur = _case(g, name)
    d, r = cur["depth_b1hw"].cuda(), cur["rendered_depth"].cuda()
    sm, bm = get_surface_mask(d, r).cpu(), get_boundary_mask(d, r).cpu()
    assert sm.dtype == bm.dtype == torch.float32 and sm.shape == bm.shape == r.shape
    n = sm.numel()
    np.testing.assert_array_equal(np.packbits(sm.numpy().astype(np.uint8).ravel()), g[f"{name}__surface_bits"])
    np.testing.assert_array_equal(np.packbits(bm.numpy().astype(np.uint8).ravel()), g[f"{name}__boundary_bits"])
    assert 0 < int(sm.sum()) < n and 0 < int(bm.sum()) < n
    s2, b2, code = eval_masks(d, r, code=True)
    code = code.cpu()
    assert torch.equal(code & 1, sm.to(torch.uint8)) and torch.equal(code >> 1, bm.to(torch.uint8))
    assert torch.equal(s2.cpu(), sm) and torch.equal(b2.cpu(), bm)


# ---- golden cases -----------------------------------------------------------------------------------------------
IOU_CASES = ["bd_thr", "bd_const", "bd_thr_mult_odd", "bd_temporal_odd", "reg_plane", "reg_plane_temporal_odd"]
DEPTH_CASES = ["bd_eval_depth", "reg_depth", "reg_depth_temporal_odd"]


def _run(g, name):
    from implicit_depth_amd.evaluation import bd_frame_scores, reg_frame_scores

    c, outputs, cur = _case(g, name)
    o, d = _cuda(outputs), _cuda(cur)
    before = {k: v.clone() for k, v in {**o, **d}.items()}
    opts = c["opts"]
    if c["loop"] == "bd":
        th = _thresholder(g) if opts.get("thresholder") else None
        sc, keep = bd_frame_scores(o, d, thresholder=th, bd_sigmoid_multiplier=opts.get("bd_sigmoid_multiplier", 1.0),
                                   temporal_eval=opts.get("temporal_eval", False), binary_eval_depth=opts.get("binary_eval_depth", False))
    else:
        th = None
        sc, keep = reg_frame_scores(o, d, regression_plane_eval=opts.get("regression_plane_eval", False), temporal_eval=opts.get("temporal_eval", False))
    assert set(o) == {"pred_0", "search_depths", "depth_pred_s0_b1hw"} and set(d) == {"depth_b1hw", "rendered_depth", "full_res_depth_b1hw"}
    for k, v in {**o, **d}.items():
        assert torch.equal(torch.nan_to_num(v), torch.nan_to_num(before[k])), f"{k} was modified"
    assert list(sc) == list(g[f"{name}__keys"])
    np.testing.assert_array_equal(keep.cpu().numpy(), g[f"{name}__keep"])
    return c, o, d, th, sc


@pytest.mark.parametrize("name", IOU_CASES)
def test_plane_scores_match_the_reference(name):
    from implicit_depth_amd import evaluation as ev

    g = load_golden(f"g14_eval_frame")
    c, o, d, th, sc = _run(g, name)
    opts, reg = c["opts"], c["loop"] == "reg"
    kw = dict(nearest=opts.get("temporal_eval", False))
    if reg:
        kw.update(regressed=True)
        pred = o["depth_pred_s0_b1hw"]
    else:
        pred = o["pred_0"]
        kw.update(sigmoid_multiplier=opts.get("bd_sigmoid_multiplier", 1.0))
        kw.update(dict(bins=th.bins.cuda(), bin_thresholds=th.thresholds.cuda()) if th is not None else dict(thresholds=list(np.linspace(0.3, 0.7, 5))))
    out, counts = ev.plane_scores(pred, d["rendered_depth"], d["full_res_depth_b1hw"], d["depth_b1hw"], return_counts=True, **kw)
    ref_counts, amb = g[f"{name}__counts"], g[f"{name}__ambiguous"]
    assert_counts(counts.cpu().numpy(), ref_counts, amb, name)
    assert (counts.cpu().numpy() == ref_counts).all(-1).mean() > 0.5  # most (frame, tag, plane) entries exact
    # scores: equal wherever the counts are; the dict carries plane_scores' values
    B, P, T = out.shape[0], out.shape[2], out.shape[3]
    names = [""] if (reg or th is not None) else [f"{t:.1f}_" for t in np.linspace(0.3, 0.7, 5)]
    where = _score_index(ev, B, P, T, names, opts.get("temporal_eval", False))
    ref_vals, out_c, cnt = g[f"{name}__values"], out.cpu(), counts.cpu().numpy()
    exact = 0
    for col, key in enumerate(sc):
        tag, dd, t, j = where[key]
        assert torch.equal(torch.nan_to_num(sc[key].cpu(), 7.0), torch.nan_to_num(out_c[:, tag, dd, t, j], 7.0))
        for b in range(B):
            if (cnt[b, tag, dd] == ref_counts[b, tag, dd]).all():
                np.testing.assert_allclose(float(sc[key][b]), ref_vals[b, col], rtol=1e-6, equal_nan=True, err_msg=key)
                exact += 1
    assert exact > 0.5 * B * len(sc)


@pytest.mark.parametrize("name", DEPTH_CASES)
def test_depth_metrics_match_the_reference(name):
    g = load_golden("g14_eval_frame")
    _, _, _, _, sc = _run(g, name)
    got = torch.stack([sc[k] for k in sc], 1).cpu().numpy()
    np.testing.assert_allclose(got, g[f"{name}__values"], rtol=2e-5)


def test_metric_rows_of_the_frame_dict():
    from implicit_depth_amd.metrics import metric_rows

    g = load_golden("g14_eval_frame")
    _, _, _, _, sc = _run(g, "bd_thr")
    rows, keys = metric_rows(sc)
    assert keys == sorted(g["bd_thr__keys"]) and rows.shape == (2, len(keys)) and rows.dtype == torch.float32
    col = {k: i for i, k in enumerate(g["bd_thr__keys"])}
    ref = g["bd_thr__values"][:, [col[k] for k in keys]]
    got = rows.cpu().numpy()
    same = np.isclose(got, ref, rtol=1e-6, equal_nan=True)
    assert same.mean() > 0.9


# ---- against a CPU torch composition -------------------------------------------------------------------------------
def compose_counts(outputs, cur, thresholds=None, thresholder=None, mult=1.0, nearest=False, regressed=False, chunk=4):
    """The torch sequence of test_bd.py:185-318 / test_reg.py:204-261 restated (masks with max_pool2d, F.interpolate, counting)
    on CPU, a few frames at a time: counts (B, 3, P, 2 + 2T) and ambiguous pixels (B, 3, P)."""
    cnt, amb = [], []
    gt_all = cur["full_res_depth_b1hw"].cpu()
    for b0 in range(0, gt_all.shape[0], chunk):
        sl = slice(b0, b0 + chunk)
        depth, rend, gt = cur["depth_b1hw"][sl].cpu(), cur["rendered_depth"][sl].cpu(), gt_all[sl]
        nan = torch.isnan(depth).expand_as(rend)
        t = (rend < depth).float()
        edges = torch.where(nan, torch.zeros_like(t), F.max_pool2d(t, 3, 1, 1) - t)
        boundary = (F.max_pool2d(edges, 7, 1, 3) > 0) & ~nan
        surface = (depth - rend).abs() / depth < 0.05
        size = gt.shape[-2:]
        mode = "nearest" if nearest else "bilinear"
        if regressed:
            pred = F.interpolate(outputs["depth_pred_s0_b1hw"][sl].cpu(), size=size, mode=mode)
        else:
            pred = F.interpolate(1 / (1 + torch.exp(-mult * outputs["pred_0"][sl].cpu())), size=size, mode=mode)
        neg = torch.full_like(rend, -1.0)
        queries = [F.interpolate(q, size=size, mode="nearest") for q in (rend, torch.where(surface, rend, neg), torch.where(boundary, rend, neg))]
        c_tags, a_tags = [], []
        for q in queries:
            valid = (gt > 0) & (q > 0)
            target = (q < gt) & valid
            p = pred.expand_as(q)
            if regressed:
                prs, near = [q < p], (q - p).abs() <= REG_MARGIN * q.abs()
            elif thresholder is not None:
                idx = torch.bucketize(q, thresholder.bins.cpu()).clamp_max(thresholder.bins.numel() - 1)
                tq = thresholder.thresholds.cpu()[idx]
                prs, near = [p > tq], (p - tq).abs() <= THR_MARGIN
            else:
                prs = [p > float(t) for t in thresholds]
                near = torch.stack([(p - float(t)).abs() <= THR_MARGIN for t in thresholds]).any(0)
            s = lambda m: m.flatten(2).sum(2)
            c_tags.append(torch.stack([s(valid), s(target)] + [s(pr & valid) for pr in prs] + [s(pr & valid & target) for pr in prs], 2))
            a_tags.append(s(near & valid))
        cnt.append(torch.stack(c_tags, 1))
        amb.append(torch.stack(a_tags, 1))
    return torch.cat(cnt).numpy(), torch.cat(amb).numpy()


def test_full_size_batch_against_torch_composition():
    """B = 32, P = 8, 192x256 -> 480x640 (the test_bd.py shape) with the Thresholder."""
    from implicit_depth_amd import evaluation as ev

    g = load_golden("g14_eval_frame")
    th = _thresholder(g)
    outputs, cur = syn.eval_frame_case(32, 8, 192, 256, 480, 640, seed=7)
    o, d = _cuda(outputs), _cuda(cur)
    out, counts = ev.plane_scores(o["pred_0"], d["rendered_depth"], d["full_res_depth_b1hw"], d["depth_b1hw"], bins=th.bins.cuda(),
                                  bin_thresholds=th.thresholds.cuda(), return_counts=True)
    ref, amb = compose_counts(outputs, cur, thresholder=th)
    assert_counts(counts.cpu().numpy(), ref, amb, "B=32")
    assert (counts.cpu().numpy() == ref).all(-1).mean() > 0.5
    sc, keep = ev.bd_frame_scores(o, d, thresholder=th)
    assert len(sc) == 3 * 8 * 3 and bool(keep.all())
    assert torch.equal(torch.nan_to_num(sc["boundary_iou_pos_d_5.0"]), torch.nan_to_num(out[:, 2, 7, 0, 1]))
    # the regressed compare at the same shape
    _, rc = ev.plane_scores(o["depth_pred_s0_b1hw"], d["rendered_depth"], d["full_res_depth_b1hw"], d["depth_b1hw"], regressed=True, return_counts=True)
    ref, amb = compose_counts(outputs, cur, regressed=True)
    assert_counts(rc.cpu().numpy(), ref, amb, "B=32 regressed")


def test_bd_frame_scores_on_fused_forward_outputs():
    """The G5 set-up: dropin.fused_forward on a synthetic BDModel, its outputs scored by bd_frame_scores (constant thresholds and
    the Thresholder) against the torch composition."""
    from implicit_depth_amd import evaluation as ev
    from implicit_depth_amd.dropin import fused_forward
    from test_bdmodel_gpu import _standin_model

    K = 7
    m = _standin_model(K, "mlp")
    syn.fill_state_dict(m, seed=30)
    m.cuda().eval()
    cur, src = syn.frame_tuple(2, K, 96, 128, seed=31, P=3)
    cur = _cuda(cur)
    src = _cuda(src)
    with torch.no_grad():
        out = fused_forward(m)("test", cur, src, return_mask=True)
    h, w = cur["rendered_depth"].shape[-2:]
    assert out["pred_0"].shape == cur["rendered_depth"].shape
    _, extra = syn.eval_frame_case(2, 3, h, w, 120, 160, seed=9)
    cur["depth_b1hw"] = extra["depth_b1hw"].cuda()
    cur["full_res_depth_b1hw"] = extra["full_res_depth_b1hw"].cuda()
    g = load_golden("g14_eval_frame")
    th = _thresholder(g)
    pred = {"pred_0": out["pred_0"].detach()}
    for thr in (None, th):
        sc, keep = ev.bd_frame_scores(pred, cur, thresholder=thr)
        assert list(sc) == ev.bd_score_keys(3, thresholder=thr)
        kw = dict(bins=thr.bins.cuda(), bin_thresholds=thr.thresholds.cuda()) if thr is not None else dict(thresholds=list(np.linspace(0.3, 0.7, 5)))
        _, counts = ev.plane_scores(pred["pred_0"], cur["rendered_depth"], cur["full_res_depth_b1hw"], cur["depth_b1hw"], return_counts=True, **kw)
        ref, amb = compose_counts({"pred_0": pred["pred_0"].cpu()}, cur, thresholds=np.linspace(0.3, 0.7, 5), thresholder=thr)
        assert_counts(counts.cpu().numpy(), ref, amb, f"fused_forward thresholder={thr is not None}")
        assert ref[:, 0, :, 0].min() > 0  # every (frame, plane) has valid pixels


def test_regressed_batch_scores_method_matches_the_composition():
    """metrics.PlaneEvaluator.compute_regressed_depth_batch_scores on full-resolution tensors (binary_metrics_utils.py:194-244)."""
    from implicit_depth_amd.metrics import PlaneEvaluator

    outputs, cur = syn.eval_frame_case(2, 3, 100, 140, 100, 140, seed=11)
    q = cur["rendered_depth"].clone()
    q[:, 1, :20] = -1.0
    gt, pred = cur["full_res_depth_b1hw"], outputs["depth_pred_s0_b1hw"]
    sc = PlaneEvaluator().compute_regressed_depth_batch_scores(q.cuda(), gt.cuda(), pred.cuda(), tag="surface")
    assert list(sc)[:3] == ["surface_iou_d_1.5", "surface_iou_pos_d_1.5", "surface_iou_neg_d_1.5"] and len(sc) == 9
    valid = (gt > 0) & (q > 0)
    tgt, pr = (q < gt) & valid, (q < pred) & valid
    s = lambda m: m.flatten(2).sum(2).float()
    nv, nt, np_, ni = s(valid), s(tgt), s(pr), s(pr & tgt)
    pos = ni / (nt + np_ - ni)
    neg = (nv - nt - np_ + ni) / ((nv - nt) + (nv - np_) - (nv - nt - np_ + ni))
    for dd, plane in enumerate((1.5, 2.0, 2.5)):
        np.testing.assert_allclose(sc[f"surface_iou_pos_d_{plane:.1f}"].cpu().numpy(), pos[:, dd].numpy(), rtol=1e-6)
        np.testing.assert_allclose(sc[f"surface_iou_neg_d_{plane:.1f}"].cpu().numpy(), neg[:, dd].numpy(), rtol=1e-6)
        np.testing.assert_allclose(sc[f"surface_iou_d_{plane:.1f}"].cpu().numpy(), (2 * pos * neg / (pos + neg))[:, dd].numpy(), rtol=1e-6)


# ---- errors -------------------------------------------------------------------------------------------------------
def test_errors_for_bad_shapes_thresholds_and_workspace():
    import ctypes as C

    from implicit_depth_amd import _lib
    from implicit_depth_amd import evaluation as ev

    outputs, cur = syn.eval_frame_case(1, 2, 24, 32, 60, 80, seed=12)
    o, d = _cuda(outputs), _cuda(cur)
    with pytest.raises(_lib.IdhError):  # prediction planes != query planes
        ev.plane_scores(o["pred_0"][:, :1], d["rendered_depth"], d["full_res_depth_b1hw"], d["depth_b1hw"], thresholds=[0.5])
    with pytest.raises(_lib.IdhError):  # model-resolution depth of another size
        ev.get_surface_mask(d["depth_b1hw"][..., :16], d["rendered_depth"])
    with pytest.raises(_lib.IdhError):  # more than 8 constant thresholds
        ev.plane_scores(o["pred_0"], d["rendered_depth"], d["full_res_depth_b1hw"], d["depth_b1hw"], thresholds=list(np.linspace(0.1, 0.9, 9)))
    with pytest.raises(_lib.IdhError):  # CPU tensors: no fallback
        ev.bd_frame_scores(outputs, cur)
    a = _lib.EvalArgs()
    a.prediction, a.rendered_bphw, a.depth_b1hw, a.gt_b1HW = o["pred_0"].data_ptr(), d["rendered_depth"].data_ptr(), d["depth_b1hw"].data_ptr(), \
        d["full_res_depth_b1hw"].data_ptr()
    thr = torch.tensor([0.5], device="cuda")
    a.thresholds, a.T, a.tag_mask, a.sigmoid_multiplier, a.surface_threshold = thr.data_ptr(), 1, 7, 1.0, 0.05
    a.B, a.P, a.h, a.w, a.H, a.W = 1, 2, 24, 32, 60, 80
    out = torch.full((1, 3, 2, 1, 3), 7.0, device="cuda")
    n = _lib.lib().idh_eval_frame_workspace_bytes(1, 2, 24, 32, 60, 80, 1)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    assert L.idh_eval_plane_scores_fwd(C.byref(a), out.data_ptr(), None, ws.data_ptr(), 16, _lib.stream_ptr()) == -4
    assert L.idh_eval_plane_scores_fwd(C.byref(a), out.data_ptr(), None, ws.data_ptr() + 4, n - 4, _lib.stream_ptr()) == -4
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # refused calls launch nothing
    assert L.idh_eval_plane_scores_fwd(C.byref(a), out.data_ptr(), None, ws.data_ptr(), n, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
