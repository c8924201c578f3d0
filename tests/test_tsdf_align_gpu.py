"""TSDF pose alignment on the GPU (idh_tsdf_align_fwd, fusion.align_depth) against the fp64 statement of the header in
tests/tsdf_align_ref.py.  The volumes are the reference's float32 pair tensors uploaded with TSDFVolume.from_values, so only the new
code is under test."""
import functools

import numpy as np
import pytest
import torch

import tsdf_align_ref as AR

pytestmark = pytest.mark.gpu

CROP_CASES = (("room24x32", False, 1, False, 0.0), ("room30x44", True, 2, True, 0.01))


def _cuda(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def _volume(name, box):
    from implicit_depth_amd import fusion

    c = AR.plane_case() if name == "plane" else AR.case(name, box)
    return fusion.TSDFVolume.from_values(_cuda(c["values"]), c["voxel_size"], c["origin"], c["trunc_voxels"])


def _align(name, box, c, pose=None, **kw):
    from implicit_depth_amd import fusion

    weight = kw.pop("weight", None)
    out = fusion.align_depth(_volume(name, box), _cuda(c["depth"])[None, None], _cuda(c["invK"]), _cuda(c["start"] if pose is None else pose),
                             weight_11hw=None if weight is None else _cuda(weight)[None, None], **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _row_case(case, crop, **kw):
    name, box, stride, weighted, huber = case
    c = AR.row_inputs(name, box, weighted, crop)
    kw.setdefault("iters", 1)
    return c, _align(name, box, c, stride=stride, huber=huber, weight=c["weight"], min_count=6, **kw)


ROW_PARAMS = [(c, False) for c in AR.ROW_CASES] + [(c, True) for c in CROP_CASES]


@pytest.mark.parametrize("case,crop", ROW_PARAMS)
def test_rows_match_fp64_and_records_are_their_sums(case, crop):
    c, out = _row_case(case, crop, return_rows=True)
    ref = AR.row_reference(*case, crop)
    rows = out["rows"].astype(np.float64)
    got_valid = (out["rows"] != 0).any(-1)
    assert not (got_valid & ~ref["selected"]).any()  # zero rows where the stride does not select
    keep = ref["selected"] & ~ref["ambiguous"]
    left_out = 1.0 - keep.sum() / ref["selected"].sum()
    print(case, crop, "left out", left_out, "valid", int(ref["valid"].sum()))
    assert left_out <= AR.CAP
    assert np.array_equal(got_valid[keep], ref["valid"][keep])
    # 1: every row within the bounds derived in the reference's docstring (zero rows on both sides where the pixel is skipped)
    eJ, er, ew = np.abs(rows[..., :6] - ref["J"]), np.abs(rows[..., 6] - ref["r"]), np.abs(rows[..., 7] - ref["wgt"])
    tiny = np.finfo(np.float32).tiny
    print("  largest error / bound: J", (eJ[keep] / (ref["eps_J"][keep] + tiny)).max(), "r", (er[keep] / (ref["eps_r"][keep] + tiny)).max(),
          "wgt", (ew[keep] / (ref["eps_w"][keep] + tiny)).max())
    assert (eJ[keep] <= ref["eps_J"][keep]).all()
    assert (er[keep] <= ref["eps_r"][keep]).all()
    assert (ew[keep] <= ref["eps_w"][keep]).all()
    # 2: the record holds the fp64 sums of the kernel's own rows: only the order of the additions may differ.  A sum of n terms in any
    # order is within n 2^-53 of the exact sum relative to the sum of the terms' magnitudes; n <= 1320: 1.5e-13, so 1e-12 of that scale
    rec = out["records"][0]
    J, r, wgt = rows[..., :6].reshape(-1, 6), rows[..., 6].ravel(), rows[..., 7].ravel()
    want, scale = [], []
    for p, q in AR.TRIU:
        want.append(((wgt * J[:, p]) * J[:, q]).sum()), scale.append(np.abs((wgt * J[:, p]) * J[:, q]).sum())
    for p in range(6):
        want.append(((wgt * J[:, p]) * r).sum()), scale.append(np.abs((wgt * J[:, p]) * r).sum())
    want.append(((wgt * r) * r).sum()), scale.append(((wgt * r) * r).sum())
    assert (np.abs(rec[:28] - np.array(want)) <= 1e-12 * np.array(scale)).all()
    assert rec[28] == got_valid.sum() and rec[28] >= 6
    assert (rec[38:] == 0).all() and rec[29] in (0.0, 2.0)


@pytest.mark.parametrize("case,crop", [ROW_PARAMS[0], ROW_PARAMS[6], ROW_PARAMS[-1]])
def test_same_bits_for_every_grid_and_call(case, crop):
    runs = [_row_case(case, crop, iters=3, max_workgroups=g, return_rows=True)[1] for g in (1, 3, 0, 0)]
    for other in runs[1:]:
        for k in ("world_T_cam", "records", "rows"):
            assert runs[0][k].tobytes() == other[k].tobytes(), k
    # 9: asking for the rows changes nothing else
    plain = _row_case(case, crop, iters=3)[1]
    assert "rows" not in plain
    assert plain["world_T_cam"].tobytes() == runs[0]["world_T_cam"].tobytes() and plain["records"].tobytes() == runs[0]["records"].tobytes()


@pytest.mark.parametrize("damping", [0.0, 1e-3])
@pytest.mark.parametrize("case", [AR.ROW_CASES[0], AR.ROW_CASES[13]])
def test_solve_and_pose_update(case, damping):
    c, out = _row_case(case, False, damping=damping)
    rec = out["records"][0]
    assert rec[29] == 0
    A, b = AR.record_system(rec)
    Ad = A + damping * np.diag(np.diag(A))
    xi = np.linalg.solve(Ad, -b)
    assert np.abs(rec[32:38] - xi).max() <= 1e-9 * np.abs(xi).max()
    assert abs(rec[30] - np.linalg.norm(xi[:3])) <= 1e-9 * rec[30] and abs(rec[31] - np.linalg.norm(xi[3:])) <= 1e-9 * rec[31]
    status, xi_ref, _ = AR.solve(A, b, int(rec[28]), damping, 6)
    assert status == 0 and np.abs(rec[32:38] - xi_ref).max() <= 1e-9 * np.abs(xi).max()
    E = c["start"].astype(np.float64)
    Rn, tn = AR.update(E[:3, :3], E[:3, 3], rec[32:38])
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = Rn, tn
    want32 = want.astype(np.float32)
    got = out["world_T_cam"][0]
    assert (np.abs(got.astype(np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32)).astype(np.float64)).all()
    assert got[3].tolist() == [0, 0, 0, 1]


FITS = [("room24x32", "A", 8), ("room24x32", "B", 8), ("room30x44", "A", 10), ("room30x44", "B", 10)]


@pytest.mark.parametrize("name,pert,iters", FITS)
def test_fit_ends_where_the_fp64_reference_ends(name, pert, iters):
    """Measured on the MI355X, distance of the GPU's end pose to the reference's in (m, rad) against the bounds: room24x32 A 5.3e-8, 4.8e-8
    (1e-4, 1.03e-4); room24x32 B 7.3e-8, 4.5e-8 (1e-4, 1.04e-4); room30x44 A 3.7e-8, 2.7e-8 and B 2.8e-8, 2.6e-8 (1e-4, 1e-4).  End
    errors to the truth: 1.06 / 1.07 / 0.87 / 0.87 mm and 0.159 / 0.158 / 0.019 / 0.019 degrees."""
    p = AR.PERTURBATION_A if pert == "A" else AR.PERTURBATION_B
    c = dict(AR.case(name, False))
    c["start"] = AR.perturb(c["pose"], *p)
    ref = AR.align(c["values"], c["origin"], c["voxel_size"], c["trunc_voxels"], c["depth"], c["invK"], c["start"], iters=iters)
    out = _align(name, False, c, iters=iters)
    assert (out["records"][:, 29] == 0).all() and ref["statuses"] == [0] * iters
    # the jitter the non-smooth objective leaves in the reference itself: MARGIN times its own last step, floored at 1e-4
    bound_t, bound_r = max(AR.MARGIN * ref["steps"][-1][0], 1e-4), max(AR.MARGIN * ref["steps"][-1][1], 1e-4)
    dt, dr = AR.pose_error(out["world_T_cam"][0], ref["world_T_cam"])
    t0, r0 = AR.pose_error(c["start"], c["pose"])
    t1, r1 = AR.pose_error(out["world_T_cam"][0], c["pose"])
    print(name, pert, "to the reference", dt, dr, "bounds", bound_t, bound_r, "to the truth", t1, np.degrees(r1), "from", t0, np.degrees(r0))
    assert dt <= bound_t and dr <= bound_r
    assert t1 <= t0 / 10 and r1 <= r0 / 4


def test_early_stop():
    name, box = "room30x44", False
    c = dict(AR.case(name, box))
    c["start"] = AR.perturb(c["pose"], *AR.PERTURBATION_A)
    out = _align(name, box, c, iters=10, min_step=1e-3)
    status = out["records"][:, 29]
    n = int((status != 3).sum())
    assert 2 <= n < 10 and (status[:n] == 0).all() and (status[n:] == 3).all()
    assert (np.delete(out["records"][n:], 29, axis=1) == 0).all()
    assert out["records"][n - 1, 30] < 1e-3 and out["records"][n - 1, 31] < 1e-3
    assert (np.maximum(out["records"][:n - 1, 30], out["records"][:n - 1, 31]) >= 1e-3).all()
    exact = _align(name, box, c, iters=n)
    assert exact["world_T_cam"].tobytes() == out["world_T_cam"].tobytes()
    assert exact["records"].tobytes() == out["records"][:n].tobytes()


def test_failure_statuses_keep_the_input_pose():
    from implicit_depth_amd import fusion

    c = dict(AR.case("room24x32", True))
    c["start"] = AR.perturb(c["pose"], *AR.PERTURBATION_A)
    holes = dict(c, depth=np.zeros_like(c["depth"]))
    holes["depth"][3, 4], holes["depth"][5, 6] = np.nan, -1.0
    out = _align("room24x32", True, holes, iters=3)
    assert out["records"][:, 29].tolist() == [1, 3, 3] and out["records"][0, 28] == 0
    assert out["world_T_cam"][0].tobytes() == c["start"].tobytes()
    # fewer than min_count usable pixels, though some
    out = _align("room24x32", True, c, iters=2, min_count=100000)
    assert out["records"][:, 29].tolist() == [1, 3] and out["records"][0, 28] > 300
    assert out["world_T_cam"][0].tobytes() == c["start"].tobytes()
    p = dict(AR.plane_case())
    p["start"] = p["pose"]
    out = _align("plane", False, p, iters=3, return_rows=True)
    assert (out["rows"][..., 0] == 0).all() and out["records"][0, 0] == 0 and out["records"][0, 28] >= 64
    assert out["records"][:, 29].tolist() == [2, 3, 3]
    assert out["world_T_cam"][0].tobytes() == p["start"].tobytes()
    summary = fusion.alignment_summary(torch.from_numpy(out["records"]).cuda())
    assert summary["status"] == 2 and summary["iterations"] == 1 and summary["stopped"]


def test_schedule_is_the_chain_of_calls():
    name, box = "room24x32", False
    c = dict(AR.case(name, box))
    c["start"] = AR.perturb(c["pose"], *AR.PERTURBATION_B)
    chained = _align(name, box, c, schedule=((2, 3), (1, 3)))
    first = _align(name, box, c, stride=2, iters=3)
    second = _align(name, box, c, pose=first["world_T_cam"][0], stride=1, iters=3)
    assert chained["world_T_cam"].tobytes() == second["world_T_cam"].tobytes()
    assert chained["records"].tobytes() == np.concatenate([first["records"], second["records"]]).tobytes()
    assert chained["records"].shape == (6, 40) and chained["records"][0, 28] < chained["records"][3, 28]


def test_method_form_and_refusals():
    from implicit_depth_amd import _lib, fusion

    c = dict(AR.case("room24x32", False))
    vol = _volume("room24x32", False)
    d, iK, T = _cuda(c["depth"])[None, None], _cuda(c["invK"]), _cuda(c["pose"])
    a, b = vol.align(d, iK, T, iters=2), fusion.align_depth(vol, d, iK, T, iters=2)
    assert torch.equal(a["world_T_cam"], b["world_T_cam"]) and torch.equal(a["records"], b["records"])
    assert a["world_T_cam"].shape == (1, 4, 4) and a["records"].dtype == torch.float64 and a["records"].is_cuda
    with pytest.raises(_lib.IdhError):
        fusion.align_depth(vol, d, iK, T, min_count=5)
    with pytest.raises(_lib.IdhError):
        fusion.align_depth(vol, d, iK, T, damping=-1.0)
    with pytest.raises(_lib.IdhError):
        fusion.align_depth(vol, d.requires_grad_(), iK, T)
