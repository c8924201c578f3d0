"""The LDS-window kernel of the dot-product volume (cv_dot_win_k, csrc/cost_volume_dot.hip) under every plane split its launcher can choose.

The launcher gives one workgroup 1, 2 or a multiple of 4 four-plane *units* (cv_win_split).  With 1 unit only 4-plane and single-plane runs
exist; 2 units add 8-plane runs, 4 add 16-plane runs and the super-group flush, 8 and more several super-groups per workgroup, and a launch
whose workgroups own all planes finishes the arg-max in the kernel.  The automatic rule reaches the larger splits only at shapes whose fp64
oracle takes minutes (64 frames of 96 x 128), so the cases here force the split (idh_volume_opts.win_units_per_split) on 3 x 3-tile maps
with a ragged last tile column and row.  Every case is checked

  * against the fp64 oracle with the bars the suite already uses for the same input generator,
  * bit for bit against the same inputs at 1 unit per workgroup (every plane sums its views in the same order with the same FMA chain,
    from LDS or from global memory, and the first maximum wins),
  * bit for bit between no scratch, a scratch that holds only the arg-max partials, and a full scratch (run lists built by cv_runs_k),
  * and through the run lists cv_runs_k left in the scratch: what the kernel actually ran (``check_run_lists``).

``CASES`` is imported by tests/test_cost_volume_split_cpu.py, which asserts that it covers the splits listed there."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
import volume_geometry as vg
from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu

C16 = 16
B = 2
MAPS = ((24, 80), (20, 67))  # 3 x 3 tiles of 32 x 8, the last column (16 / 3 pixels) and row (8 of 8 / 4 of 8) ragged
TILE_W, TILE_H, WIN_W, WIN_H, RUNS_PER_PAIR = 32, 8, 48, 12, 16  # kTileW, kTileH, kWW, kWH, kRunsPerPair of csrc/cost_volume_dot.hip
KERNEL_WINDOW = 3  # IDH_CV_KERNEL_WINDOW

# (K, D, forced units): what each row reaches
SPLIT_ROWS = [
    (2, 64, (1, 2, 4, 8, 16)),  # every run length; psplit = 16 ... 1
    (4, 64, (16,)),             # 16 pairs, four super-groups, psplit = 1
    (8, 64, (8,)),              # 16 pairs, two super-groups
    (16, 64, (4,)),             # 16 pairs, one super-group
    (5, 96, (12,)),             # 15 pairs, three super-groups, psplit = 2
    (2, 96, (24,)),             # six super-groups, psplit = 1
    (3, 50, (4, 8, 16)),        # 13 units: splits 8 + 5, last unit of 2 planes, partial last super-group
    (7, 20, (2, 4, 8)),         # 5 units, 14 pairs at 8, psplit = 1
    # the remaining (psplit == 1 | > 1) x units combinations
    (2, 4, (1,)), (2, 8, (2,)), (2, 16, (4,)), (2, 48, (12,)),  # one workgroup owns all planes with 1, 2, 4 and 12 units
    (3, 96, (16,)), (2, 130, (24,)),                             # 16 + 8 and 24 + 9 units over two workgroups
]
# every geometry family at (K = 2, D = 64, units 2 / 4 / 16) and at two of the 16-pair rows
FAMILY_ROWS = [(2, 64, (2, 4, 16)), (4, 64, (16,)), (8, 64, (8,))]
FAMILIES = ("random0", "random1", "zcross", "intrinsics", "roll_pitch", "planes_pixel", "planes_const")
# "syn" bars: rel_err < TOL, arg-max plane mismatch < 5e-3 (tests/test_cost_volume_gpu.py); the others: the statistical bars of
# tests/test_cost_volume_stress_gpu.py (check_vs_fp64)
SYN_BARS = ("syn", "planes_pixel", "planes_const")


def _cases():
    out = []
    for i, (K, D, units) in enumerate(SPLIT_ROWS):
        out += [("syn", K, D, u, MAPS[i % 2]) for u in units]
    for fam in FAMILIES:
        for i, (K, D, units) in enumerate(FAMILY_ROWS):
            out += [(fam, K, D, u, MAPS[0 if i == 0 else 1]) for u in units]
    # four views in front of the camera, rolled by about 90 degrees: a tile's 32-pixel edge spans more source rows than the 12-row window, so
    # every plane of every view is its own global-tap entry -> tasks whose list is full (4 super-groups x 4 views x 16 planes = 256 entries)
    out.append(("rolled", 4, 64, 16, MAPS[0]))
    return out


CASES = _cases()
case_id = lambda c: f"{c[0]}-K{c[1]}-D{c[2]}-u{c[3]}-{c[4][0]}x{c[4][1]}"


def query_plan(Bn, K, H, W, D, kernel=KERNEL_WINDOW, units=0):
    """idh_cost_volume_dot_plan -> (rc, dict): the split and the scratch layout of a launch (host only, no GPU needed)"""
    from implicit_depth_amd import _lib

    ps, un, rs = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    pf, sf = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    rc = _lib.lib().idh_cost_volume_dot_plan(Bn, K, C16, H, W, D, kernel, units, ctypes.byref(ps), ctypes.byref(un), ctypes.byref(pf), ctypes.byref(rs),
                                             ctypes.byref(sf))
    return rc, {"psplit": ps.value, "units": un.value, "partial_floats": pf.value, "runs_stride": rs.value, "scratch_floats": sf.value}


def case_plan(case):
    fam, K, D, units, (H, W) = case
    rc, p = query_plan(B, K, H, W, D, KERNEL_WINDOW, units)
    assert rc == 0, case
    nunits = -(-D // 4)
    p["pairs"] = (min(p["units"], nunits) + 3) // 4 * K  # (super-groups of the largest task) x views
    return p


# ---- inputs and oracle of one (family, K, D, map): built once, shared by the splits of that group ---------------------------------------
def _rolled_inputs(K, H, W):
    inp = syn.cost_volume_inputs(B, K, C16, H, W, seed=11)
    poses = np.tile(np.eye(4), (B, K, 1, 1))
    for b in range(B):
        for k in range(K):
            poses[b, k, :3, :3] = vg.rot(np.array([0.0, 0.0, 1.0]), math.radians((90.0, -90.0, 87.0, -93.0)[k % 4]))
            poses[b, k, :3, 3] = [0.01 * (k - 1.5), 0.005 * b, 0.0]
    inp["src_poses"] = torch.tensor(poses, dtype=torch.float32)
    inp["src_extrinsics"] = torch.tensor(np.linalg.inv(poses), dtype=torch.float32)
    return inp


@functools.lru_cache(maxsize=None)
def _group(fam, K, D, hw):
    """-> dict: CPU inputs, depth range, caller planes (or None), fp64 oracle (cost, lowest)"""
    from oracle import cost_volume as ocv

    H, W = hw
    planes = None
    if fam in SYN_BARS:
        inp = syn.cost_volume_inputs(B, K, C16, H, W, seed=B + K, behind_view=K - 1, big_rotation_view=0)
        lo, hi = 0.25, 5.0
        if fam == "planes_pixel":
            planes = syn.custom_depth_planes(B, D, H, W, seed=4)
        elif fam == "planes_const":  # image-constant planes handed over as an expand()ed (B, D, 1, 1) view
            planes = syn.custom_depth_planes(B, D, H, W, seed=5)[:, :, :1, :1].contiguous().expand(B, D, H, W)
    elif fam == "rolled":
        inp, lo, hi = _rolled_inputs(K, H, W), 0.25, 5.0
    else:
        if fam in ("random0", "random1", "zcross"):
            rng = np.random.default_rng({"random0": 4200, "random1": 4201, "zcross": 4300}[fam])
            inp = vg.random_geometry(rng, B, K, H, W)
            lo = float(rng.uniform(0.2, 1.0))
            hi = lo * float(rng.uniform(3.0, 20.0))
            if fam == "zcross":
                inp = vg.cross_source_plane(rng, inp, H, W, lo, hi)
            g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
            inp["cur_feats"] = torch.randn(B, C16, H, W, generator=g)
            inp["src_feats"] = torch.randn(B, K, C16, H, W, generator=g)
        else:
            inp = vg.build_case(fam, 100 + K, B, K, C16, H, W)
            lo, hi = inp["min_depth"], inp["max_depth"]
    d = {k: v.double() for k, v in inp.items() if torch.is_tensor(v)}
    ref, rlow, _ = ocv.cost_volume_dot(d["cur_feats"], d["src_feats"], d["src_extrinsics"], d["src_Ks"], d["cur_invK"], lo, hi, D,
                                       planes_bdhw=None if planes is None else planes.double())
    return {"inp": inp, "lo": lo, "hi": hi, "planes": planes, "ref": ref, "rlow": rlow}


@functools.lru_cache(maxsize=4)
def _device_group(fam, K, D, hw):
    from implicit_depth_amd.cost_volume import to_nhwc

    g = _group(fam, K, D, hw)
    inp = {k: v.cuda() for k, v in g["inp"].items() if torch.is_tensor(v)}
    dev = {"Ks": inp["src_Ks"].contiguous(), "E": inp["src_extrinsics"].contiguous(), "iK": inp["cur_invK"].contiguous(),
           "planes": None if g["planes"] is None else g["planes"].cuda()}
    cur, src = to_nhwc(inp["cur_feats"]), to_nhwc(inp["src_feats"])
    if g["planes"] is not None:  # one (B, K+1, H, W, C) feature buffer addressed with batch strides, NHWC output with a channel stride > D
        dev["feats"] = torch.cat([cur[:, None], src], 1).contiguous()
        dev["pad"] = 8
    else:
        dev["cur"], dev["src"], dev["pad"] = cur, src, 0
    return dev


PAD_FILL = -7.0


def _launch(case, units, scratch):
    """one forced-split launch through the C ABI -> (cost (B,D,H,W), lowest, int32 view of the run lists or None).  ``scratch``: "none",
    "partials" (a scratch that ends behind the arg-max partials) or "full"."""
    from implicit_depth_amd import _lib
    from implicit_depth_amd.cost_volume import volume_opts

    fam, K, D, _, (H, W) = case
    g, dev = _group(fam, K, D, (H, W)), _device_group(fam, K, D, (H, W))
    rc, plan = query_plan(B, K, H, W, D, KERNEL_WINDOW, units)
    assert rc == 0
    hw = H * W * C16
    if "feats" in dev:
        cur_ptr, src_ptr, cbs, sbs = dev["feats"].data_ptr(), dev["feats"].data_ptr() + 4 * hw, (K + 1) * hw, (K + 1) * hw
    else:
        cur_ptr, src_ptr, cbs, sbs = dev["cur"].data_ptr(), dev["src"].data_ptr(), 0, 0
    opts, keep = volume_opts(B, K, C16, H, W, D, dev["planes"], cbs, sbs, kernel=KERNEL_WINDOW, dot_scratch_device=None if scratch == "none" else "cuda",
                             win_units=units)
    runs = None
    if scratch != "none":
        assert opts.scratch_floats == plan["scratch_floats"] > 0
        keep[0].zero_()  # (a list cv_runs_k left unwritten would read as empty and show as a wrong volume)
        if scratch == "partials":
            opts.scratch_floats = plan["partial_floats"]
        else:
            runs = keep[0].view(torch.int32)[plan["partial_floats"]:]
    pad = dev["pad"]
    if pad:
        out = torch.full((B, H, W, D + pad), PAD_FILL, device="cuda")
    else:
        out = torch.empty(B, D, H, W, device="cuda")
    low = torch.full((B, H, W), -1.0, device="cuda")
    _lib.check(_lib.lib().idh_cost_volume_dot_ex_fwd(cur_ptr, src_ptr, dev["Ks"].data_ptr(), dev["E"].data_ptr(), dev["iK"].data_ptr(), g["lo"], g["hi"],
                                                     B, K, C16, H, W, D, out.data_ptr(), D + pad if pad else 0, low.data_ptr(), None, opts,
                                                     _lib.stream_ptr()), "idh_cost_volume_dot_ex_fwd")
    torch.cuda.synchronize()
    if pad:
        assert bool((out[..., D:] == PAD_FILL).all()), (case, units, scratch, "padding channels of the NHWC output were written")
        out = out[..., :D].permute(0, 3, 1, 2)
    return out.cpu(), low.cpu(), None if runs is None else runs.cpu().numpy(), plan


@functools.lru_cache(maxsize=None)
def _baseline(fam, K, D, hw):
    """the same inputs with ONE unit per workgroup (what every other window test of the suite runs)"""
    cost, low, _, plan = _launch((fam, K, D, 1, hw), 1, "full")
    assert plan["units"] == 1
    return cost, low


# ---- what the kernel actually ran ----------------------------------------------------------------------------------------------------
def check_run_lists(runs, plan, K, H, W, D):
    """The run lists cv_runs_k left ([task][runs_stride] = {count, (xy, info) x count}, task = ((b ty) tx) psplit + group; RunEntry::info =
    wneed | hneed << 8 | mode << 16 | j0 << 18 | (L - 1) << 22 | pair << 26): asserts their invariants, returns what occurred."""
    psplit, per, stride = plan["psplit"], plan["units"], plan["runs_stride"]
    nunits = -(-D // 4)
    tiles = -(-W // TILE_W) * -(-H // TILE_H)
    ntasks = B * tiles * psplit
    assert runs.size == ntasks * stride
    seen = {"win16": 0, "win8": 0, "win4": 0, "win1": 0, "global": 0, "skipped_planes": 0, "full_tasks": 0, "max_count": 0, "full_task_ids": []}
    for t in range(ntasks):
        sp = t % psplit
        ua, ub = sp * per, min(sp * per + per, nunits)
        sg0 = ua >> 2
        nsg = ((ub + 3) >> 2) - sg0
        pairs = nsg * K
        row = runs[t * stride:(t + 1) * stride]
        cnt = int(row[0])
        assert 0 <= cnt <= pairs * RUNS_PER_PAIR and 1 + 2 * cnt <= stride, (t, cnt, pairs)
        seen["max_count"] = max(seen["max_count"], cnt)
        if cnt == 256:
            seen["full_tasks"] += 1
            seen["full_task_ids"].append(t)
        covered, run_planes = {}, {}
        last_pair = -1
        for i in range(cnt):
            xy, info = int(row[1 + 2 * i]), int(row[2 + 2 * i])
            wneed, hneed, mode = info & 0xFF, (info >> 8) & 0xFF, (info >> 16) & 3
            j0, L, pair = (info >> 18) & 15, ((info >> 22) & 15) + 1, (info >> 26) & 63
            assert last_pair <= pair < pairs, (t, i, pair, last_pair, pairs)
            last_pair = pair
            sgi = pair // K
            ulo, uhi = max(ua - 4 * (sg0 + sgi), 0), min(ub - 4 * (sg0 + sgi), 4)
            assert 4 * ulo <= j0 and j0 + L <= 4 * uhi, (t, i, j0, L, ulo, uhi)  # inside the task's units
            assert 16 * (sg0 + sgi) + j0 < D, (t, i, "a run that starts behind the last plane")
            end = covered.get(pair, -1)
            assert j0 >= end, (t, i, j0, end)  # ascending and disjoint within the pair
            covered[pair] = j0 + L
            run_planes[pair] = run_planes.get(pair, 0) + min(L, D - 16 * (sg0 + sgi) - j0)  # the real planes it serves
            assert L in (1, 4, 8, 16) and j0 % L == 0
            if mode == 1:  # WM_WINDOW
                x0, y0 = xy & 0xFFFF, xy >> 16
                assert 1 <= wneed <= WIN_W and 1 <= hneed <= WIN_H and 0 <= x0 and x0 + WIN_W <= W and 0 <= y0 and y0 + WIN_H <= H, (t, i, x0, y0, wneed, hneed)
                seen[f"win{L}"] += 1
            else:
                assert mode == 2 and L == 1, (t, i, mode, L)  # WM_GLOBAL leaves only; skipped and descended nodes never reach the list
                seen["global"] += 1
        # planes of this task no entry serves = skipped
        for pair in range(pairs):
            sgi = pair // K
            ulo, uhi = max(ua - 4 * (sg0 + sgi), 0), min(ub - 4 * (sg0 + sgi), 4)
            real = max(min(4 * uhi, D - 16 * (sg0 + sgi)) - 4 * ulo, 0)
            seen["skipped_planes"] += real - run_planes.get(pair, 0)
            assert run_planes.get(pair, 0) <= real
    return seen


WORST = {}  # family -> worst figures, printed by every case


@functools.lru_cache(maxsize=None)
def run_case(idx):
    """all checks of CASES[idx] -> what its run lists held"""
    from test_cost_volume_gpu import _lowest_mismatch
    from test_cost_volume_stress_gpu import check_vs_fp64

    case = CASES[idx]
    fam, K, D, units, (H, W) = case
    g = _group(fam, K, D, (H, W))
    res = {mode: _launch(case, units, mode) for mode in ("none", "partials", "full")}
    cost, low, runs, plan = res["full"]
    nunits = -(-D // 4)
    assert plan["units"] == min(units, 4 * -(-nunits // 4)) and plan["psplit"] == -(-nunits // plan["units"])
    # fp64 oracle
    if fam in SYN_BARS:
        err, mism = rel_err(cost, g["ref"]), _lowest_mismatch(low, g["rlow"])
        print(f"{case_id(case)}: psplit {plan['psplit']} rel_err {err:.3g} arg-max mismatch {mism:.3g}")
        assert err < TOL and mism < 5e-3, (case, err, mism)
        w = WORST.setdefault(fam, {"rel_err": 0.0, "lowest_mismatch": 0.0})
        w["rel_err"], w["lowest_mismatch"] = max(w["rel_err"], err), max(w["lowest_mismatch"], mism)
    else:
        st = check_vs_fp64(cost, low, g["ref"], g["rlow"], case)
        print(f"{case_id(case)}: psplit {plan['psplit']} {st}")
        w = WORST.setdefault(fam, {k: 0.0 for k in st})
        for k in st:
            w[k] = max(w[k], st[k])
    assert float(low.min()) > 0  # every pixel's arg-max plane was written
    # the same bits whatever the scratch holds
    for mode in ("none", "partials"):
        assert torch.equal(res[mode][0], cost), (case, mode, "cost")
        assert torch.equal(res[mode][1], low), (case, mode, "lowest")
    # the same bits as one unit per workgroup
    bcost, blow = _baseline(fam, K, D, (H, W))
    diff = (bcost != cost)
    assert not bool(diff.any()), (case, "cost differs from the 1-unit split", int(diff.sum()), float((bcost - cost).abs().max()))
    assert torch.equal(blow, low), (case, "lowest differs from the 1-unit split")
    seen = check_run_lists(runs, plan, K, H, W, D)
    if fam == "planes_pixel":  # per-pixel planes: the convex-hull argument does not hold, nothing may be skipped
        assert seen["skipped_planes"] == 0, seen
    if fam == "rolled":  # the full lists hold real work: their tiles' costs are non-zero values the oracle confirms (above)
        assert seen["full_tasks"] > 0, seen
        tiles_x, tiles_y = -(-W // TILE_W), -(-H // TILE_H)
        for t in seen["full_task_ids"]:
            lin = t // plan["psplit"]
            tx, ty, b = lin % tiles_x, (lin // tiles_x) % tiles_y, lin // (tiles_x * tiles_y)
            tile = cost[b, :, ty * TILE_H:(ty + 1) * TILE_H, tx * TILE_W:(tx + 1) * TILE_W]
            assert float((tile != 0).float().mean()) > 0.9, (case, t)
    print(f"{case_id(case)}: runs {dict((k, v) for k, v in seen.items() if k != 'full_task_ids')}")
    print(f"worst so far [{fam}]: {WORST[fam]}")
    return seen


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_forced_split_vs_oracle_unit_split_and_scratch(idx):
    run_case(idx)


def test_run_lists_hold_every_kind_of_run():
    """Over the whole case list the launches ran window runs of 16, 8, 4 and 1 planes, global-tap leaves, skipped planes and a task whose
    256-entry list is full - facts read back from the scratch, not hopes about the inputs."""
    total = {}
    for idx in range(len(CASES)):
        for k, v in run_case(idx).items():
            if k == "max_count":
                total[k] = max(total.get(k, 0), v)
            elif k != "full_task_ids":
                total[k] = total.get(k, 0) + v
    print("run lists over all cases:", total)
    for fam, w in WORST.items():
        print(f"worst [{fam}]: {w}")
    for k in ("win16", "win8", "win4", "win1", "global", "skipped_planes", "full_tasks"):
        assert total[k] > 0, (k, total)
    assert total["max_count"] == 256


def test_hook_is_ignored_by_a_struct_that_stops_short_of_it_and_by_the_other_kernels():
    """struct_size short of win_units_per_split: an invalid value there is not read and the launch is the automatic one; the quad kernel never
    reads the field."""
    from implicit_depth_amd import _lib
    from implicit_depth_amd.cost_volume import to_nhwc, volume_opts

    K, D, (H, W) = 2, 64, MAPS[0]
    inp = {k: v.cuda() for k, v in syn.cost_volume_inputs(B, K, C16, H, W, seed=1).items()}
    cur, src = to_nhwc(inp["cur_feats"]), to_nhwc(inp["src_feats"])
    Ks, E, iK = (inp[k].contiguous() for k in ("src_Ks", "src_extrinsics", "cur_invK"))

    def launch(kernel, units, short):
        opts, keep = volume_opts(B, K, C16, H, W, D, kernel=kernel)
        opts.win_units_per_split = units
        if short:
            opts.struct_size = _lib.VolumeOpts.win_units_per_split.offset
        cost, low = torch.empty(B, D, H, W, device="cuda"), torch.empty(B, H, W, device="cuda")
        rc = _lib.lib().idh_cost_volume_dot_ex_fwd(cur.data_ptr(), src.data_ptr(), Ks.data_ptr(), E.data_ptr(), iK.data_ptr(), 0.25, 5.0, B, K, C16, H, W, D,
                                                   cost.data_ptr(), 0, low.data_ptr(), None, opts, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, cost, low

    rc0, c0, l0 = launch(KERNEL_WINDOW, 0, False)
    assert rc0 == 0
    assert launch(KERNEL_WINDOW, 3, False)[0] == -1  # IDH_EINVAL
    rc, c, l = launch(KERNEL_WINDOW, 3, True)
    assert rc == 0 and torch.equal(c, c0) and torch.equal(l, l0)
    rq0, cq0, lq0 = launch(2, 0, False)
    rq, cq, lq = launch(2, 3, False)
    assert rq0 == rq == 0 and torch.equal(cq, cq0) and torch.equal(lq, lq0)
