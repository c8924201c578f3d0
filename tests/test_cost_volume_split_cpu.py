"""The plane split of the dot-product volume's window kernel, without a GPU: idh_cost_volume_dot_plan (the function the launch calls,
csrc/cost_volume_dot.hip: cv_win_plan / cv_win_split) against a plain restatement of the rule, the validation of the test hook
idh_volume_opts.win_units_per_split, the scratch sizes, and the coverage of the case list of tests/test_cost_volume_split_gpu.py."""
import ctypes

from test_cost_volume_split_gpu import B as CASE_B
from test_cost_volume_split_gpu import CASES, KERNEL_WINDOW, case_plan, query_plan

EINVAL, EUNSUPPORTED = -1, -2
cdiv = lambda a, b: -(-a // b)


def split_rule(B, K, H, W, D):
    """cv_win_split restated: whole super-groups per workgroup unless that leaves fewer than 6144 workgroups or more than 16 (super-group,
    view) pairs, then halved; 8- and 4-plane slices while the grid has fewer than 2048 workgroups -> (psplit, units per workgroup)"""
    nunits = cdiv(D, 4)
    tiles = B * cdiv(W, 32) * cdiv(H, 8)
    per = 4 * cdiv(nunits, 4)
    while per > 4 and (tiles * cdiv(nunits, per) < 6144 or (per // 4) * K > 16):
        per = 4 * cdiv(per // 4, 2)
    if per == 4 and tiles * cdiv(nunits, per) < 2048:
        per = 2
    if per == 2 and tiles * cdiv(nunits, per) < 2048:
        per = 1
    return cdiv(nunits, per), per


def window_runs(B, K, H, W, forced):
    """cv_pick_kernel restated for C = 16: does the window kernel take the launch"""
    ok = K > 0 and K * H * W * 16 < 2 ** 31 and W >= 48 and H >= 12 and W < 32768 and H < 32768 and K <= 16
    return ok and (forced or B * cdiv(W, 32) * cdiv(H, 8) >= 96)


def expected_plan(B, K, H, W, D, psplit, per):
    tasks = B * cdiv(W, 32) * cdiv(H, 8) * psplit
    stride = 1 + 2 * cdiv(per, 4) * K * 16
    partial = 2 * psplit * B * H * W if psplit > 1 else 0
    return {"psplit": psplit, "units": per, "partial_floats": partial, "runs_stride": stride, "scratch_floats": partial + tasks * stride}


ZERO = {"psplit": 0, "units": 0, "partial_floats": 0, "runs_stride": 0, "scratch_floats": 0}


def test_operating_points():
    """96 x 128, K = 8, D = 64: the split of every batch size README.md and DESIGN.md quote (a retune of the rule shows up here as a diff)"""
    got = [query_plan(b, 8, 96, 128, 64, kernel=0)[1]["units"] for b in (4, 8, 16, 32, 64)]
    assert got == [1, 2, 4, 4, 8], got
    assert [query_plan(b, 8, 96, 128, 64, kernel=0)[1]["psplit"] for b in (4, 8, 16, 32, 64)] == [16, 8, 4, 4, 2]
    assert query_plan(1, 8, 96, 128, 64, kernel=0) == (0, ZERO)  # a single frame stays on the quad kernel
    assert query_plan(1, 8, 96, 128, 64, kernel=KERNEL_WINDOW)[1]["units"] == 1


def test_rule_replica_over_a_grid():
    from implicit_depth_amd import _lib

    n = 0
    for Bn in (1, 2, 3, 4, 8, 16, 32, 64, 200):
        for K in (1, 2, 5, 8, 16):
            for H, W in ((96, 128), (12, 48), (24, 80), (20, 67), (40, 160), (56, 96), (97, 131), (192, 256), (8, 64), (24, 40)):
                for D in (1, 4, 5, 20, 50, 64, 96, 130, 512):
                    for forced in (0, KERNEL_WINDOW):
                        rc, got = query_plan(Bn, K, H, W, D, kernel=forced)
                        if forced and not window_runs(Bn, K, H, W, True):
                            assert rc == EINVAL, (Bn, K, H, W, D)  # the launch refuses a forced window kernel on a map below 48 x 12
                            continue
                        assert rc == 0
                        want = expected_plan(Bn, K, H, W, D, *split_rule(Bn, K, H, W, D)) if window_runs(Bn, K, H, W, forced) else ZERO
                        assert got == want, (Bn, K, H, W, D, forced, got, want)
                        if not forced:  # idh_cost_volume_dot_scratch_floats is the same code
                            assert int(_lib.lib().idh_cost_volume_dot_scratch_floats(Bn, K, 16, H, W, D)) == want["scratch_floats"]
                        if want["units"]:
                            assert want["units"] in (1, 2) or want["units"] % 4 == 0
                            assert (want["units"] // 4) * K <= 16 and (want["psplit"] - 1) * want["units"] < cdiv(D, 4) <= want["psplit"] * want["units"]
                        n += 1
    assert n > 7000


def test_hook_values():
    H, W = 24, 80
    for D, K in ((64, 2), (50, 3), (20, 7), (96, 2), (4, 2)):
        nunits = cdiv(D, 4)
        top = 4 * cdiv(nunits, 4)
        for units in (1, 2, 4, 8, 12, 16, 24, 28, 64, 4096):
            eff = min(units, top)  # over-large values count as every super-group D has
            rc, got = query_plan(2, K, H, W, D, units=units)
            if (eff // 4) * K > 16:
                assert rc == EINVAL, (D, K, units)
                continue
            assert rc == 0 and got == expected_plan(2, K, H, W, D, cdiv(nunits, eff), eff), (D, K, units, got)
        for bad in (3, 5, 6, 7, 9, 10, 14, 18, -1, -4, -(2 ** 31)):
            assert query_plan(2, K, H, W, D, units=bad)[0] == EINVAL, (D, K, bad)
    # more than 16 (super-group, view) pairs in a workgroup
    assert query_plan(2, 8, H, W, 64, units=12)[0] == EINVAL  # 3 x 8
    assert query_plan(2, 8, H, W, 64, units=16)[0] == EINVAL  # 4 x 8
    assert query_plan(2, 16, H, W, 64, units=8)[0] == EINVAL  # 2 x 16
    assert query_plan(2, 5, H, W, 96, units=16)[0] == EINVAL  # 4 x 5
    assert query_plan(2, 8, H, W, 64, units=8)[0] == 0 and query_plan(2, 16, H, W, 64, units=4)[0] == 0 and query_plan(2, 4, H, W, 64, units=16)[0] == 0
    assert query_plan(2, 8, H, W, 16, units=16)[1]["units"] == 4  # clamped first: one super-group, 8 pairs
    # the field means nothing where another kernel takes the launch
    assert query_plan(2, 2, H, W, 64, kernel=2, units=3) == (0, ZERO)
    assert query_plan(1, 2, 8, 8, 64, kernel=0, units=3) == (0, ZERO)
    # outputs are optional, dimensions are checked
    from implicit_depth_amd import _lib

    assert _lib.lib().idh_cost_volume_dot_plan(2, 2, 16, H, W, 64, KERNEL_WINDOW, 4, None, None, None, None, None) == 0
    for bad in ((0, 2, H, W, 64), (2, -1, H, W, 64), (2, 2, 0, W, 64), (2, 2, H, -5, 64), (2, 2, H, W, 0), (2, 2, H, W, 513), (2, 17, H, W, 64)):
        assert query_plan(*bad)[0] == EINVAL, bad
    assert query_plan(2, 2, H, W, 64, kernel=7)[0] == EINVAL


def test_launch_validates_the_hook_before_it_launches_anything():
    """idh_cost_volume_dot_ex_fwd itself, on a shape whose grid (2^31 workgroups) it refuses with IDH_EUNSUPPORTED behind the validation and in
    front of every launch: no device access either way.  A struct whose struct_size stops short of the field does not have it read."""
    from implicit_depth_amd import _lib

    L = _lib.lib()
    Bn, K, H, W, D = 2 ** 29, 1, 12, 48, 4  # 4 tiles a frame, one plane group

    def rc(units, short=False):
        o = _lib.VolumeOpts()
        o.kernel, o.win_units_per_split = KERNEL_WINDOW, units
        if short:
            o.struct_size = _lib.VolumeOpts.win_units_per_split.offset
        fake = 0x10000  # never dereferenced on the host
        return L.idh_cost_volume_dot_ex_fwd(fake, fake, fake, fake, fake, 0.25, 5.0, Bn, K, 16, H, W, D, fake, 0, None, None, ctypes.byref(o), None)

    assert rc(0) == EUNSUPPORTED
    for ok in (1, 2, 4, 8, 400):
        assert rc(ok) == EUNSUPPORTED, ok
    for bad in (3, 6, -1):
        assert rc(bad) == EINVAL, bad
        assert rc(bad, short=True) == EUNSUPPORTED, bad
    assert _lib.VolumeOpts.win_units_per_split.offset + 4 == ctypes.sizeof(_lib.VolumeOpts)  # the slot that was reserved0: the struct did not grow


def test_scratch_sizing():
    """scratch_floats = arg-max partials + run lists of the reported split; 0 where no window launch happens; monotone in the batch size for
    as long as the split stays what it is.  (Across a change of the automatic split it is NOT monotone, and rightly so: at 96 x 128, K = 8,
    D = 64 five frames in 4-plane slices want 2,952,960 floats, six frames in 8-plane slices 1,771,776 - half the plane groups, half the
    partials per frame.  Under a forced split it is monotone throughout.)"""
    K, H, W, D = 8, 96, 128, 64
    prev, prev_units = 0, 0
    for units in (1, 2, 4, 8):
        sizes = [query_plan(Bn, K, H, W, D, units=units)[1]["scratch_floats"] for Bn in range(1, 70)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), units
    for Bn in range(1, 70):
        rc, p = query_plan(Bn, K, H, W, D, kernel=0)
        assert rc == 0
        if Bn < 2:
            assert p == ZERO  # quad kernel: no scratch
            continue
        assert p["scratch_floats"] == p["partial_floats"] + Bn * 48 * p["psplit"] * p["runs_stride"] > 0
        assert p["partial_floats"] == (2 * p["psplit"] * Bn * H * W if p["psplit"] > 1 else 0)
        assert p["runs_stride"] == 1 + 2 * cdiv(p["units"], 4) * K * 16
        assert p["scratch_floats"] > prev or p["units"] != prev_units, (Bn, p, prev)
        assert p["units"] >= prev_units  # the split only coarsens with the batch
        prev, prev_units = p["scratch_floats"], p["units"]
    # a forced split sizes the scratch of THAT split
    for units in (1, 2, 4, 8):
        p = query_plan(4, K, H, W, D, units=units)[1]
        assert p == expected_plan(4, K, H, W, D, cdiv(16, units), units)
    # volume_opts asks the same query when the kernel or the split is forced (no device: nothing to allocate, the struct is not built)
    assert query_plan(1, K, 24, 32, D, kernel=0)[1]["scratch_floats"] == 0


def test_gpu_case_list_covers_every_split():
    plans = [(c, case_plan(c)) for c in CASES]
    assert all(c[4] in ((24, 80), (20, 67)) for c, _ in plans) and CASE_B == 2
    combos = {(p["psplit"] == 1, p["units"]) for _, p in plans}
    for single in (True, False):
        for units in (1, 2, 4, 8, 12, 16, 24):
            assert (single, units) in combos, (single, units)
    # the (K, D, units) rows
    rows = {(c[1], c[2], c[3]) for c, _ in plans if c[0] == "syn"}
    want = [(2, 64, u) for u in (1, 2, 4, 8, 16)] + [(4, 64, 16), (8, 64, 8), (16, 64, 4), (5, 96, 12), (2, 96, 24)]
    want += [(3, 50, u) for u in (4, 8, 16)] + [(7, 20, u) for u in (2, 4, 8)]
    assert all(r in rows for r in want), [r for r in want if r not in rows]
    # 16 pairs in one workgroup, three ways: (super-groups, K) = (4, 4), (2, 8), (1, 16); and 15 and 14 pairs
    sixteen = {(p["pairs"] // c[1], c[1]) for c, p in plans if p["pairs"] == 16}
    assert {(4, 4), (2, 8), (1, 16)} <= sixteen, sixteen
    assert {15, 14} <= {p["pairs"] for _, p in plans}
    assert all(p["pairs"] <= 16 for _, p in plans)
    # partial last unit / super-group, several super-groups per workgroup with psplit > 1
    assert any(c[2] % 4 and p["units"] >= 4 for c, p in plans) and any(cdiv(c[2], 4) % 4 and p["units"] >= 8 for c, p in plans)
    # every geometry family at K = 2 with 2, 4 and 16 units and at two 16-pair rows
    for fam in ("syn", "random0", "random1", "zcross", "intrinsics", "roll_pitch", "planes_pixel", "planes_const"):
        mine = [(c, p) for c, p in plans if c[0] == fam]
        assert {2, 4, 16} <= {c[3] for c, _ in mine if c[1] == 2 and c[2] == 64}, fam
        assert len({(c[1], c[3]) for c, p in mine if p["pairs"] == 16}) >= 2, fam
    assert any(c[0] == "rolled" and p["pairs"] == 16 and p["psplit"] == 1 for c, p in plans)
