"""The op kinds of idh_run_ops other than CONV / STEM, without a GPU: launch counts, import grouping, refusals, and the arithmetic of the
case table that test_op_kinds_gpu.py runs on the device (tests/op_kind_ref.py).

idh_count_launches replays idh_run_ops' validation and launch decisions and touches no device.  The refusal rows are additionally sent
through idh_run_ops itself with made-up pointers: a descriptor refused there without a device present was refused before any launch, which
is what allows the GPU file to run the same rows against real buffers."""
import pytest
import torch

import op_kind_ref as K


def _lib_nhwc():
    from implicit_depth_amd import _lib, nhwc

    return _lib.lib(), nhwc


def _count(L, nhwc, ops):
    arr, p = K.op_array(nhwc, ops)
    return L.idh_count_launches(p, len(ops))


def test_every_declared_kind_has_cases():
    """Every IDH_OP_* of the header other than CONV, STEM and the reserved number has small cases and refusal rows here, under the code the
    header gives it; and no descriptor of the tables is accepted under a kind number the tables do not know."""
    L, nhwc = _lib_nhwc()
    declared = K.declared_kinds()
    here = {name: code for code, name in K.KINDS.values()}
    assert declared == {**here, **K.NOT_HERE, **K.RESERVED}, sorted(set(declared) ^ set({**here, **K.NOT_HERE, **K.RESERVED}))
    assert (nhwc.OP_IMPORT, nhwc.OP_EXPORT, nhwc.OP_COPY, nhwc.OP_UPSAMPLE2_NEAREST, nhwc.OP_UPSAMPLE2, nhwc.OP_HEAD, nhwc.OP_POINTWISE_NCHW,
            nhwc.OP_POINTWISE_UP, nhwc.OP_INSTNORM) == tuple(K.KINDS[k][0] for k in ("import", "export", "copy", "nearest", "up2", "head", "pw_nchw", "pw_up", "instnorm"))
    for k in K.KINDS:
        assert any(c.kind == k for c in K.CASES), k
        assert any(r[1].kind == k for r in K.REFUSALS), k
    assert {c.kind for c in K.LARGE} == set(K.CAPS)
    # a kind number idh_run_ops accepts beyond the declared ones would accept one of these well-formed descriptors
    known = set(declared.values())
    for spec in {c.kind: c for c in K.CASES}.values():
        for code in range(0, 64):
            if code in known:
                continue
            op = K.build_op(nhwc, spec, K.fake_ptr)
            op.kind = code
            assert _count(L, nhwc, [op]) == K.EINVAL, (spec.name, code)


@pytest.mark.parametrize("spec", K.CASES + K.LARGE, ids=lambda s: s.name)
def test_accepted_case_and_its_launch_count(spec):
    """1 launch for every kind but INSTNORM (statistics, finalise[, apply])."""
    L, nhwc = _lib_nhwc()
    assert _count(L, nhwc, [K.build_op(nhwc, spec, K.fake_ptr)]) == spec.launches
    assert spec.launches == (1 if spec.kind != "instnorm" else 3 if spec.out else 2)
    assert spec.N >= 2


def test_the_case_table_has_the_shapes_the_kernels_can_go_wrong_at():
    of = lambda k: [c for c in K.CASES if c.kind == k]
    hw = lambda k: {c.H * c.W for c in of(k)}
    assert {c.C for c in of("import")} == {3, 24, 70} and hw("import") == {1, 63, 65, 221}
    assert {c.C for c in of("export")} == {1, 32, 70} and hw("export") == {1, 64, 65, 221} and all(c.in_cs > c.C for c in of("export"))
    for k in ("copy", "nearest"):
        assert {(c.C, c.H, c.W) for c in of(k)} == {(Cc, H, W) for Cc in (4, 68) for H, W in ((1, 1), (5, 7))}
        assert all(c.in_cs > c.C and c.out_cs > c.C and c.in_cs != c.out_cs for c in of(k))
    assert {(c.C, c.H, c.W) for c in of("up2")} == {(Cc, H, W) for Cc in (4, 64) for H, W in ((1, 1), (1, 9), (9, 1), (5, 7))}
    assert {(c.C, c.bias, c.exp) for c in of("head")} == {(Cc, b, e) for Cc in (4, 64, 68) for b in (True, False) for e in (True, False)}
    assert all(c.in_cs > c.C for c in of("head"))
    assert hw("pw_nchw") == {1, 15, 64, 65, 70} and all(c.N == 3 and c.out_cs == 136 for c in of("pw_nchw")) and {c.bias for c in of("pw_nchw")} == {True, False}
    assert {(c.C, c.H, c.W, c.bias) for c in of("pw_up")} == {(Cc, H, W, b) for Cc in (64, 128) for H, W in ((2, 2), (2, 34), (6, 12)) for b in (True, False)}
    assert all(c.in_cs == 3 * c.C and c.low_cs == c.C + 8 and c.out_cs > c.C for c in of("pw_up"))
    assert {(c.C, c.H * c.W) for c in of("instnorm") if c.out} == {(Cc, n) for Cc in (4, 64) for n in (1000, 1024, 1025)}
    assert sum(not c.out for c in of("instnorm")) == 1 and all(c.in_cs > c.C and c.out_cs > c.C for c in of("instnorm"))


# ------------------------------------------------------------------------------------------------------------------
# grouped imports
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", K.IMPORT_GROUPS, ids=lambda g: g[0])
def test_import_group_launch_counts(group):
    L, nhwc = _lib_nhwc()
    name, members, ids, launches = group
    ptr = lambda m: (lambda nm: K.fake_ptr(m.name + nm))
    assert _count(L, nhwc, [K.build_op(nhwc, m, ptr(m), g) for m, g in zip(members, ids)]) == launches
    assert _count(L, nhwc, [K.build_op(nhwc, m, ptr(m), 0) for m in members]) == len(members)


def test_import_group_table_is_what_it_claims():
    g = {name: (members, ids, launches) for name, members, ids, launches in K.IMPORT_GROUPS}
    blocks = lambda m: -(-m.H * m.W // 64) * -(-m.C // 32) * m.N
    assert len(g["pyramid-of-five"][0]) == 5 and g["pyramid-of-five"][2] == 1
    assert len(g["nine-members"][0]) == K.K_MAX_IMPORT + 1 and g["nine-members"][2] == 2
    assert g["group-0"][1] == [0, 0, 0] and g["group-0"][2] == 3
    assert g["two-ids"][1] == [3, 3, 4, 4] and g["two-ids"][2] == 2
    small, large = g["large-member"][0]
    assert blocks(small) <= K.IMPORT_GROUP_MAX_BLOCKS < blocks(large) and g["large-member"][2] == 2
    for name, (members, ids, launches) in g.items():
        if name != "large-member":
            assert all(blocks(m) <= K.IMPORT_GROUP_MAX_BLOCKS for m in members)


def test_an_import_does_not_share_a_grid_with_another_kind():
    L, nhwc = _lib_nhwc()
    imp = next(c for c in K.CASES if c.kind == "import")
    cp = next(c for c in K.CASES if c.kind == "copy")
    ops = [K.build_op(nhwc, imp, lambda nm: K.fake_ptr("a" + nm), 7), K.build_op(nhwc, cp, lambda nm: K.fake_ptr("b" + nm), 7)]
    assert _count(L, nhwc, ops) == 2
    assert _count(L, nhwc, [ops[0]] * 2) == 1  # (the same id on two imports does)


# ------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refusal", K.REFUSALS, ids=lambda r: r[0])
def test_refusals_and_their_codes(refusal):
    """One mutation per validation rule.  The dry run and the real entry point answer the same - without a device, so before any launch."""
    L, nhwc = _lib_nhwc()
    name, spec, mutate, code = refusal
    op = K.build_op(nhwc, spec, K.fake_ptr)
    assert _count(L, nhwc, [op]) == spec.launches  # the unmutated descriptor is a valid one
    mutate(op)
    assert code in (K.EINVAL, K.EUNSUPPORTED)
    assert _count(L, nhwc, [op]) == code
    arr, p = K.op_array(nhwc, [op])
    assert L.idh_run_ops(p, 1, None) == code


def test_refusal_table_covers_the_rules_added_with_it():
    names = {r[0] for r in K.REFUSALS}
    for k in ("copy", "nearest", "export", "head"):
        for what in ("h-zero", "w-zero", "cin-zero", "cs-below-cin"):
            assert f"{k}-NEW-{what}" in names
    assert {"copy-NEW-out-cs-below-cin", "nearest-NEW-out-cs-below-cin", "head-NEW-n-zero", "instnorm-NEW-h-zero"} <= names


# ------------------------------------------------------------------------------------------------------------------
# the large cases and the grid caps
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", K.LARGE, ids=lambda s: s.name)
def test_large_cases_cross_their_grid_cap_by_a_part(spec):
    """Each large case exceeds its kernel's grid cap, and by less than a quarter of it: only part of the grid takes the extra trip, so a
    kernel that loses its loop, or strides by a wrong amount, shows.  pointwise_nchw's pipelined loop leaves through its first exit after an
    odd number of trips and through its second after an even one: its case has workgroups with 3 and with 4."""
    cap, grid = K.CAPS[spec.kind], K.natural_grid(spec)
    trips, extra = divmod(grid, cap)
    print(f"{spec.name}: {grid} workgroups of work on a grid of {cap}: {extra} workgroups take {trips + 1} trips, the others {trips}")
    if spec.kind == "pw_nchw":
        assert trips == 3 and 0 < extra < cap // 4
        assert (spec.H * spec.W, -(-spec.H * spec.W // K.PW_TILE)) == (70, 2)  # two tiles per image, the second with 6 pixels
    else:
        assert cap < grid < 1.25 * cap and trips == 1
    # every sub-range of the partitioned run stays under the cap, and together they are the whole batch
    rs = K.sub_ranges(spec)
    assert rs[0] == (0, 2) and all(a < b for a, b in rs) and [a for a, b in rs[1:]] == [b for a, b in rs[:-1]] and rs[-1][1] == spec.N
    assert all(K.natural_grid(spec, b - a) <= cap for a, b in rs) and len(rs) >= 3
    # no buffer above 1 GiB
    floats = max(spec.N * spec.image_floats(n) for n in ("x", "low", "out", "exp")) + (2 * spec.image_floats("out") if spec.kind in K.DENSE_OUT else 0)
    assert 4 * floats < 1 << 30
    if spec.kind == "pw_up":
        assert (spec.H, spec.W) == (6, 12)
    if spec.kind == "up2":
        assert 0.75 * (1 << 30) < 4 * floats  # "about 0.8 GB": the largest buffer of the file


def test_mirrored_caps_are_the_sources():
    """The constants of op_kind_ref.py against the named constants of csrc/conv.hip they copy: each is defined ONCE with the mirrored value, is
    the bound of the grid clamp (or the grouping test) inside the run_<kind> function of its op kind, and appears in no other one - a cap that
    changes, or moves to another kind, fails here, before a large case silently stops crossing it."""
    import os
    import re

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "implicit-depth_amd", "csrc", "conv.hip")
    with open(path) as f:
        whole = f.read()
    defs = {}
    for m in re.finditer(r"^constexpr (?:int|unsigned|long long) (k\w+) = ([^;]+);", whole, re.M):
        assert m.group(1) not in defs, m.group(1)  # defined once
        defs[m.group(1)] = m.group(2)

    def value(name):  # products of integer literals and other constants of the file, nothing else
        v = 1
        for f in defs[name].split("*"):
            f = f.strip()
            v *= int(f) if re.fullmatch(r"\d+", f) else value(f)
        return v

    # each run_<kind> is a function of the anonymous namespace: its body ends at the first closing brace in column 0
    body = {m.group(1): whole[m.end():].split("\n}\n")[0] for m in re.finditer(r"^int (run_\w+)\(const idh_op \*ops, int i, int n, RunCtx &ctx\) \{$", whole, re.M)}
    caps = {"kCopyMaxBlocks": (K.CAP_COPY, "run_copy", "std::min(idh_cdiv(npix * (s.Cin >> 2), 256), kCopyMaxBlocks)"),
            "kNearestMaxBlocks": (K.CAP_NEAREST, "run_upsample2_nearest", "std::min(idh_cdiv(tot, 256), kNearestMaxBlocks)"),
            "kHeadMaxBlocks": (K.CAP_HEAD, "run_pointwise_head", "std::min(idh_cdiv(M, 256), kHeadMaxBlocks)"),
            "kUpsampleMaxBlocks": (K.CAP_UP2, "run_upsample2", "std::min(idh_cdiv(quads, 256), kUpsampleMaxBlocks)"),
            "kPwNchwMaxBlocks": (K.CAP_PW_NCHW, "run_pointwise_nchw", "std::min<long long>(pa.tiles, kPwNchwMaxBlocks)"),
            "kPwUpMaxBlocks": (K.CAP_PW_UP, "run_pointwise_up", "std::min<long long>(pa.tiles, kPwUpMaxBlocks)"),
            "kImportGroupMaxBlocks": (K.IMPORT_GROUP_MAX_BLOCKS, "run_nchw_to_nhwc", "blocks > kImportGroupMaxBlocks"),
            "kMaxImport": (K.K_MAX_IMPORT, "run_nchw_to_nhwc", "g.n < kMaxImport")}
    assert set(K.CAPS.values()) <= {v[0] for v in caps.values()} and len(body) == 11, sorted(body)
    for name, (mirrored, fn, use) in caps.items():
        assert value(name) == mirrored, (name, defs[name], mirrored)
        assert use in body[fn], (name, fn)
        assert [f for f in body if name in body[f]] == [fn], name  # ... and is the bound of no other kind
    # ... and that clamp is the function's only one: no bare literal took a cap's place beside it
    for name, (mirrored, fn, use) in caps.items():
        assert body[fn].count("std::min") == use.startswith("std::min") and "if (grid >" not in body[fn], fn
    assert value("kLevelMaxBlocks") == 512 and defs["kImportGroupMaxBlocks"] == "8 * kLevelMaxBlocks" and K.IMPORT_GROUP_MAX_BLOCKS == 512 * 8
    assert K.CAP_PW_NCHW == 256 * 4 * 4 and K.CAP_PW_UP == 256 * 8
    assert "constexpr int kPwCin = 64, kPwCout = 128, kPwTile = 64;" in whole and K.PW_TILE == 64


# ------------------------------------------------------------------------------------------------------------------
# the references check themselves
# ------------------------------------------------------------------------------------------------------------------
ARITH = [c for c in K.CASES if c.kind in ("head", "pw_nchw", "pw_up")]


@pytest.mark.parametrize("spec", ARITH, ids=lambda s: s.name)
def test_fp64_reference_equals_the_fp32_composition_within_the_bound(spec):
    t = K.logical_tensors(spec)
    ref, B = K.reference(spec, t)
    tol = K.tolerance(spec, ref, B)
    got = K.compose_fp32(spec, t)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    err = (got.double() - ref).abs()
    print(f"{spec.name}: fp32 composition, worst err / bound {(err / tol).max().item():.3f}")
    assert (err <= tol).all()
    assert 0.3 < ref.std().item() < 4.0


@pytest.mark.parametrize("name", ["head-c68-bias-exp", "head-c4-nobias", "pw_nchw-7x10-bias", "pw_up-c64-6x12-bias", "pw_up-c128-2x34-nobias"])
def test_bound_catches_one_zeroed_weight(name):
    """The same fp32 composition with ONE weight zeroed leaves the bound, and only at the output channel that weight feeds."""
    spec = next(c for c in K.CASES if c.name == name)
    t = K.logical_tensors(spec)
    ref, B = K.reference(spec, t)
    tol = K.tolerance(spec, ref, B)
    t = dict(t)
    w = t["w"].clone()
    if spec.kind == "head":
        w[spec.C - 1] = 0.0
        co = 0
    else:
        co = spec.cout - 3
        w[co, spec.C - 1] = 0.0
    t["w"] = w
    bad = (K.compose_fp32(spec, t).double() - ref).abs() > tol
    ch = bad[:, 0] if spec.kind == "head" else bad[..., co]
    frac = ch.double().mean().item()
    print(f"{name}: one weight of {spec.C * spec.cout} zeroed -> {100 * frac:.1f} % of the channel's elements leave the bound")
    assert frac > 0.9
    if spec.kind != "head":
        assert not bad[..., :co].any() and not bad[..., co + 1:].any()


def test_data_movement_references():
    """permute / repeat_interleave spelled out once, on a tensor whose value names its own index."""
    spec = next(c for c in K.CASES if c.name == "nearest-c4-5x7")
    x = torch.arange(2 * 5 * 7 * 4, dtype=torch.float32).view(2, 5, 7, 4)
    ref, _ = K.reference(spec, {"x": x})
    assert ref.shape == (2, 10, 14, 4)
    for y in range(10):
        for xx in range(14):
            assert torch.equal(ref[:, y, xx], x[:, y // 2, xx // 2])
    imp = next(c for c in K.CASES if c.name == "import-c3-7x9")
    x = torch.arange(2 * 3 * 7 * 9, dtype=torch.float32).view(2, 3, 7, 9)
    ref, _ = K.reference(imp, {"x": x})
    assert ref.shape == (2, 7, 9, 3) and ref[1, 4, 5, 2] == x[1, 2, 4, 5]
    exp = next(c for c in K.CASES if c.name == "export-c32-8x8")
    x = torch.arange(2 * 8 * 8 * 32, dtype=torch.float32).view(2, 8, 8, 32)
    ref, _ = K.reference(exp, {"x": x})
    assert ref.shape == (2, 32, 8, 8) and ref[1, 30, 4, 5] == x[1, 4, 5, 30]
