"""The conv op ABI without a GPU: which kernel each hand-built idh_op of tests/conv_op_ref.py runs on.

idh_conv_variant (include/idh_ops.h) answers with prep_conv's own decision, idh_count_launches with the grouping of
idh_run_ops; neither touches the device.  The same case table is executed against fp64 by test_conv_op_matrix_gpu.py -
these tests make sure each of its cases reaches the kernel it was written for, that together they reach every branch
of launch_conv, and that the requests the header refuses are refused with the documented code."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv_op_ref as R


def _lib_nhwc():
    from implicit_depth_amd import _lib, nhwc

    return _lib.lib(), nhwc


def _count(L, nhwc, ops):
    arr, p = R.op_array(nhwc, ops)
    return L.idh_count_launches(p, len(ops))


@pytest.mark.parametrize("spec", R.CASES, ids=lambda s: s.name)
def test_case_runs_on_the_variant_it_names(spec):
    L, nhwc = _lib_nhwc()
    op = R.build_op(nhwc, spec, R.fake_ptr)
    rc, v = R.variant_of(L, nhwc, op)
    assert rc == R.OK
    assert v == spec.variant, (v, spec.variant)
    assert _count(L, nhwc, [op]) == spec.launches


def test_every_launch_conv_branch_has_a_case():
    """The variants of the accepted cases are exactly the branches of launch_conv."""
    L, nhwc = _lib_nhwc()
    seen = set()
    for spec in R.CASES:
        rc, v = R.variant_of(L, nhwc, R.build_op(nhwc, spec, R.fake_ptr))
        assert rc == R.OK, spec.name
        seen.add(v[:4] + v[5:])
    assert seen == R.LAUNCH_CONV_BRANCHES, (sorted(seen - R.LAUNCH_CONV_BRANCHES), sorted(R.LAUNCH_CONV_BRANCHES - seen))
    assert len(R.LAUNCH_CONV_BRANCHES) == 14 + 9 + 4  # LDS, direct, split-precision (2 tile heights) + F(2x2) + F(4x4)
    # every clamp the table claims is a real one
    assert any(s.split_k > s.S > 1 for s in R.CASES if s.variant[0] == 0) and any(s.split_k > s.S > 1 for s in R.CASES if s.variant[0] != 0)


def test_prep_conv_accepts_nothing_outside_the_kernel_tables():
    """The other direction: whatever prep_conv accepts, launch_conv has a kernel for.  Every direct / LDS case of the table (all its sources,
    paddings, strides, split counts, fused upsampling and normalise-on-load) is asked onto every tile_m x tile_n x Cout of the sweep; a request
    idh_conv_variant accepts must name an entry of LAUNCH_CONV_BRANCHES (so the dry count launches it: 1 + the reduce), a refused one leaves
    the outputs untouched."""
    import copy

    L, nhwc = _lib_nhwc()
    bases = [s for s in R.CASES if s.family in ("direct", "lds")]
    accepted, refused, seen = 0, 0, set()
    for base in bases:
        for tm in (0, 1, 2, 4, 8, 9):
            for tn in (0, 1, 2, 4):
                for cout in (16, 32, 48, 64):
                    spec = copy.copy(base)
                    spec.tile_m, spec.tile_n, spec.cout = tm, tn, cout
                    op = R.build_op(nhwc, spec, R.fake_ptr)
                    rc, v = R.variant_of(L, nhwc, op)
                    what = (base.name, tm, tn, cout, rc, v)
                    if rc != R.OK:
                        assert rc in (R.EINVAL, R.EUNSUPPORTED) and v == (-7,) * 8, what
                        assert _count(L, nhwc, [op]) == rc, what
                        refused += 1
                        continue
                    assert v[:4] + v[5:] in R.LAUNCH_CONV_BRANCHES, what
                    assert 1 <= v[4] <= max(1, spec.split_k) and _count(L, nhwc, [op]) == 1 + (v[4] > 1), what
                    accepted += 1
                    seen.add(v[:4] + v[5:])
    print(f"{len(bases)} base cases x 96 requests: {accepted} accepted on {len(seen)} table entries, {refused} refused")
    assert accepted + refused == 6 * 4 * 4 * len(bases) and refused > 0
    assert seen == {b for b in R.LAUNCH_CONV_BRANCHES if b[0] in (0, 4, 8)}  # the sweep is not vacuous: it reaches all 14 + 9 table entries itself


def test_every_hidden_kernel_template_has_a_case():
    """The Winograd and split-precision launchers pick template arguments the variant tuple does not show (a fused second source, F(4x4)'s
    <PROJ, RES>, the split kernel's SRC2 x tile rows, the grouped F(2x2) kernel with / without second sources): the table reaches each, and
    each of these cases names a descriptor the library accepts on that kernel (test_case_runs_on_the_variant_it_names)."""
    seen = {s.template for s in R.CASES if s.template is not None}
    assert seen == R.KERNEL_TEMPLATES, (seen ^ R.KERNEL_TEMPLATES)
    L, nhwc = _lib_nhwc()
    grouped = set()
    for name, members, launches in R.GROUPS:
        if all(m.kind == "conv" and m.family == "wino" for m in members):
            assert all(R.variant_of(L, nhwc, R.build_op(nhwc, m, R.fake_ptr, 7)) == (R.OK, m.variant) for m in members)
            grouped |= {("conv3x3_wino_group_k", len(m.srcs) > 1) for m in members}
    assert grouped == R.GROUP_KERNEL_TEMPLATES
    # what the issue of the grouped launcher turns on: a run longer than kWinoMaxGroup, a run of mixed second sources, fewer than 8 tiles in all
    tiles = lambda m: m.N * -(-m.Ho // 8) * -(-m.Wo // 32) * (m.cout // 32)
    wino_groups = [g for g in R.GROUPS if all(m.kind == "conv" and m.family == "wino" for m in g[1])]
    assert any(len(g[1]) > R.K_WINO_MAX_GROUP for g in wino_groups)
    assert any(len({len(m.srcs) for m in g[1]}) == 2 for g in wino_groups)
    assert any(sum(tiles(m) for m in g[1]) < 8 for g in wino_groups)
    # ... and of the persistent F(4x4) grid: more tiles than 2 x 256 workgroups, not a multiple of the 8 XCDs
    t4 = [s.N * -(-s.Ho // 8) * -(-s.Wo // 32) * (s.cout // 64) for s in R.CASES if s.family == "wino4"]
    assert any(n > 512 and n % 8 for n in t4)


@pytest.mark.parametrize("group", R.GROUPS, ids=lambda g: g[0])
def test_group_launch_counts(group):
    """Members with one group id share grids as launch_group / launch_level decide; with group = 0 each member launches alone."""
    L, nhwc = _lib_nhwc()
    name, members, launches = group
    build = lambda m, g: R.build_up_op(nhwc, m, R.fake_ptr, g) if m.kind == "up" else R.build_op(nhwc, m, R.fake_ptr, g)
    for m in members:
        if m.kind == "conv":
            rc, v = R.variant_of(L, nhwc, build(m, 7))
            assert (rc, v) == (R.OK, m.variant), m.name
    assert _count(L, nhwc, [build(m, 7) for m in members]) == launches
    alone = sum(1 if m.kind == "up" else m.launches for m in members)
    assert _count(L, nhwc, [build(m, 0) for m in members]) == alone
    assert launches < alone


@pytest.mark.parametrize("refusal", R.REFUSALS, ids=lambda r: r[0])
def test_refusals_and_their_codes(refusal):
    L, nhwc = _lib_nhwc()
    name, spec, mutate, code = refusal
    op = R.build_op(nhwc, spec, R.fake_ptr)
    if mutate is not None:
        assert R.variant_of(L, nhwc, op)[0] == R.OK  # the unmutated descriptor is a valid one
        mutate(op)
    rc, v = R.variant_of(L, nhwc, op)
    assert rc == code
    if code == R.OK:
        assert v == spec.variant and _count(L, nhwc, [op]) == 1
    else:
        assert v == (-7,) * 8  # outputs untouched
        assert _count(L, nhwc, [op]) == code


def test_kind_5_is_reserved():
    """IDH_OP_SPLITK_REDUCE is declared but never accepted: the reduce is implicit in a conv with split_k > 1."""
    L, nhwc = _lib_nhwc()
    assert nhwc.OP_SPLITK == 5
    op = R.build_op(nhwc, R.CASES[0], R.fake_ptr)
    op.kind = nhwc.OP_SPLITK
    assert _count(L, nhwc, [op]) == R.EINVAL
    arr, p = R.op_array(nhwc, [op])
    assert L.idh_run_ops(p, 1, None) == R.EINVAL  # refused before anything is launched
    assert R.variant_of(L, nhwc, op) == (R.EINVAL, (-7,) * 8)
    out = (C.c_int32 * 8)()
    assert L.idh_conv_variant(None, out) == R.EINVAL and L.idh_conv_variant(p, None) == R.EINVAL


def test_elu_constant_covers_the_cpu_measurement():
    """conv_op_ref.ELU_F32_ERR (a term of the GPU tolerance) is the measured error of fp32 F.elu against fp64 on the reference's
    pre-activations of every ELU case, rounded up: no case may exceed it, and it may not be padded beyond 1.5x the measurement."""
    worst = 0.0
    elu = [s for s in R.CASES if s.act == R.ACT_ELU] + [m for g in R.GROUPS for m in g[1] if m.kind == "conv" and m.act == R.ACT_ELU]
    assert len(elu) >= 6
    for spec in elu:
        ref, pre, B = R.reference(spec, R.logical_tensors(spec))
        worst = max(worst, (F.elu(pre.float()).double() - ref).abs().max().item())
    print(f"fp32 elu vs fp64 on the pre-activations: {worst:.3e}")
    assert worst <= R.ELU_F32_ERR <= 1.5 * worst, worst


def test_reference_matches_torch_conv_in_fp32():
    """The fp64 reference and the buffer packing agree with a plain fp32 F.conv2d of the same tensors (guards the helper itself)."""
    spec = next(s for s in R.CASES if s.name == "direct-4x4-proj1x1s2")
    t = R.logical_tensors(spec)
    ref, pre, B = R.reference(spec, t)
    x0, x1 = (t[k].permute(0, 3, 1, 2) for k in ("x0", "x1"))
    y = F.conv2d(x0, t["w0"], padding=1) + F.conv2d(x1, t["w1"], stride=2) + t["bias"][None, :, None, None]
    y = F.leaky_relu(y.permute(0, 2, 3, 1) + t["res"], R.SLOPE)
    assert ((y.double() - ref).abs() <= R.tolerance(spec, ref, B, t)).all()
    assert 0.5 < ref.std().item() < 3.0 and (B >= pre.abs()).all()


# ------------------------------------------------------------------------------------------------------------------
# the Winograd error model of conv_op_ref.tolerance
# ------------------------------------------------------------------------------------------------------------------
WINO_CASES = [s for s in R.CASES if s.family in ("wino", "wino4")] + [m for g in R.GROUPS for m in g[1] if m.kind == "conv" and m.family == "wino"]
_M = {"wino": 2, "wino4": 4}


@pytest.mark.parametrize("m", [2, 4])
def test_winograd_matrices_reproduce_the_convolution(m):
    """(a) The fp64 Winograd algorithm with the A^T, G, B^T that conv_op_ref copied from the kernels equals fp64 conv2d to 1e-12 - at a map with
    row and column tails against the m x m blocks."""
    g = torch.Generator().manual_seed(m)
    x = torch.randn(2, 5, 9, 11, generator=g, dtype=torch.float64)
    w = torch.randn(7, 5, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(x, w, padding=1)
    got = R.wino_conv(x, w, m)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    assert (R.wino_conv(x, w, m, magnitude=True) >= F.conv2d(x.abs(), w.abs(), padding=1) - 1e-12).all()  # B_wino >= B: same terms, no cancellation


def _emulate_fp32(spec, t, w0=None, matrices=None):
    """The op in fp32 on the CPU with source 0 by the Winograd algorithm (transforms, products and sums in fp32)."""
    x0 = t["x0"].permute(0, 3, 1, 2)
    y = R.wino_conv(x0, t["w0"] if w0 is None else w0, _M[spec.family], dtype=torch.float32, matrices=matrices)
    if len(spec.srcs) > 1:
        y = y + F.conv2d(t["x1"].permute(0, 3, 1, 2), t["w1"])
    y = y.permute(0, 2, 3, 1)
    if spec.bias:
        y = y + t["bias"]
    if spec.res:
        y = y + t["res"]
    assert y.dtype == torch.float32
    if spec.act == R.ACT_LRELU:
        y = F.leaky_relu(y, spec.slope)
    elif spec.act == R.ACT_ELU:
        y = F.elu(y)
    return y.double()


@pytest.mark.parametrize("spec", WINO_CASES, ids=lambda s: s.name)
def test_fp32_winograd_emulation_stays_inside_the_bound(spec):
    """(b) What the kernels compute, evaluated in fp32 by torch, obeys the bound the GPU test applies to them."""
    t = R.logical_tensors(spec)
    ref, pre, B = R.reference(spec, t)
    tol = R.tolerance(spec, ref, B, t)
    err = (_emulate_fp32(spec, t) - ref).abs()
    print(f"{spec.name}: fp32 emulation, worst err / bound {(err / tol).max().item():.3f}")
    assert (err <= tol).all()


@pytest.mark.parametrize("name", ["wino-epi-bias-res-lrelu", "wino-proj80-res", "wino4-epi-bias-res-none", "wino4-cin136", "wino4-proj112-elu"])
def test_bound_catches_a_wrong_tap_and_a_wrong_coefficient(name):
    """(c) The bound is loose by design (it follows the magnitudes of the transformed operands), yet tight enough that ONE wrong term shows:
    the same fp32 emulation with one filter tap of one (co, ci) pair zeroed, or one coefficient of B^T replaced by that of the neighbouring
    interpolation point (its sign flipped), leaves the bound at elements the change reaches."""
    spec = next(s for s in R.CASES if s.name == name)
    t = R.logical_tensors(spec)
    ref, pre, B = R.reference(spec, t)
    tol = R.tolerance(spec, ref, B, t)
    m = _M[spec.family]
    # one tap of one channel pair: reaches output channel `co` only, at every pixel
    co, ci = spec.cout - 3, spec.srcs[0].cin - 1
    w = t["w0"].clone()
    w[co, ci, 2, 0] = 0.0
    bad = (_emulate_fp32(spec, t, w0=w) - ref).abs() > tol
    assert not bad[..., :co].any() and not bad[..., co + 1:].any()
    frac = bad[..., co].double().mean().item()
    print(f"{name}: one tap of {9 * spec.srcs[0].cin} zeroed -> {100 * frac:.1f} % of the channel's elements leave the bound")
    assert frac > 0.05
    # one coefficient of the input transform: row 1 takes row 2's entry in column 1 (the points +-1 of F(2x2), +-1/2 of F(4x4), differ by that sign)
    AT, G, BT = R.wino_matrices(m, torch.float32)
    BT = BT.clone()
    assert BT[1, 1] == -BT[2, 1]
    BT[1, 1] = BT[2, 1]
    bad = (_emulate_fp32(spec, t, matrices=(AT, G, BT)) - ref).abs() > tol
    frac = bad.double().mean().item()
    print(f"{name}: one coefficient of B^T wrong -> {100 * frac:.1f} % of all elements leave the bound")
    assert frac > 0.25
