"""The conv op ABI without a GPU: which kernel each hand-built idh_op of tests/conv_op_ref.py runs on.

idh_conv_variant (include/idh_ops.h) answers with prep_conv's own decision, idh_count_launches with the grouping of
idh_run_ops; neither touches the device.  The same case table is executed against fp64 by test_conv_op_matrix_gpu.py -
these tests make sure each of its cases reaches the kernel it was written for, that together they reach every branch
of launch_conv, and that the requests the header refuses are refused with the documented code."""
import ctypes as C

import pytest
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
    """The variants of the accepted cases are exactly the non-Winograd, non-split-precision branches of launch_conv."""
    L, nhwc = _lib_nhwc()
    seen = set()
    for spec in R.CASES:
        rc, v = R.variant_of(L, nhwc, R.build_op(nhwc, spec, R.fake_ptr))
        assert rc == R.OK, spec.name
        seen.add(v[:4] + v[5:])
    assert seen == R.LAUNCH_CONV_BRANCHES, (sorted(seen - R.LAUNCH_CONV_BRANCHES), sorted(R.LAUNCH_CONV_BRANCHES - seen))
    assert len(R.LAUNCH_CONV_BRANCHES) == 14 + 9
    # every clamp the table claims is a real one
    assert any(s.split_k > s.S > 1 for s in R.CASES if s.variant[0] == 0) and any(s.split_k > s.S > 1 for s in R.CASES if s.variant[0] != 0)


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
    assert ((y.double() - ref).abs() <= R.tolerance(spec, ref, B)).all()
    assert 0.5 < ref.std().item() < 3.0 and (B >= pre.abs()).all()
