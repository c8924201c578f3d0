"""Every kernel variant idh_run_ops can launch for an IDH_OP_CONV, run from a hand-built descriptor and compared with fp64.

The case table, op builder, reference and tolerance live in tests/conv_op_ref.py; test_conv_op_matrix_cpu.py asserts (without
a GPU) that each case reaches the variant it names and that the table covers every branch of launch_conv.  Here each case
runs once on the device: the return code is IDH_OK, the derived elementwise bound holds, and nothing outside the output's
channel slice was written.  Grouped cases additionally match the same ops run alone bit for bit."""
import pytest
import torch

import conv_op_ref as R

pytestmark = pytest.mark.gpu


def _run(ops):
    from implicit_depth_amd import _lib, nhwc

    arr, p = R.op_array(nhwc, ops)
    rc = _lib.lib().idh_run_ops(p, len(ops), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _check(case):
    """Asserts the bound and the untouched surroundings; returns the written slice."""
    spec = case.spec
    got, clean = R.read_output(case)
    ref, pre, B = R.reference(spec, case.t)
    tol = R.tolerance(spec, ref, B, case.t)
    err = (got.double() - ref).abs()
    ok = err <= tol  # (a NaN - an element never written - compares false)
    worst = (err / tol).nan_to_num(nan=float("inf")).max().item()
    print(f"{spec.name} [{getattr(spec, 'family', 'up')}]: max err {err.nan_to_num(nan=float('inf')).max().item():.3e}, max err / bound {worst:.3f}")
    assert ok.all(), f"{spec.name}: {int((~ok).sum())} of {ok.numel()} elements exceed the bound, worst err / bound {worst:.3g}, first at {tuple((~ok).nonzero()[0].tolist())}"
    assert clean, f"{spec.name}: a store landed outside channels [{R.OUT_C0}, {R.OUT_C0 + case.cout}) of the output buffer"
    return got


@pytest.mark.parametrize("spec", R.CASES, ids=lambda s: s.name)
def test_conv_op_matches_fp64(spec):
    from implicit_depth_amd import _lib, nhwc

    case = R.make_conv_case(spec, "cuda")
    assert R.variant_of(_lib.lib(), nhwc, case.op) == (R.OK, spec.variant)  # with the real pointers too
    assert _run([case.op]) == R.OK
    _check(case)


@pytest.mark.parametrize("group", R.GROUPS, ids=lambda g: g[0])
def test_grouped_launch_matches_fp64_and_the_ops_run_alone(group):
    from implicit_depth_amd import _lib, nhwc

    name, members, launches = group
    cases = [R.make_conv_case(m, "cuda", group=7) for m in members]
    ops = [c.op for c in cases]
    arr, p = R.op_array(nhwc, ops)
    assert _lib.lib().idh_count_launches(p, len(ops)) == launches
    assert _run(ops) == R.OK
    together = [_check(c) for c in cases]
    for c, grouped in zip(cases, together):
        R.prefill(c)
        c.op.group = 0
        assert _run([c.op]) == R.OK
        alone = _check(c)
        assert torch.equal(alone.view(torch.int32), grouped.view(torch.int32)), f"{c.spec.name}: grouped and lone launch differ in bits"
