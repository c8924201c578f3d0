"""CPU-side checks of the whole-model C entry (include/idh_model.h): the header is plain C99 / C++, the host-only size query covers every
shipped reference configuration, and idh_model_fwd refuses bad requests before it launches anything (fake device pointers: nothing is
dereferenced on these paths)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def _entry(volume="mlp", decoder="bd", use_prior=False, K=7, D=64, H=96, W=128, with_head=False):
    from hot_helpers import holder
    from implicit_depth_amd.model_abi import ModelEntry

    return ModelEntry.of(holder(K, volume, H, W, D, use_prior=use_prior, decoder=decoder, with_head=with_head))


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_standalone(lang, tmp_path):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.skip("no host compiler")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "idh_model.h"\nint f(void) { idh_model_size_info s; return (int)sizeof(s) + IDH_MODEL_BD; }\n')
    std = ["-std=c99"] if lang == "c" else ["-std=c++11"]
    r = subprocess.run([cc, *std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_version_and_exports():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert L.idh_version() == 112
    for s in ("idh_model_sizes", "idh_model_pack", "idh_model_fwd", "idh_debug_set_plan_observer"):
        assert s in _lib.declared_symbols()


def test_struct_mirrors_match_header():
    """Field offsets of the ctypes mirror equal the C compiler's for the structs a host fills."""
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("no host compiler")
    from implicit_depth_amd import model_abi as m

    structs = {"idh_model_desc": m.ModelDesc, "idh_model_params": m.ModelParams, "idh_model_inputs": m.ModelInputs,
               "idh_model_outputs": m.ModelOutputs, "idh_model_size_info": m.ModelSizes}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "idh_model.h"', "int main(void) {"]
    for cn, py in structs.items():
        tn = cn if cn != "idh_model_params" else "struct idh_model_params"
        lines.append(f'printf("{cn} %zu\\n", sizeof({tn}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cn}.{f} %zu\\n", offsetof({tn}, {f}));')
    lines.append("return 0; }")
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "o.c"), os.path.join(d, "o")
        open(src, "w").write("\n".join(lines))
        r = subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for cn, py in structs.items():
        assert int(got[cn]) == C.sizeof(py), cn
        for f, _ in py._fields_:
            assert int(got[f"{cn}.{f}"]) == getattr(py, f).offset, f"{cn}.{f}"


# every shipped reference config (configs/models/*.yaml): unet_pp decoder, mlp_feature_volume or simple_cost_volume, BD or regression,
# with or without use_prior
CONFIGS = [("mlp", "bd", False), ("mlp", "bd", True), ("mlp", "depth", False), ("dot", "depth", False), ("dot", "bd", False)]


@pytest.mark.parametrize("volume,decoder,use_prior", CONFIGS)
def test_sizes_cover_shipped_configs(volume, decoder, use_prior):
    from implicit_depth_amd import model_abi as m

    e = _entry(volume, decoder, use_prior)
    keys = set()
    for B in (1, 4, 32):
        pm = m.PRIOR_INPUTS if use_prior else m.PRIOR_NONE
        d = e.desc(B, 7, 16, 96, 128, P=2, prior_mode=pm)
        s1, s2 = e.sizes(d, B), e.sizes(d, B)
        assert (s1.weight_floats, s1.workspace_floats, s1.plan_key) == (s2.weight_floats, s2.workspace_floats, s2.plan_key)  # deterministic
        assert s1.weight_floats > 0 and s1.workspace_floats > 0 and s1.conv_ops > 100 and 0 < s1.conv_launches <= s1.conv_ops
        keys.add(s1.plan_key)
    assert len(keys) == 3, "plan_key changes with B"


def test_plan_key_changes_with_k_and_d():
    e7, e8, e96 = _entry(K=7), _entry(K=8), _entry(D=96)
    k = lambda e, K: e.sizes(e.desc(1, K, 16, 96, 128, P=1), 1).plan_key
    assert len({k(e7, 7), k(e8, 8), k(e96, 7)}) == 3


def test_unsupported_descriptors():
    from implicit_depth_amd import _lib
    from implicit_depth_amd import model_abi as m

    L = _lib.lib()
    e = _entry()
    s = m.ModelSizes()
    base = lambda: e.desc(1, 7, 16, 96, 128, P=1)
    for field, val in (("math", 1), ("matching_scale", 2), ("skip_decoder", 1), ("volume", m.VOLUME_ZERO), ("C", 32), ("K", 9), ("D", 40)):
        d = base()
        setattr(d, field, val)
        assert L.idh_model_sizes(C.byref(d), 1, C.byref(s)) == -2, field
    d = base()
    d.net = None
    assert L.idh_model_sizes(C.byref(d), 1, C.byref(s)) == -1
    assert L.idh_model_sizes(C.byref(base()), 0, C.byref(s)) == -1


@pytest.mark.parametrize("mi", [1, 2])
def test_sizes_with_the_matching_head(mi):
    """layer1 input (NCHW / channels-last): the head is part of the plan - more ops, its own key, and it needs the head's parameters."""
    from implicit_depth_amd import _lib
    from implicit_depth_amd import model_abi as m

    e = _entry(with_head=True)
    base = e.sizes(e.desc(4, 7, 16, 96, 128, P=1), 4)
    d = e.desc(4, 7, 16, 96, 128, P=1, matching_input=mi)
    s = e.sizes(d, 4)
    assert s.conv_ops == base.conv_ops + 4 and s.plan_key != base.plan_key
    # the 1x1 conv reads the NCHW map in place (FUSE_HEAD_IMPORT); channels-last takes the generic conv: different op lists
    other = e.sizes(e.desc(4, 7, 16, 96, 128, P=1, matching_input=3 - mi), 4)
    assert other.plan_key != s.plan_key
    d.C = 32  # the head's 3x3 conv makes 16 channels
    assert _lib.lib().idh_model_sizes(C.byref(d), 4, C.byref(m.ModelSizes())) != 0


def test_head_fusion_constants_match_nhwc():
    """The head-fusion switches the C++ builder mirrors equal nhwc.py's defaults."""
    import re

    from implicit_depth_amd import nhwc

    src = open(os.path.join(ROOT, "implicit-depth_amd", "csrc", "networks.hip")).read()
    for cname, pyname in (("kFuseHeadNorm", "FUSE_HEAD_NORM"), ("kFuseHeadImport", "FUSE_HEAD_IMPORT")):
        mt = re.search(rf"constexpr bool {cname} = (true|false);", src)
        assert mt, cname
        assert (mt.group(1) == "true") == bool(getattr(nhwc, pyname)), cname


def _fake_call(e, mutate):
    """idh_model_fwd on fake, well-separated, 256-aligned addresses: every refusal below happens on the host, before any launch."""
    from implicit_depth_amd import _lib
    from implicit_depth_amd import model_abi as m

    B, K, Cc, H, W, P = 1, 7, 16, 96, 128, 2
    d = e.desc(B, K, Cc, H, W, P=P)
    s = e.sizes(d, B)
    nxt = [1 << 40]

    def addr(n=1 << 28):
        a = nxt[0]
        nxt[0] += n
        return a

    i, o = m.ModelInputs(), m.ModelOutputs()
    i.matching_cur, i.matching_src = addr(), addr()
    for k in range(5):
        i.pyramid[k] = addr()
    i.src_cam_T_cur_cam, i.cur_cam_T_src_cam, i.src_K, i.cur_invK, i.rendered_depth = addr(), addr(), addr(), addr(), addr()
    o.pred_0, o.lowest_cost = addr(), addr()
    blob, ws = addr(1 << 34), addr(1 << 34)
    args = dict(blob=blob, wf=s.weight_floats, key=s.plan_key, ws=ws, wsf=s.workspace_floats)
    mutate(args, i, o, d)
    return _lib.lib().idh_model_fwd(C.byref(d), args["blob"], args["wf"], args["key"], B, C.byref(i), C.byref(o), args["ws"], args["wsf"], None)


def test_fwd_refuses_before_launch():
    import torch

    if torch.cuda.is_available():  # fake device addresses: never hand them to a library that could launch on a real device
        pytest.skip("host-side refusals are checked where no GPU is present")
    e = _entry()

    def wrong_key(a, i, o, d):
        a["key"] ^= 1

    def wrong_weight_floats(a, i, o, d):
        a["wf"] -= 1

    def short_ws(a, i, o, d):
        a["wsf"] -= 1

    def out_on_input(a, i, o, d):
        o.pred_0 = i.rendered_depth + 64

    def out_in_ws(a, i, o, d):
        o.lowest_cost = a["ws"] + 4096

    def out_on_out(a, i, o, d):
        o.lowest_cost = o.pred_0

    def missing_input(a, i, o, d):
        i.rendered_depth = None

    assert _fake_call(e, wrong_key) == -1
    assert _fake_call(e, wrong_weight_floats) == -1
    assert _fake_call(e, short_ws) == -4
    assert _fake_call(e, out_on_input) == -1
    assert _fake_call(e, out_in_ws) == -1
    assert _fake_call(e, out_on_out) == -1
    assert _fake_call(e, missing_input) == -1

