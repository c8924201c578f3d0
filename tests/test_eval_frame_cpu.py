"""Host-side checks of the fused per-frame evaluation (include/idh.h, csrc/eval_frame.hip, implicit-depth_amd/evaluation.py):
the header compiles on its own, the ctypes mirror of idh_eval_args has the C layout, argument errors come back before any
device call, and the score-dict keys match the reference's (golden G14)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden


def _lib():
    from implicit_depth_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib


def test_eval_args_layout_matches_the_header(tmp_path):
    L = _lib()
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "idh.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(idh_eval_args), offsetof(idh_eval_args, prediction), '
                   'offsetof(idh_eval_args, rendered_bphw), offsetof(idh_eval_args, W)); return IDH_EVAL_TAG_BOUNDARY - 4; }\n')
    exe = str(tmp_path / "s")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    size, off_pred, off_rend, off_w = map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    E = L.EvalArgs
    assert size == C.sizeof(E) == L.lib().idh_sizeof_eval_args() == E().struct_size
    assert (off_pred, off_rend, off_w) == (E.prediction.offset, E.rendered_bphw.offset, E.W.offset)
    assert (L.EVAL_TAG_ALL, L.EVAL_TAG_SURFACE, L.EVAL_TAG_BOUNDARY, L.EVAL_NEAREST, L.EVAL_PRED_DEPTH) == (1, 2, 4, 1, 1)


def _args(L, **kw):
    a = L.EvalArgs()
    a.prediction, a.rendered_bphw, a.depth_b1hw, a.gt_b1HW, a.thresholds = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    a.sigmoid_multiplier, a.surface_threshold, a.T, a.tag_mask = 1.0, 0.05, 5, 7
    a.B, a.P, a.h, a.w, a.H, a.W = 2, 8, 192, 256, 480, 640
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_errors_return_before_any_device_call():
    L = _lib()
    h = L.lib()
    ws_need = h.idh_eval_frame_workspace_bytes(2, 8, 192, 256, 480, 640, 5)
    assert ws_need >= 2 * 3 * 8 * 12 * 4 + 2 * 8 * 192 * 256
    assert h.idh_eval_frame_workspace_bytes(2, 8, 192, 256, 480, 640, 9) == 0
    assert h.idh_eval_frame_workspace_bytes(-1, 8, 192, 256, 480, 640, 5) == 0
    fwd = lambda a, ws=0x8000, n=ws_need, out=0x7000: h.idh_eval_plane_scores_fwd(C.byref(a), out, None, ws, n, None)
    assert h.idh_eval_plane_scores_fwd(None, 0x7000, None, 0x8000, ws_need, None) == -1
    assert fwd(_args(L, struct_size=8)) == -1                       # caller's struct shorter than the library's
    assert fwd(_args(L, T=9)) == -1                                 # at most 8 constant thresholds
    assert fwd(_args(L, T=0)) == -1
    assert fwd(_args(L, H=0)) == -1 and fwd(_args(L, P=0)) == -1    # bad shapes
    assert fwd(_args(L, sampling=2)) == -1 and fwd(_args(L, pred_kind=2)) == -1
    assert fwd(_args(L, tag_mask=0)) == -1 and fwd(_args(L, tag_mask=8)) == -1
    assert fwd(_args(L, bins=0x6000, n_bins=8)) == -1               # the Thresholder takes T = 1
    assert fwd(_args(L, pred_kind=L.EVAL_PRED_DEPTH)) == -1         # the regressed compare takes T = 1
    assert fwd(_args(L, depth_b1hw=None)) == -1                     # surface / boundary need the model-resolution depth
    assert fwd(_args(L, prediction=None)) == -1 and fwd(_args(L, gt_b1HW=None)) == -1
    assert fwd(_args(L), out=None) == -1
    assert fwd(_args(L), ws=None) == -4 and fwd(_args(L), n=ws_need - 1) == -4 and fwd(_args(L), ws=0x8004) == -4
    assert fwd(_args(L, B=0)) == 0                                  # nothing to do
    assert fwd(_args(L, B=70000, P=1)) == -4                        # (validated before the grid limit: the workspace comes first)
    # masks: every output may be NULL, not all three
    assert h.idh_eval_masks_fwd(0x3000, 0x2000, 2, 8, 192, 256, 0.05, None, None, None, None) == -1
    assert h.idh_eval_masks_fwd(None, 0x2000, 2, 8, 192, 256, 0.05, 0x1000, None, None, None) == -1
    assert h.idh_eval_masks_fwd(0x3000, 0x2000, 2, 8, 0, 256, 0.05, 0x1000, None, None, None) == -1
    assert h.idh_eval_masks_fwd(0x3000, 0x2000, 40000, 2, 192, 256, 0.05, 0x1000, None, None, None) == -2  # B*P above the grid's y limit
    assert h.idh_eval_masks_fwd(0x3000, 0x2000, 0, 8, 192, 256, 0.05, None, None, None, None) == 0
    # depth metrics over an upsampled prediction
    dws = h.idh_eval_frame_workspace_bytes(2, 1, 192, 256, 480, 640, 1)
    dm = lambda **k: h.idh_eval_depth_metrics_fwd(k.get("gt", 0x1000), k.get("pred", 0x2000), 2, 192, 256, 480, 640, k.get("s", 0), 0.5, 0,
                                                  k.get("out", 0x3000), k.get("ws", 0x8000), k.get("n", dws), None)
    assert dm(s=3) == -1 and dm(gt=None) == -1 and dm(out=None) == -1
    assert dm(n=64) == -4 and dm(ws=None) == -4 and dm(ws=0x8004) == -4


def test_score_keys_match_the_reference_key_lists():
    """evaluation.bd_score_keys / reg_score_keys (the code path that names bd_frame_scores' / reg_frame_scores' dict) against the key
    lists the reference built for every golden case, order included."""
    from implicit_depth_amd import evaluation as ev

    g = load_golden("g14_eval_frame")
    names = list(g["case_names"])
    assert len(names) >= 9
    for name in names:
        case = json.loads(str(g[f"{name}__case"]))
        P, opts = case["shape"][1], case["opts"]
        if case["loop"] == "bd":
            keys = ev.bd_score_keys(P, thresholder=object() if opts.get("thresholder") else None, temporal_eval=opts.get("temporal_eval", False),
                                    binary_eval_depth=opts.get("binary_eval_depth", False))
        else:
            keys = ev.reg_score_keys(P, opts.get("regression_plane_eval", False), opts.get("temporal_eval", False))
        assert keys == list(g[f"{name}__keys"]), name
        assert g[f"{name}__values"].shape == (case["shape"][0], len(keys))
    # temporal_eval names every plane "-1.0": the reference's dict keeps the first plane's slot and the last plane's value
    k = ev.bd_score_keys(2, temporal_eval=True)
    assert len(k) == len(set(k)) == 3 * 5 * 3 and k[0] == "iou_0.3_d_-1.0"


def test_generator_cases_and_inputs():
    """tests/golden/gen_golden_eval.py's case list is the golden's, its inputs are reproducible and carry the NaN / zero patches, and
    the fixture stays small."""
    import sys

    import torch

    import implicit_depth_amd.synthetic as syn

    sys.path.insert(0, GOLDEN)
    import gen_golden_eval as gen

    g = load_golden("g14_eval_frame")
    assert [c[0] for c in gen.CASES] == list(g["case_names"])
    assert os.path.getsize(os.path.join(GOLDEN, "g14_eval_frame.npz")) < 256 * 1024
    shapes = {c[1][2:6] for c in gen.CASES}
    assert (192, 256, 480, 640) in shapes and (100, 140, 333, 467) in shapes
    o1, c1 = syn.eval_frame_case(2, 3, 100, 140, 333, 467, 2)
    o2, c2 = syn.eval_frame_case(2, 3, 100, 140, 333, 467, 2)
    for k in o1:
        assert torch.equal(o1[k], o2[k])
    for k in c1:
        assert torch.equal(torch.nan_to_num(c1[k]), torch.nan_to_num(c2[k]))
    for k in ("depth_b1hw", "full_res_depth_b1hw"):
        assert torch.isnan(c1[k]).any() and (c1[k] == 0).any()
    # the ambiguity margins leave most (b, tag, d) entries exact
    amb = np.concatenate([g[f"{n}__ambiguous"].ravel() for n in g["case_names"] if f"{n}__ambiguous" in g])
    assert (amb == 0).mean() > 0.5
