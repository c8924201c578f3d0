"""Host side of the depth warp (include/idh_raster.h: idh_depth_warp_fwd; raster.warp_depth / decode_source): the fp64 reference of
tests/warp_ref.py on the committed scenes - its ambiguity caps, that the close-up scene holds what it is there for, the tear rule - the
source id's encoding, and the argument validation of the C entry point and of the Python one."""
import ctypes as C

import numpy as np
import pytest
import torch

import raster_ref as rr
import warp_ref as WR

OK, EINVAL, EUNSUPPORTED, EWORKSPACE = 0, -1, -2, -4
P = 0x1000  # a non-null, 256-byte aligned pointer that validation never dereferences


@pytest.mark.parametrize("name", list(WR.TARGETS))
def test_scenes_stay_under_the_ambiguity_cap(name):
    ref = WR.scene_reference(name)
    cov = (ref["depth"] > 0).mean()
    print(f"{name}: ambiguous {ref['ambiguous'].mean():.4%}, covered {cov:.3f}, drawn {ref['drawn']}, large {ref['large']}, crossing {ref['crossing']}")
    assert ref["ambiguous"].mean() <= rr.AMBIGUOUS_CAP, (name, ref["ambiguous"].mean())
    assert 0.2 < cov < 1.0, (name, cov)  # something is drawn and something is left empty
    if name in WR.PLAIN:
        assert ref["crossing"] == 0


def test_the_closeup_scene_goes_through_the_queue_and_crosses_z0():
    ref = WR.scene_reference("closeup")
    assert ref["large"] > 0 and ref["crossing"] > 0, (ref["large"], ref["crossing"])


def test_the_tear_rule_drops_faces_round_the_box_and_inf_drops_none():
    depth, invK, T, _, _, _ = WR.scene_inputs("24x32")
    _, faces, torn, valid = WR.build(depth[0], invK[0], T[0], 1.1)
    _, _, sheet, _ = WR.build(depth[0], invK[0], T[0], np.inf)
    all_valid = valid.reshape(-1)[faces].all(1)
    assert (sheet == all_valid).all() and 0 < (~all_valid).sum() < len(faces)  # inf: only the invalid taps remove faces
    dropped = sheet & ~torn
    assert dropped.sum() > 0 and (torn <= sheet).all()
    # every torn face touches the box's rim: one corner inside the box, one outside
    inbox = np.zeros((WR.SRC_H, WR.SRC_W), bool)
    inbox[WR.BOX] = True
    fin = inbox.reshape(-1)[faces[dropped]]
    assert (fin.any(1) & ~fin.all(1)).all()
    # the same scene without the box tears nothing at the default ratio
    _, _, smooth, v2 = WR.build(WR.source_depth(box=False), invK[0], T[0], 1.1)
    assert (smooth == v2.reshape(-1)[faces].all(1)).all()
    # exactly at the ratio a face still draws (<=): float32 on both sides
    d = np.full((2, 2), 1.0, np.float32)
    d[1, 1] = np.float32(1.0) * np.float32(1.1)
    assert WR.build(d, invK[0], T[0], 1.1)[2].all()
    d[1, 1] = np.nextafter(d[1, 1], np.float32(2))
    assert WR.build(d, invK[0], T[0], 1.1)[2].tolist() == [True, False]


def test_decode_source_round_trips():
    from implicit_depth_amd import raster

    h, w = 5, 7
    F = 2 * (h - 1) * (w - 1)
    ids = np.arange(3 * F)
    m, i, j, up = raster.decode_source(ids, h, w)
    assert m.max() == 2 and i.max() == h - 2 and j.max() == w - 2 and set(up.tolist()) == {0, 1}
    assert (WR.source_id(m, i, j, up, h, w) == ids).all()
    assert (m == ids // F).all() and (2 * (i * (w - 1) + j) + up == ids % F).all()
    t = torch.tensor([[-1, 0, 1], [F - 1, F, 2 * F + 3]], dtype=torch.int32)
    tm, ti, tj, tu = raster.decode_source(t, h, w)
    assert tm.tolist() == [[-1, 0, 0], [0, 1, 2]] and ti.tolist() == [[-1, 0, 0], [h - 2, 0, 0]]
    assert tj.tolist() == [[-1, 0, 0], [w - 2, 0, 1]] and tu.tolist() == [[-1, 0, 1], [1, 0, 1]]
    # the reference's face list is the one the ids name
    _, faces, _, _ = WR.build(np.ones((h, w), np.float32), np.eye(4), np.eye(4))
    v00 = i * w + j
    want = np.where(up[:, None] == 0, np.stack([v00, v00 + w, v00 + 1], -1), np.stack([v00 + 1, v00 + w, v00 + w + 1], -1))
    assert (faces[ids % F] == want).all()
    with pytest.raises(raster._lib.IdhError):
        raster.decode_source(ids, 1, 7)


def _call(L, **k):
    from implicit_depth_amd import _lib

    a = _lib.DepthWarpArgs()
    base = dict(depth_m1hw=P, src_invK_m44=P, cam_T_src_bm44=P, K_b44=P, depth_b1hw=P, source_bhw=P, workspace=P, workspace_bytes=1 << 24,
                tear_ratio=1.1, empty_depth=-1.0, B=1, M=2, h=4, w=5, H=6, W=7)
    for name, val in {**base, **k}.items():
        setattr(a, name, val)
    return L.idh_depth_warp_fwd(C.byref(a), None)


def test_entry_point_validates_on_the_host():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert L.idh_sizeof_depth_warp_args() == C.sizeof(_lib.DepthWarpArgs) == _lib.DepthWarpArgs().struct_size
    wb = L.idh_depth_warp_workspace_bytes
    need = wb(1, 2, 4, 5, 6, 7)
    assert need % 256 == 0 and need >= 2 * 24 * 4 + 6 * 7 * 8  # the queue (4 B per face and source) and the key plane
    for bad in ((0, 1, 4, 4, 4, 4), (1, 0, 4, 4, 4, 4), (1, 1, 1, 4, 4, 4), (1, 1, 4, 1, 4, 4), (1, 1, 4, 4, 0, 4), (1, 1, 4, 4, 4, 0), (-1, 1, 4, 4, 4, 4)):
        assert wb(*bad) == 0, bad
    r = lambda **k: _call(L, **k)
    assert L.idh_depth_warp_fwd(None, None) == EINVAL and r(struct_size=8) == EINVAL
    for bad in (dict(tear_ratio=0.99), dict(tear_ratio=float("nan")), dict(tear_ratio=-1.0), dict(B=0), dict(M=0), dict(H=0), dict(W=-2),
                dict(h=1), dict(w=1), dict(h=0), dict(depth_m1hw=None), dict(src_invK_m44=None), dict(cam_T_src_bm44=None), dict(K_b44=None),
                dict(depth_b1hw=None)):
        assert r(**bad) == EINVAL, bad
    # valid requests get as far as the workspace check
    for good in (dict(), dict(tear_ratio=1.0), dict(tear_ratio=float("inf")), dict(source_bhw=None),
                 dict(empty_depth=1e9), dict(h=2, w=2)):
        assert r(**good, workspace=None) == EWORKSPACE, good
    assert r(workspace_bytes=need - 1) == EWORKSPACE and r(workspace_bytes=-1) == EWORKSPACE and r(workspace=P + 128) == EWORKSPACE
    assert r(B=300, M=300, workspace_bytes=1 << 40) == EUNSUPPORTED                # B * M in grid y
    assert r(B=40000, M=1, H=256, W=256, workspace_bytes=1 << 40) == EUNSUPPORTED  # B * H * W >= 2^31
    assert r(M=16, h=8200, w=8200, workspace_bytes=1 << 50) == EUNSUPPORTED        # the source id would not fit an int32


def test_python_entry_point_refuses_bad_arguments():
    from implicit_depth_amd import raster
    from implicit_depth_amd._lib import IdhError

    depth, invK, T, K = torch.ones(2, 1, 4, 5), torch.eye(4).expand(2, 4, 4), torch.eye(4).expand(1, 2, 4, 4), torch.eye(4)[None]
    with pytest.raises(IdhError):  # CPU tensors: there is no CPU fallback
        raster.warp_depth(depth, invK, T, K, 6, 7)
    # the float64 composition of the poses, rounded once
    a, b = WR.GENERIC_POSE, WR.CLOSE_POSE
    rel = raster.relative_poses([a, b], [b, np.eye(4), a])
    assert tuple(rel.shape) == (2, 3, 4, 4) and rel.dtype == torch.float32
    assert np.array_equal(rel[1, 2].numpy(), (np.linalg.inv(b) @ a).astype(np.float32))
    assert np.array_equal(rel[0, 1].numpy(), np.linalg.inv(a).astype(np.float32))
    with pytest.raises(IdhError):
        raster.relative_poses([np.eye(3)], [np.eye(4)])
