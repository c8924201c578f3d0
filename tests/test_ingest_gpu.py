"""The frame ingest on the MI355X (csrc/ingest.hip, implicit_depth_amd/ingest.py) against what Pillow and torch produced on the CPU
(tests/golden/g_ingest.npz, written by tests/golden/gen_golden_ingest.py).  Every comparison is ``torch.equal``: the resized bytes are
Pillow's, the floats are ``to_tensor`` / ``normalize`` of those bytes in IEEE fp32, so there is nothing to tolerate.

The case that would differ if the horizontal pass's result were kept wider than uint8 is ``ingest_ref.WIDE_INTERMEDIATE_CASE``
(the checkerboard with bicubic taps); tests/test_ingest_cpu.py::test_wide_intermediate_case_differs shows on the CPU that it does."""
import os

import numpy as np
import pytest
import torch

import ingest_ref as ref
from conftest import ROOT, TOL, rel_err

pytestmark = pytest.mark.gpu

FILTERS = sorted(ref.FILTER_NAMES)
CASE_IDS = [c[0] for c in ref.COLOR_CASES]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g_ingest.npz")))


def _expected_float(golden, u8_bhw3, table="normalize_table"):
    """(B,3,h,w): the float the reference's loader gives for every resized byte (the tables hold torch's value for each of the 3 x 256)."""
    c = np.arange(3)[None, :, None, None]
    return torch.from_numpy(golden[table][c, np.moveaxis(u8_bhw3, 3, 1)])


@pytest.mark.parametrize("fname", FILTERS)
@pytest.mark.parametrize("case", ref.COLOR_CASES, ids=CASE_IDS)
def test_load_color_equals_pillow_and_torch(golden, case, fname):
    from implicit_depth_amd import ingest

    name, src, dst = case
    x = torch.from_numpy(golden[f"{name}_in"]).cuda()
    want_u8 = golden[f"{name}_{fname}_u8"]
    img, u8 = ingest.load_color(x, dst, resample=fname, return_u8=True)
    assert img.shape == (3, 3) + dst and img.dtype == torch.float32 and u8.shape == (3,) + dst + (3,) and u8.dtype == torch.uint8
    assert torch.equal(u8.cpu(), torch.from_numpy(want_u8)), f"{name} {fname}: resized bytes"
    assert torch.equal(img.cpu(), _expected_float(golden, want_u8)), f"{name} {fname}: normalised floats"
    # the same floats without the byte output, and to_tensor alone
    assert torch.equal(ingest.load_color(x, dst, resample=fname), img)
    assert torch.equal(ingest.load_color(x, dst, resample=fname, normalize=False).cpu(), _expected_float(golden, want_u8, "to_tensor_table"))


def test_wide_intermediate_case_is_among_the_cases():
    name, fname = ref.WIDE_INTERMEDIATE_CASE
    assert name in CASE_IDS and fname in FILTERS


@pytest.mark.parametrize("fname", FILTERS)
def test_batch_equals_frame_by_frame(golden, fname):
    from implicit_depth_amd import ingest

    x = torch.from_numpy(golden["ragged_in"]).cuda()
    img, u8 = ingest.load_color(x, (33, 65), resample=fname, return_u8=True)
    for b in range(3):
        i1, u1 = ingest.load_color(x[b:b + 1], (33, 65), resample=fname, return_u8=True)
        assert torch.equal(i1[0], img[b]) and torch.equal(u1[0], u8[b])


def test_wide_store_paths_equal_the_reference(golden):
    """Targets whose width is a multiple of 16 (16-byte stores of bytes and floats), of 4 only (float4, bytes one by one) and of neither,
    more than one tile each way, from one source: all equal the restatement."""
    from implicit_depth_amd import ingest

    x = golden["ragged_in"]
    for dst in ((40, 80), (17, 68), (18, 67)):
        want_img, want_u8 = ref.load_color(x, dst, ref.BICUBIC)
        img, u8 = ingest.load_color(torch.from_numpy(x).cuda(), dst, resample="bicubic", return_u8=True)
        assert torch.equal(u8.cpu(), torch.from_numpy(want_u8)) and torch.equal(img.cpu(), torch.from_numpy(want_img)), dst


def test_ratio_above_the_cap_raises(golden):
    from implicit_depth_amd import _lib, ingest

    x = torch.from_numpy(golden["cap8_in"]).cuda()  # 64 x 64
    for dst in ((7, 8), (8, 7)):
        with pytest.raises(_lib.IdhError):
            ingest.load_color(x, dst, resample="bicubic")
    with pytest.raises(_lib.IdhError):
        ingest.load_color(x.float(), (8, 8))
    with pytest.raises(_lib.IdhError):
        ingest.load_color(x[..., :2], (8, 8))
    with pytest.raises(_lib.IdhError):
        ingest.load_depth(x[..., 0])  # uint8 is not a depth


@pytest.mark.parametrize("case", ref.DEPTH_CASES, ids=[c[0] for c in ref.DEPTH_CASES])
def test_load_depth_equals_pillow_and_torch(golden, case):
    from implicit_depth_amd import ingest

    name, src, dst = case
    d = torch.from_numpy(golden[f"{name}_in"]).cuda()
    depth, mask, mask_b = ingest.load_depth(d, dst)
    want = [torch.from_numpy(golden[f"{name}_{k}"]) for k in ("depth", "mask", "mask_b")]
    assert depth.shape == want[0].shape and depth.dtype == torch.float32 and mask.dtype == torch.float32 and mask_b.dtype == torch.bool
    depth, mask, mask_b = depth.cpu(), mask.cpu(), mask_b.cpu()
    assert torch.equal(depth.isnan(), want[0].isnan()) and torch.equal(depth.isnan(), ~want[2])
    assert torch.equal(depth.nan_to_num(-1.0), want[0].nan_to_num(-1.0))
    assert torch.equal(mask, want[1]) and torch.equal(mask_b, want[2])


def _same(a, b):
    """Equal, NaNs in the same places."""
    return torch.equal(a.nan_to_num(-1.0), b.nan_to_num(-1.0)) if a.is_floating_point() else torch.equal(a, b)


def test_frame_ingest_returns_the_reference_dictionary(golden):
    """48x64 images, 24x32 depths: every key of get_frame with its shape and dtype, both depth triples from one call equal to the separate
    calls, matrices equal to the host maths."""
    from implicit_depth_amd import ingest

    B = 2
    frames = torch.from_numpy(golden["ragged_in"][:B]).cuda()  # 75 x 100
    depth = torch.from_numpy(golden["d_half_in"]).cuda()       # 48 x 64
    rng = np.random.default_rng(3)
    pose = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    pose[:, :3, :] += (0.3 * rng.standard_normal((B, 3, 4))).astype(np.float32)
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 57.7, 57.9, 31.6, 24.2
    fi = ingest.FrameIngest((48, 64), (24, 32), resample="bicubic", high_res_size=(60, 80), include_full_res_depth=True, include_full_depth_K=True)
    out = fi(frames, pose, K, depth_u16=depth)
    shapes = {"image_b3hw": (B, 3, 48, 64), "high_res_color_b3hw": (B, 3, 60, 80), "depth_b1hw": (B, 1, 24, 32), "mask_b1hw": (B, 1, 24, 32),
              "mask_b_b1hw": (B, 1, 24, 32), "full_res_depth_b1hw": (B, 1, 48, 64), "full_res_mask_b1hw": (B, 1, 48, 64),
              "full_res_mask_b_b1hw": (B, 1, 48, 64), "world_T_cam_b44": (B, 4, 4), "cam_T_world_b44": (B, 4, 4),
              "K_full_depth_b44": (B, 4, 4), "invK_full_depth_b44": (B, 4, 4)}
    shapes.update({f"{p}_s{i}_b44": (B, 4, 4) for p in ("K", "invK") for i in range(5)})
    assert sorted(out) == sorted(shapes)
    for k, s in shapes.items():
        assert out[k].is_cuda and tuple(out[k].shape) == s and out[k].dtype == (torch.bool if "mask_b_" in k else torch.float32), k
    assert torch.equal(out["image_b3hw"].cpu(), torch.from_numpy(ref.load_color(golden["ragged_in"][:B], (48, 64), ref.BICUBIC)[0]))
    assert torch.equal(out["high_res_color_b3hw"], ingest.load_color(frames, (60, 80), resample="bicubic"))
    for got, want in zip((out["depth_b1hw"], out["mask_b1hw"], out["mask_b_b1hw"]), ingest.load_depth(depth, (24, 32))):
        assert _same(got, want)
    for got, want in zip((out["full_res_depth_b1hw"], out["full_res_mask_b1hw"], out["full_res_mask_b_b1hw"]), ingest.load_depth(depth)):
        assert _same(got, want)
    assert torch.equal(out["depth_b1hw"].cpu().nan_to_num(-1.0), torch.from_numpy(golden["d_half_depth"]).nan_to_num(-1.0))
    want = ref.intrinsics_pyramid(np.tile(K, (B, 1, 1)), (48, 64), (24, 32), include_full_depth_K=True)
    for k, v in want.items():
        assert torch.equal(out[k].cpu(), torch.from_numpy(v)), k
    assert torch.equal(out["world_T_cam_b44"].cpu(), torch.from_numpy(pose))
    assert torch.equal(out["cam_T_world_b44"].cpu(), torch.from_numpy(np.linalg.inv(pose)))
    # without a depth or the options: the colour image, poses and intrinsics only
    small = ingest.FrameIngest((48, 64), (24, 32))(frames, pose, K)
    assert sorted(small) == sorted(["image_b3hw", "world_T_cam_b44", "cam_T_world_b44"] + [f"{p}_s{i}_b44" for p in ("K", "invK") for i in range(5)])


def test_frame_ingest_image_feeds_the_native_stem(golden):
    """``image_b3hw`` is what the native matching stem takes: its layer1 map equals torch's float64 composition on the same floats."""
    from implicit_depth_amd import ingest
    from test_matching_stem_gpu import _encoder, _ref

    frames = torch.from_numpy(golden["ragged_in"]).cuda()
    out = ingest.FrameIngest((48, 64), (24, 32))(frames, np.tile(np.eye(4, dtype=np.float32), (3, 1, 1)), np.eye(4, dtype=np.float32))
    e = _encoder()
    want = _ref(e, out["image_b3hw"].cpu(), 5)
    got = e.cuda().backbone(out["image_b3hw"])
    torch.cuda.synchronize()
    assert got.shape == (3, 64, 12, 16)
    assert rel_err(got.cpu(), want) < TOL
