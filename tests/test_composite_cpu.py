"""AR compositing without a GPU: the numpy restatement (tests/composite_ref.py) against the reference's own code
(tests/golden/g16_composite.npz, written by tests/golden/gen_golden_composite.py), the host-side argument validation of the two C entry
points, and the Python functions' refusals.

Comparison rule for uint8 frames (g16): probability and depth inputs must match exactly; with logits inputs a pixel the generator marked
ambiguous (a +-2e-6 shift of the resized probability changes a channel) may differ by 1 per channel, every other pixel exactly, and at
most 2 % of a frame may be ambiguous."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import composite_ref as cr
from conftest import load_golden

MAX_AMBIGUOUS = 0.02
PLANE = 2.0


@pytest.fixture(scope="module")
def g16():
    return load_golden("g16_composite")


def golden_case(g16, name):
    """(spec dict, frames uint8 (B,H,W,3), ambiguous bool (B,H,W) or None)"""
    spec = json.loads(str(g16[f"{name}__case"]))
    frames = g16[f"{name}__frames"]
    amb = None
    if f"{name}__ambiguous_bits" in g16:
        n = int(np.prod(frames.shape[:3]))
        amb = np.unpackbits(g16[f"{name}__ambiguous_bits"])[:n].astype(bool).reshape(frames.shape[:3])
    return spec, frames, amb


def fades_of(frames):
    return [i / 45 if i < 45 else 1.0 for i in frames]


def ref_kwargs(case, spec):
    """composite_ref.composite's keywords for a golden case's options (the generator always runs with fadein)."""
    o = spec["opts"]
    kw = dict(virtual_rgba=case["rgba"] if o.get("rgba") else None, fade=fades_of(spec["frames"]), bgr=bool(o.get("bgr")))
    if o["kind"] == "depth":
        kw.update(depth=case["depth"], soft=o["soft"], virtual_depth=case["virtual_depth"] if o.get("rgba") else PLANE)
    elif o["kind"] == "prob":
        kw.update(occlusion=case["prob"], logits=False)
    else:
        kw.update(occlusion=case["logits"], logits=True, multiplier=o.get("multiplier", 1.0))
    return kw


def assert_frames(got, want, amb, what):
    got, want = np.asarray(got).astype(np.int16), np.asarray(want).astype(np.int16)
    assert got.shape == want.shape, what
    diff = np.abs(got - want).max(-1)
    if amb is None:
        assert diff.max() == 0, f"{what}: {int((diff > 0).sum())} pixels differ, must be exact"
        return
    for b in range(amb.shape[0]):
        assert amb[b].mean() <= MAX_AMBIGUOUS, f"{what}[{b}]: {amb[b].mean():.4f} of the frame is ambiguous"
    assert diff[~amb].max(initial=0) == 0, f"{what}: {int((diff[~amb] > 0).sum())} unambiguous pixels differ"
    assert diff[amb].max(initial=0) <= 1, f"{what}: an ambiguous pixel differs by {int(diff[amb].max())}"


CASE_NAMES = ["mask_logits_rgba", "mask_logits_mult_odd_bgr", "mask_logits_colour_same", "mask_logits_rgba_down", "mask_logits_fade_seq",
              "mask_prob_rgba_odd", "mask_prob_rgba_tall", "mask_prob_rgba_same", "mask_prob_colour_down_bgr", "depth_soft_map",
              "depth_hard_map_odd_bgr", "depth_soft_map_same", "depth_soft_map_fade_seq", "depth_soft_plane_odd", "depth_hard_plane_down",
              "depth_soft_plane_same"]


def test_golden_holds_the_cases(g16):
    assert [str(n) for n in g16["case_names"]] == CASE_NAMES


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_reproduces_the_reference_frames(g16, name):
    """The resize of the fixture is torch's CPU ``F.interpolate``; the restatement (and csrc/composite.hip) round it the same way, see
    ``composite_ref.resize_bilinear``."""
    import implicit_depth_amd.synthetic as syn

    spec, frames, amb = golden_case(g16, name)
    B, h, w, H, W, seed = spec["shape"]
    case = syn.composite_case(B, h, w, H, W, seed)
    got, matte = cr.composite(case["image"], **ref_kwargs(case, spec))
    print(f"{name}: ambiguous {0.0 if amb is None else amb.mean():.4f}, differing pixels {int((got != frames).any(-1).sum())}")
    assert matte.dtype == np.float32 and matte.shape == frames.shape[:3]
    if spec["opts"].get("rgba") and spec["opts"]["kind"] != "depth":  # no asset: the camera image, exactly
        rgb = frames[..., ::-1] if spec["opts"].get("bgr") else frames
        none = case["rgba"].numpy()[..., 3] == 0
        assert none.any() and (rgb[none] == case["image"].numpy()[none]).all()
    assert_frames(got, frames, amb, name)


# output (H, W): either side of H + W = 128, with shapes whose pixel count and whose sum disagree about which is "small" (100x30, 20x200,
# 300x4 against 64x64, 63x65), and the sizes of the fixture
RESIZE_SHAPES = [(100, 30), (33, 120), (20, 200), (300, 4), (65, 64), (64, 65), (2, 127), (1, 128), (64, 64), (63, 65), (2, 126), (1, 127),
                 (60, 80), (31, 47), (10, 13)]


@pytest.mark.parametrize("size", RESIZE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_resize_is_torchs_cpu_bilinear(size):
    """``composite_ref.resize_bilinear`` (and with it ``blend4`` of csrc/composite.hip, which the GPU tests hold to it) against
    ``F.interpolate`` on the CPU, bit for bit, for an upscale, an odd-sized and a downscale source, two planes at once."""
    import implicit_depth_amd.synthetic as syn

    H, W = size
    for k, (h, w) in enumerate(((24, 32), (9, 20), (70, 90))):
        m = syn.randn((2, 1, h, w), 31 + k) * 3
        want = torch.nn.functional.interpolate(m, size=(H, W), mode="bilinear", align_corners=False)[:, 0].numpy()
        got = cr.resize_bilinear(m[:, 0], H, W)
        assert got.dtype == np.float32 and np.array_equal(got, want), f"{(h, w)} -> {size}: {int((got != want).sum())} of {want.size} differ"


def test_restatement_reproduces_the_reference_prepared_depth(g16):
    import implicit_depth_amd.synthetic as syn

    for name in [str(n) for n in g16["prep_names"]]:
        B, Hr, Wr, h, w, seed = json.loads(str(g16[f"{name}__case"]))["shape"]
        render = syn.composite_case(B, h, w, 8, 8, seed, render_hw=(Hr, Wr))["render"]
        assert tuple(render.shape) == (B, 1, Hr, Wr)
        want = g16[f"{name}__prepared"]
        got = cr.prepare_rendered_depth(render, (h, w))
        assert got.dtype == np.float32 and np.array_equal(got, want), name
    # the large hole's centre stays 0 after the fill, the isolated holes do not
    render = syn.composite_case(1, 24, 32, 8, 8, 23, render_hw=(24, 32))["render"]
    out = cr.prepare_rendered_depth(render, (24, 32))
    assert out[0, 0, 12, 16] == 0 and (out == 0).sum() < (render.numpy() == 0).sum()


def test_composite_case_is_what_the_tests_need():
    import implicit_depth_amd.synthetic as syn

    c = syn.composite_case(2, 9, 20, 31, 47, 2, render_hw=(37, 53))
    a = c["rgba"][..., 3]
    assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any()
    assert c["image"].dtype == torch.uint8 and tuple(c["image"].shape) == (2, 31, 47, 3)
    assert c["logits"].max() == 40 and c["logits"].min() == -40
    assert ((c["virtual_depth"] == 0) == (a == 0)).all()
    r = c["render"][0, 0]
    assert (r[0] == 0).any() and (r[-1] == 0).any() and (r[:, 0] == 0).any() and (r[:, -1] == 0).any()
    assert r[0, 0] == 0 and r[0, -1] == 0 and r[-1, 0] == 0 and r[-1, -1] == 0
    again = syn.composite_case(2, 9, 20, 31, 47, 2, render_hw=(37, 53))
    assert all(torch.equal(c[k], again[k]) for k in c)


# ---- C entry points: validation happens before any launch ---------------------------------------------------------------------
def _args(**over):
    from implicit_depth_amd import _lib

    a = _lib.CompositeArgs()
    a.image_bHW3, a.virtual_rgba_bHW4, a.map_b1hw, a.out_bHW3 = 0x1000, 0x2000, 0x3000, 0x4000
    a.mode, a.B, a.h, a.w, a.H, a.W = _lib.COMPOSITE_MASK_LOGITS, 1, 4, 4, 8, 8
    a.sigmoid_multiplier = 1.0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_composite_entry_validates_before_launching():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -2
    assert L.idh_version() == 112
    assert L.idh_sizeof_composite_args() == C.sizeof(_lib.CompositeArgs) == _lib.CompositeArgs().struct_size
    call = lambda a: L.idh_composite_fwd(C.byref(a), None)
    assert L.idh_composite_fwd(None, None) == EINVAL
    assert call(_args(B=0)) == 0  # a well-formed request for no frames: nothing is launched
    # struct_size: a caller built against a shorter struct is refused
    assert call(_args(B=0, struct_size=C.sizeof(_lib.CompositeArgs) - 8)) == EINVAL
    assert call(_args(B=0, struct_size=0)) == EINVAL
    assert call(_args(B=0, struct_size=C.sizeof(_lib.CompositeArgs) + 8)) == 0
    for k in ("image_bHW3", "map_b1hw", "out_bHW3"):
        assert call(_args(**{k: None})) == EINVAL, k
    for k in ("h", "w", "H", "W"):
        assert call(_args(**{k: 0})) == EINVAL and call(_args(**{k: -3})) == EINVAL, k
    assert call(_args(B=-1)) == EINVAL
    assert call(_args(mode=4)) == EINVAL and call(_args(mode=-1)) == EINVAL
    # missing inputs: neither a render nor a constant colour; both
    assert call(_args(virtual_rgba_bHW4=None)) == EINVAL
    assert call(_args(has_colour=1)) == EINVAL
    assert call(_args(B=0, virtual_rgba_bHW4=None, has_colour=1)) == 0
    # depth modes need the render's depth map or a plane distance, and not both; mask modes take neither
    for mode in (_lib.COMPOSITE_DEPTH_SOFT, _lib.COMPOSITE_DEPTH_HARD):
        assert call(_args(mode=mode)) == EINVAL
        assert call(_args(mode=mode, virtual_depth_bHW=0x5000, has_plane=1, plane_distance=2.0)) == EINVAL
        assert call(_args(B=0, mode=mode, virtual_depth_bHW=0x5000)) == 0
        assert call(_args(B=0, mode=mode, has_plane=1, plane_distance=2.0)) == 0
    for mode in (_lib.COMPOSITE_MASK_LOGITS, _lib.COMPOSITE_MASK_PROB):
        assert call(_args(mode=mode, virtual_depth_bHW=0x5000)) == EINVAL
        assert call(_args(mode=mode, has_plane=1)) == EINVAL
    # 32-bit pixel indices
    assert call(_args(B=2, H=32768, W=32768)) == EUNSUPPORTED


def test_prep_entry_validates_before_launching():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    f = L.idh_prep_rendered_depth_fwd
    assert f(None, 1, 8, 8, 4, 4, 0x2000, None) == -1
    assert f(0x1000, 1, 8, 8, 4, 4, None, None) == -1
    for bad in ((-1, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, 0, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, -2), (1, 65536, 65536, 4, 4)):
        assert f(0x1000, *bad, 0x2000, None) == -1, bad
    assert f(0x1000, 70000, 8, 8, 4, 4, 0x2000, None) == -2
    assert f(0x1000, 0, 8, 8, 4, 4, 0x2000, None) == 0


# ---- Python surface -------------------------------------------------------------------------------------------------------------
def test_python_functions_refuse_what_the_kernels_cannot_take():
    from implicit_depth_amd import _lib
    from implicit_depth_amd import compositing as cp

    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    occ = torch.zeros(1, 1, 4, 4)
    with pytest.raises(_lib.IdhError):  # CPU tensors
        cp.composite_mask(img, occ)
    with pytest.raises(_lib.IdhError):
        cp.composite_depth(img, occ, virtual_depth=2.0)
    with pytest.raises(_lib.IdhError):
        cp.prepare_rendered_depth(torch.zeros(1, 1, 8, 8))
    with pytest.raises(_lib.IdhError):  # the image must be uint8
        cp.composite_mask(img.float(), occ)
    with pytest.raises(_lib.IdhError):
        cp.composite_depth(img, occ, virtual_depth=None)
    comp = cp.ARCompositor(fadein=True)
    with pytest.raises(_lib.IdhError):  # a mask and a depth together (determine_method)
        comp.frame(3, img, mask=occ, depth=occ, virtual_depth=2.0)
    with pytest.raises(_lib.IdhError):
        comp.frame(3, img, {"pred_0": occ, "depth_pred_s0_b1hw": occ}, virtual_depth=2.0)
    with pytest.raises(_lib.IdhError):  # neither
        comp.frame(3, img)
    assert cp.FADE_IN_FRAMES == 45 and cp.COLOUR == (0.30, 0.9, 0.78)
