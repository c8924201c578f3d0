"""AR compositing on the GPU (csrc/composite.hip through implicit_depth_amd.compositing): against the reference's own code
(tests/golden/g16_composite.npz) and against the numpy restatement (tests/composite_ref.py) on further seeds.

Rule for uint8 frames: probability and depth inputs exactly; logits inputs exactly outside the pixels a +-2e-6 shift of the resized
probability changes, within 1 per channel inside them, at most 2 % of a frame ambiguous.  Mattes in fp32: exact for probability and depth
inputs, <= 2e-6 for logits.  Prepared depths bit-exact.
"""
import json

import numpy as np
import pytest
import torch

import composite_ref as cr
from test_composite_cpu import CASE_NAMES, MAX_AMBIGUOUS, PLANE, assert_frames, fades_of, g16, golden_case, ref_kwargs  # noqa: F401

pytestmark = pytest.mark.gpu

MARGIN = 2e-6
SHAPES = [(24, 32, 60, 80), (9, 20, 31, 47), (12, 16, 12, 16), (24, 32, 10, 13), (24, 32, 100, 30)]  # the last: few pixels, H + W > 128
# the logits + RGBA inputs of the two tiny shapes mark 4 of 192 and 3 of 130 pixels at their first seed, above 2 %: these seeds do not
SEEDS = {((12, 16, 12, 16), 0): 202, ((24, 32, 10, 13), 0): 203}


def gpu(case):
    return {k: v.cuda() for k, v in case.items()}


def run(cp, c, kw, return_matte=False):
    """implicit_depth_amd.compositing with composite_ref.composite's keywords."""
    kw = dict(kw)
    common = dict(virtual_rgba=None if kw.get("virtual_rgba") is None else c["rgba"], fade=kw.get("fade"), bgr=kw.get("bgr", False), return_matte=return_matte)
    if "colour" in kw:
        common["colour"] = kw["colour"]
    if kw.get("depth") is not None:
        vd = kw["virtual_depth"]
        return cp.composite_depth(c["image"], c["depth"], virtual_depth=vd if isinstance(vd, float) else c["virtual_depth"], soft=kw["soft"], **common)
    return cp.composite_mask(c["image"], c["logits"] if kw["logits"] else c["prob"], logits=kw["logits"], multiplier=kw.get("multiplier", 1.0), **common)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_frames_against_the_reference(g16, name):
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import compositing as cp

    spec, frames, amb = golden_case(g16, name)
    B, h, w, H, W, seed = spec["shape"]
    case = syn.composite_case(B, h, w, H, W, seed)
    got = run(cp, gpu(case), ref_kwargs(case, spec))
    assert got.dtype == torch.uint8 and tuple(got.shape) == frames.shape
    got = got.cpu().numpy()
    print(f"{name}: differing pixels {int((got != frames).any(-1).sum())}")
    assert_frames(got, frames, amb, name)


def _ambiguous(case, kw):
    base, _ = cr.composite(case["image"], **kw)
    a = np.zeros(base.shape[:3], bool)
    for s in (MARGIN, -MARGIN):
        a |= (cr.composite(case["image"], prob_shift=s, **kw)[0] != base).any(-1)
    return a


MODES = [
    dict(kind="logits", rgba=True), dict(kind="logits", multiplier=2.5, rgba=False, bgr=True), dict(kind="prob", rgba=True, bgr=True),
    dict(kind="prob", rgba=False), dict(kind="depth", soft=True, rgba=True), dict(kind="depth", soft=False, rgba=True, bgr=True),
    dict(kind="depth", soft=True, rgba=False, plane=True), dict(kind="depth", soft=False, rgba=True, plane=True),
    dict(kind="depth", soft=True, rgba=False, bgr=True), dict(kind="depth", soft=False, rgba=False, plane=True, bgr=True),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
@pytest.mark.parametrize("mode", MODES, ids=lambda m: "-".join(f"{k}={v}" for k, v in m.items()))
def test_frames_and_mattes_against_the_restatement(shape, mode):
    """Further seeds, B = 2 with fades 1.0 and 7/45, every mode crossed with every shape, frame and matte from one call."""
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import compositing as cp

    h, w, H, W = shape
    seed = SEEDS.get((shape, MODES.index(mode)), 100 + SHAPES.index(shape) + 10 * MODES.index(mode))
    case, kw, amb = _inputs(syn, shape, mode, seed)  # assert_frames holds amb (restatement only, nothing from the GPU) to the 2 % bound
    want, want_matte = cr.composite(case["image"], **kw)
    got, matte = run(cp, gpu(case), kw, return_matte=True)
    matte = matte.cpu().numpy()
    err = float(np.abs(matte.astype(np.float64) - want_matte).max())
    print(f"seed {seed}: matte max error {err:.3g}, differing pixels {int((got.cpu().numpy() != want).any(-1).sum())}")
    if mode["kind"] == "logits":
        assert err <= MARGIN
    else:
        assert np.array_equal(matte, want_matte)
    assert_frames(got.cpu().numpy(), want, amb, str(mode))
    again = run(cp, gpu(case), kw)  # without the matte output: the same frame
    assert torch.equal(again, got)


def _inputs(syn, shape, mode, seed):
    h, w, H, W = shape
    case = syn.composite_case(2, h, w, H, W, seed)
    kw = dict(virtual_rgba=case["rgba"] if mode["rgba"] else None, fade=[1.0, 7 / 45], bgr=bool(mode.get("bgr")))
    if not mode["rgba"]:
        kw["colour"] = (0.30, 0.9, 0.78) if mode.get("bgr") else (0.1, 0.55, 1.0)
    if mode["kind"] == "depth":
        kw.update(depth=case["depth"], soft=mode["soft"], virtual_depth=PLANE if mode.get("plane") else case["virtual_depth"])
    else:
        kw.update(occlusion=case["logits"] if mode["kind"] == "logits" else case["prob"], logits=mode["kind"] == "logits", multiplier=mode.get("multiplier", 1.0))
    return case, kw, _ambiguous(case, kw) if mode["kind"] == "logits" else None


def test_unaligned_views_take_the_per_pixel_path():
    """A frame tensor that starts one byte into its allocation: same result as the aligned one."""
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import compositing as cp

    case = gpu(syn.composite_case(2, 9, 20, 31, 47, 77))
    want = cp.composite_mask(case["image"], case["prob"], logits=False, virtual_rgba=case["rgba"])
    buf = torch.empty(case["image"].numel() + 1, dtype=torch.uint8, device="cuda")
    img = buf[1:].view_as(case["image"]).copy_(case["image"])
    assert img.data_ptr() % 4 == 1
    assert torch.equal(cp.composite_mask(img, case["prob"], logits=False, virtual_rgba=case["rgba"]), want)


def test_prepared_depth_is_bit_exact(g16):
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import compositing as cp

    for name in [str(n) for n in g16["prep_names"]]:
        B, Hr, Wr, h, w, seed = json.loads(str(g16[f"{name}__case"]))["shape"]
        render = syn.composite_case(B, h, w, 8, 8, seed, render_hw=(Hr, Wr))["render"]
        got = cp.prepare_rendered_depth(render.cuda(), (h, w)).cpu().numpy()
        assert np.array_equal(got, g16[f"{name}__prepared"]), name
        render2 = syn.composite_case(B, h, w, 8, 8, seed + 50, render_hw=(Hr, Wr))["render"]
        assert np.array_equal(cp.prepare_rendered_depth(render2.cuda(), (h, w)).cpu().numpy(), cr.prepare_rendered_depth(render2, (h, w))), name


def test_compositor_loop(g16):
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import compositing as cp

    comp = cp.ARCompositor(fadein=True)
    for name, key in (("mask_logits_fade_seq", "pred_0"), ("depth_soft_map_fade_seq", "depth_pred_s0_b1hw")):
        spec, frames, amb = golden_case(g16, name)
        B, h, w, H, W, seed = spec["shape"]
        assert spec["frames"] == [1, 7, 45]
        c = gpu(syn.composite_case(B, h, w, H, W, seed))
        src = c["logits"] if key == "pred_0" else c["depth"]
        extra = {} if key == "pred_0" else dict(virtual_depth=c["virtual_depth"][:1])
        assert comp.frame(0, c["image"][:1], {key: src[:1]}, virtual_rgba=c["rgba"][:1], **extra) is None
        for b, idx in enumerate(spec["frames"]):
            extra = {} if key == "pred_0" else dict(virtual_depth=c["virtual_depth"][b: b + 1])
            out = comp.frame(idx, c["image"][b: b + 1], {key: src[b: b + 1]}, virtual_rgba=c["rgba"][b: b + 1], **extra)
            assert_frames(out.cpu().numpy(), frames[b: b + 1], None if amb is None else amb[b: b + 1], f"{name} frame {idx}")
    # a bare tensor is taken as pred_0
    c = gpu(syn.composite_case(1, 9, 20, 31, 47, 5))
    assert torch.equal(comp.frame(50, c["image"], c["logits"], virtual_rgba=c["rgba"]), cp.composite_mask(c["image"], c["logits"], virtual_rgba=c["rgba"]))


def test_render_to_frame_smoke():
    """MeshDepthRasterizer render -> prepare_rendered_depth -> composite_mask at model size."""
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import compositing as cp
    from implicit_depth_amd.raster import MeshDepthRasterizer

    verts, faces, cam_T_world, K = syn.raster_scene(96, 128, seed=3)[:4]
    r = MeshDepthRasterizer(96, 128)
    render = r.render_depth(cam_T_world.cuda().float(), K.cuda().float(), mesh=(verts.cuda().float(), faces.cuda())).clamp_min(0)  # -1 = nothing hit
    prepared = cp.prepare_rendered_depth(render, (48, 64))
    assert tuple(prepared.shape) == (render.shape[0], 1, 48, 64) and prepared.dtype == torch.float32
    B = render.shape[0]
    case = gpu(syn.composite_case(B, 48, 64, 240, 320, 9))
    out = cp.composite_mask(case["image"], syn.randn((B, 1, 48, 64), 4).cuda(), virtual_rgba=case["rgba"])
    assert tuple(out.shape) == (B, 240, 320, 3) and out.dtype == torch.uint8
    none = case["rgba"][..., 3] == 0
    assert none.any() and torch.equal(out[none], case["image"][none])
