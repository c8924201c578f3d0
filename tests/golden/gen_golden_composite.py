#!/usr/bin/env python
"""Generate tests/golden/g16_composite.npz: the reference's AR compositing (inference/composite.py:75-143) and asset-depth
preparation (inference/inference.py:117-128) replayed statement by statement on CPU, with the reference's own get_mask,
determine_method, DEPTH_ALPHA_BAND_SIZE, FADE_IN_FRAMES (inference/composite.py) and sigmoid_custom (modules/layers.py).

Runs only where the reference checkout is (see gen_golden.py); inputs come from ``implicit_depth_amd.synthetic.composite_case``
(seeded, basic arithmetic), so the fixture holds only outputs: the uint8 frames, the packed ambiguity bits of the logits cases and the
prepared depths.

NOT CHECKED: cv2 and torchvision are not installed where this runs.  A stand-in ``cv2`` module lets ``inference.composite`` import;
where the reference calls ``cv2.resize(..., INTER_LINEAR)`` the replay calls ``F.interpolate(mode="bilinear", align_corners=False)``,
and where it calls torchvision's ``resize(NEAREST)`` the replay calls ``F.interpolate(mode="nearest")`` (what torchvision's tensor path
calls).  cv2's INTER_LINEAR samples at the same half-pixel positions with replicated borders and does not antialias; that its float32
rounding equals torch's has not been measured by anyone.  The fixture therefore pins the torch arithmetic, not cv2's.

Logits cases: the device's expf may differ from the host's by a few ulp, so the replay is run twice more with the resized probability
shifted by +2e-6 and -2e-6 (the margin g14 uses for the same interpolated sigmoid); a pixel either shift changes in any channel is
*ambiguous* and may differ by 1 per channel.  At most 2 % of a frame may be ambiguous (asserted here and in the tests).

    python tests/golden/gen_golden_composite.py
"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch
import torch.nn.functional as F

from gen_golden import import_reference, save  # noqa: E402  (also puts the repository root on sys.path)

MARGIN = 2e-6
MAX_AMBIGUOUS = 0.02
PLANE = 2.0  # composite()'s virtual_depth (composite.py:211)

# name, (B, h, w, H, W, seed), frame index per frame, options.  Frame 45 is the first unfaded one; 7 fades by 7 / 45.  The frames are noise
# and do not compress, so the large shapes hold one frame and the B = 2 cases (a lane's four pixels straddling two frames, one fade per
# frame) sit on the small ones.  Output 100x30 has fewer pixels than 60x80 but H + W > 128: with 60x80 (also above) and 31x47 / 10x13
# (below) it pins which of torch's two CPU resize kernels made a frame (composite_ref.resize_bilinear).
CASES = [
    ("mask_logits_rgba", (1, 24, 32, 60, 80, 1), (7,), dict(kind="logits", rgba=True)),
    ("mask_logits_mult_odd_bgr", (2, 9, 20, 31, 47, 2), (45, 7), dict(kind="logits", multiplier=2.5, rgba=True, bgr=True)),
    ("mask_logits_colour_same", (2, 12, 16, 12, 16, 3), (45, 7), dict(kind="logits")),
    ("mask_logits_rgba_down", (2, 24, 32, 10, 13, 4), (45, 7), dict(kind="logits", rgba=True)),
    ("mask_logits_fade_seq", (3, 24, 32, 10, 13, 5), (1, 7, 45), dict(kind="logits", rgba=True)),
    ("mask_prob_rgba_odd", (1, 9, 20, 31, 47, 6), (7,), dict(kind="prob", rgba=True)),
    ("mask_prob_rgba_tall", (1, 24, 32, 100, 30, 7), (7,), dict(kind="prob", rgba=True)),  # the other kernel's rounding moves 3 of its pixels
    ("mask_prob_rgba_same", (2, 12, 16, 12, 16, 8), (45, 7), dict(kind="prob", rgba=True)),
    ("mask_prob_colour_down_bgr", (2, 24, 32, 10, 13, 9), (45, 7), dict(kind="prob", bgr=True)),
    ("depth_soft_map", (1, 24, 32, 60, 80, 10), (45,), dict(kind="depth", soft=True, rgba=True)),
    ("depth_hard_map_odd_bgr", (2, 9, 20, 31, 47, 11), (45, 7), dict(kind="depth", soft=False, rgba=True, bgr=True)),
    ("depth_soft_map_same", (2, 12, 16, 12, 16, 12), (45, 7), dict(kind="depth", soft=True, rgba=True)),
    ("depth_soft_map_fade_seq", (3, 24, 32, 10, 13, 13), (1, 7, 45), dict(kind="depth", soft=True, rgba=True)),
    ("depth_soft_plane_odd", (1, 9, 20, 31, 47, 14), (45,), dict(kind="depth", soft=True)),
    ("depth_hard_plane_down", (2, 24, 32, 10, 13, 15), (45, 7), dict(kind="depth", soft=False)),
    ("depth_soft_plane_same", (2, 12, 16, 12, 16, 16), (45, 7), dict(kind="depth", soft=True)),
]
# name, (B, Hr, Wr, h, w, seed)
PREP_CASES = [("prep_50x70", (2, 50, 70, 24, 32, 21)), ("prep_odd", (2, 37, 53, 9, 20, 22)), ("prep_same", (2, 24, 32, 24, 32, 23))]


def import_composite():
    """inference/composite.py with stand-ins for the modules it (and vdr_sequence.py) imports at the top and that are absent here."""
    import_reference()
    for name in ("cv2", "tqdm", "PIL", "PIL.Image", "scipy", "scipy.spatial", "scipy.spatial.transform"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    cv2 = sys.modules["cv2"]
    if not hasattr(cv2, "resize"):  # the stand-in: never called, the replay resizes with F.interpolate (module docstring)
        cv2.INTER_LINEAR = 1
        sys.modules["tqdm"].__dict__.setdefault("tqdm", lambda x, *a, **k: x)
        sys.modules["PIL"].__dict__.setdefault("Image", sys.modules["PIL.Image"])
        sys.modules["scipy.spatial.transform"].__dict__.setdefault("Rotation", None)
    from inference import composite as rc

    return rc


def _resize_linear(a_hw: np.ndarray, w: int, h: int) -> np.ndarray:
    """In place of cv2.resize(a, (w, h), INTER_LINEAR) — see the module docstring."""
    return F.interpolate(torch.from_numpy(np.ascontiguousarray(a_hw))[None, None], size=(h, w), mode="bilinear", align_corners=False)[0, 0].numpy()


def replay_frame(rc, frame_idx, image_u8, *, fadein, use_depth_banding, raw_matte=None, depth=None, rgba_u8=None, virtual_depthmap=None,
                 virtual_depth=None, shift=0.0):
    """composite.py:75-143 for one frame.  ``raw_matte`` is what :98-100 loads, ``depth`` what :114 yields, ``rgba_u8`` what Image.open
    gives at :82, ``virtual_depthmap`` the .npy of :122.  ``rgba_u8 is None`` stands for ``rendered_rgb_dir is None``.  ``shift`` is added
    to the resized matte (ambiguity margin).  Returns the array handed to cv2.imwrite before its [:, :, ::-1] (RGB)."""
    method = rc.determine_method(predicted_masks_dir=None if raw_matte is None else "masks", predicted_depths_dir=None if depth is None else "depths")
    h, w = image_u8.shape[:2]
    im = image_u8 / 255.0
    if rgba_u8 is not None:
        virtual_rgba = np.array(rgba_u8).astype(np.float32) / 255.0
        virtual_rgb = virtual_rgba[:, :, :3]
        valid_virtual_pixels = virtual_rgba[:, :, 3]
    else:
        virtual_rgb = np.zeros((h, w, 3))
        virtual_rgb[:, :, 0] = 0.30
        virtual_rgb[:, :, 1] = 0.9
        virtual_rgb[:, :, 2] = 0.78
        valid_virtual_pixels = np.ones_like(virtual_rgb[:, :, 0])
    if fadein and frame_idx < rc.FADE_IN_FRAMES:
        fade_amount = frame_idx / rc.FADE_IN_FRAMES
        valid_virtual_pixels *= fade_amount
    if method == "mask":
        matte = _resize_linear(raw_matte, w, h)
        if shift:
            matte = matte + np.float32(shift)
        matte = 1.0 - matte * valid_virtual_pixels.astype(np.float32)
    else:
        assert method == "predicted_depth"
        if depth.shape != (h, w):
            depth = _resize_linear(depth, w, h)
        if rgba_u8 is not None:
            valid_virtual_pixels = (virtual_depthmap > 0).astype(np.float32)
            if fadein and frame_idx < rc.FADE_IN_FRAMES:
                fade_amount = frame_idx / rc.FADE_IN_FRAMES
                valid_virtual_pixels *= fade_amount
            matte = rc.get_mask(predicted=depth, virtual=virtual_depthmap, soft=use_depth_banding)
            matte = 1.0 - matte * valid_virtual_pixels
        else:
            virtual_depthmap = np.ones((h, w)) * virtual_depth
            matte = 1.0 - rc.get_mask(predicted=depth, virtual=virtual_depthmap, soft=use_depth_banding)
    matte = matte[:, :, None].astype(np.float32)
    composited = matte * im + (1 - matte) * virtual_rgb
    return (composited * 255.0).astype(np.uint8)


def replay_prep(rendered_depth: np.ndarray, h: int, w: int) -> np.ndarray:
    """inference.py:117-128 for one frame; torchvision's resize(NEAREST) on a tensor is F.interpolate(mode="nearest")."""
    rendered_depth_bchw = torch.Tensor(rendered_depth)[None, None, ...]
    rendered_depth_bchw_padded = F.max_pool2d(rendered_depth_bchw, 7, 1, 3).clone()
    rendered_depth_bchw[rendered_depth_bchw == 0] = rendered_depth_bchw_padded[rendered_depth_bchw == 0]
    return F.interpolate(rendered_depth_bchw, size=(h, w), mode="nearest")[0, 0].numpy()


def main():
    rc = import_composite()
    import implicit_depth_amd.synthetic as syn
    from modules.layers import sigmoid_custom

    assert rc.DEPTH_ALPHA_BAND_SIZE == 0.2 and rc.FADE_IN_FRAMES == 45
    out = {"case_names": np.array([c[0] for c in CASES]), "prep_names": np.array([c[0] for c in PREP_CASES])}
    for name, shape, frames, opts in CASES:
        B, h, w, H, W, seed = shape
        case = syn.composite_case(B, h, w, H, W, seed)
        out[f"{name}__case"] = np.array(json.dumps(dict(shape=shape, frames=frames, opts=opts)))
        kind = opts["kind"]
        res, amb = [], []
        for b in range(B):
            kw = dict(fadein=True, use_depth_banding=opts.get("soft", True), rgba_u8=case["rgba"][b].numpy() if opts.get("rgba") else None)
            if kind == "depth":
                kw.update(depth=case["depth"][b, 0].numpy(), virtual_depthmap=case["virtual_depth"][b].numpy(), virtual_depth=PLANE)
            elif kind == "prob":
                kw.update(raw_matte=case["prob"][b, 0].numpy())
            else:  # inference.py:159-162
                pred_bdhw = sigmoid_custom(case["logits"][b: b + 1], multiplier=opts.get("multiplier", 1.0))
                kw.update(raw_matte=pred_bdhw.squeeze(0).detach().cpu().numpy().astype(np.float32)[0])
            im = case["image"][b].numpy()
            f0 = replay_frame(rc, frames[b], im, **kw)
            if kind == "logits":
                a = np.zeros(f0.shape[:2], bool)
                for s in (MARGIN, -MARGIN):
                    a |= (replay_frame(rc, frames[b], im, shift=s, **kw) != f0).any(-1)
                assert a.mean() <= MAX_AMBIGUOUS, (name, b, a.mean())
                amb.append(a)
            res.append(f0[:, :, ::-1] if opts.get("bgr") else f0)  # (:142)
        out[f"{name}__frames"] = np.stack(res)
        msg = ""
        if amb:
            out[f"{name}__ambiguous_bits"] = np.packbits(np.stack(amb).ravel())
            msg = f", ambiguous {100 * np.stack(amb).mean():.2f} % of pixels"
        print(f"G16 {name}: frames {out[f'{name}__frames'].shape}{msg}")
    for name, (B, Hr, Wr, h, w, seed) in PREP_CASES:
        render = syn.composite_case(B, h, w, 8, 8, seed, render_hw=(Hr, Wr))["render"]
        before = render.clone()
        out[f"{name}__case"] = np.array(json.dumps(dict(shape=(B, Hr, Wr, h, w, seed))))
        out[f"{name}__prepared"] = np.stack([replay_prep(render[b, 0].numpy().copy(), h, w) for b in range(B)])[:, None]
        assert torch.equal(render, before)
        print(f"G16 {name}: {(render == 0).float().mean():.3f} holes in, {(out[f'{name}__prepared'] == 0).mean():.3f} out")
    save("g16_composite", **out)


if __name__ == "__main__":
    main()
