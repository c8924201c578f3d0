"""AR compositing on the GPU (csrc/composite.hip, include/idh_composite.h): from the model's outputs to the frame a user sees.

The reference does this on the CPU with numpy / cv2: ``inference/inference.py:117-128`` prepares the asset's depth render for the model,
``:159-162`` turns ``pred_0`` into probabilities and ``inference/composite.py:75-143`` resizes them (or a regressed / lidar depth) to the
camera image, builds the matte and blends.  Here:

``prepare_rendered_depth``  inference.py:117-128 (hole filling + nearest resize), bit-exact
``composite_mask``          composite.py's "mask" method, from ``pred_0`` logits (sigmoid in the kernel) or saved probabilities
``composite_depth``         composite.py's "predicted_depth" / "lidar" methods against the render's depth map or a plane distance
``ARCompositor``            the per-sequence loop of ``composite()``: frame 0 skipped, 45-frame fade-in, mask xor depth

Images are ``uint8`` (B,H,W,3) RGB tensors on the GPU, renders ``uint8`` (B,H,W,4) RGBA.  Dtype contract and resize semantics: DESIGN.md §4.9.
Video encoding, file IO and ``VDRSequence`` are not covered.  There is no CPU fallback."""
from __future__ import annotations

import functools
from typing import Optional, Sequence, Tuple, Union

import torch

from . import _lib

FADE_IN_FRAMES = 45           # composite.py:16
COLOUR = (0.30, 0.9, 0.78)    # composite.py:87-89
MODEL_SIZE = (192, 256)


def _u8(name, t, channels, like=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.IdhError(f"{name} must be a tensor on the MI355X (there is no CPU fallback)")
    if t.dtype != torch.uint8:
        raise _lib.IdhError(f"{name} must be uint8 (got {t.dtype})")
    if t.dim() != 4 or t.shape[-1] != channels or (like is not None and tuple(t.shape[:3]) != tuple(like.shape[:3])):
        raise _lib.IdhError(f"{name} {tuple(t.shape)} must be (B,H,W,{channels})" + ("" if like is None else f" with the image's {tuple(like.shape[:3])}"))
    return t.contiguous()


def _map(name, t, B):
    _lib.require_cuda_f32(t)
    if t.dim() == 3:
        t = t[:, None]
    if t.dim() != 4 or t.shape[1] != 1 or t.shape[0] != B:
        raise _lib.IdhError(f"{name} {tuple(t.shape)} must be ({B},1,h,w)")
    return t.contiguous()


def prepare_rendered_depth(rendered_b1HW: torch.Tensor, size: Tuple[int, int] = MODEL_SIZE) -> torch.Tensor:
    """(B,1,h,w): the asset's depth render (0 = no asset) with its zero pixels filled by the 7x7 maximum, resized with nearest sampling
    to the model's ``size`` (inference.py:117-128)."""
    if not isinstance(rendered_b1HW, torch.Tensor):
        raise _lib.IdhError("prepare_rendered_depth: the render must be a tensor")
    _lib.require_cuda_f32(rendered_b1HW)
    if rendered_b1HW.dim() != 4 or rendered_b1HW.shape[1] != 1:
        raise _lib.IdhError(f"prepare_rendered_depth: render {tuple(rendered_b1HW.shape)} must be (B,1,H,W)")
    x = rendered_b1HW.contiguous()
    B, _, Hr, Wr = x.shape
    h, w = int(size[0]), int(size[1])
    out = torch.empty(B, 1, h, w, device=x.device)
    _lib.check(_lib.lib().idh_prep_rendered_depth_fwd(x.data_ptr(), B, Hr, Wr, h, w, out.data_ptr(), _lib.stream_ptr()), "idh_prep_rendered_depth_fwd")
    return out


@functools.lru_cache(maxsize=256)
def _fade_on_device(values: Tuple[float, ...], device: torch.device) -> torch.Tensor:
    """One float per frame on the device.  Cached: a sequence has 45 distinct fades, so the per-frame loop copies each to the GPU once."""
    return torch.tensor(values, dtype=torch.float32).to(device)


def _composite(image_u8, map_b1hw, mode, *, multiplier=1.0, virtual_depth=None, virtual_rgba=None, colour=COLOUR, fade=None, bgr=False,
               return_matte=False):
    image = _u8("image", image_u8, 3)
    B, H, W, _ = image.shape
    m = _map("occlusion" if mode <= _lib.COMPOSITE_MASK_PROB else "depth", map_b1hw, B)
    keep = [image, m]
    a = _lib.CompositeArgs()
    a.image_bHW3, a.map_b1hw, a.mode = image.data_ptr(), m.data_ptr(), mode
    a.B, a.h, a.w, a.H, a.W = B, m.shape[2], m.shape[3], H, W
    a.sigmoid_multiplier, a.bgr = float(multiplier), int(bool(bgr))
    if virtual_rgba is not None:
        rgba = _u8("virtual_rgba", virtual_rgba, 4, like=image)
        keep.append(rgba)
        a.virtual_rgba_bHW4 = rgba.data_ptr()
    else:
        if colour is None or len(colour) != 3:
            raise _lib.IdhError("a render (virtual_rgba) or a constant colour of three components is needed")
        a.has_colour = 1
        a.colour[0], a.colour[1], a.colour[2] = (float(c) for c in colour)
    if isinstance(virtual_depth, torch.Tensor):
        _lib.require_cuda_f32(virtual_depth)
        if virtual_depth.numel() != B * H * W or virtual_depth.shape[-2:] != (H, W):
            raise _lib.IdhError(f"virtual_depth {tuple(virtual_depth.shape)} must be ({B},{H},{W})")
        vd = virtual_depth.contiguous()
        keep.append(vd)
        a.virtual_depth_bHW = vd.data_ptr()
    elif virtual_depth is not None:
        a.has_plane, a.plane_distance = 1, float(virtual_depth)
    if fade is not None:
        if isinstance(fade, torch.Tensor) and fade.is_cuda:  # already on the device: used as it is, no copy
            f = fade.reshape(-1)
            if f.dtype != torch.float32 or f.numel() != B:
                raise _lib.IdhError(f"a fade tensor must hold one float32 per frame ({B}), got {f.numel()} of {f.dtype}")
            f = f.contiguous()
        else:
            vals = tuple(float(v) for v in torch.as_tensor(fade, dtype=torch.float64).reshape(-1).tolist())
            if len(vals) == 1:
                vals = vals * B
            if len(vals) != B:
                raise _lib.IdhError(f"fade must hold one value per frame ({B}), got {len(vals)}")
            f = _fade_on_device(vals, image.device)
        keep.append(f)
        a.fade_b = f.data_ptr()
    out = torch.empty_like(image)
    matte = torch.empty(B, H, W, device=image.device) if return_matte else None
    a.out_bHW3, a.matte_out_bHW = out.data_ptr(), _lib.ptr(matte)
    _lib.check(_lib.lib().idh_composite_fwd(a, _lib.stream_ptr()), "idh_composite_fwd")
    return (out, matte) if return_matte else out


def composite_mask(image_u8: torch.Tensor, occlusion: torch.Tensor, *, logits: bool = True, multiplier: float = 1.0,
                   virtual_rgba: Optional[torch.Tensor] = None, colour: Sequence[float] = COLOUR, fade=None, bgr: bool = False,
                   return_matte: bool = False):
    """The composited uint8 (B,H,W,3) frame from an occlusion map (B,1,h,w): ``pred_0`` logits (``sigmoid_custom(x, multiplier)`` is applied
    in the kernel) or, with ``logits=False``, probabilities as inference.py saves them.  ``matte = 1 - resize(p) * alpha * fade``
    (composite.py:92-102).  ``virtual_rgba`` uint8 (B,H,W,4) or the constant ``colour``; ``fade`` one float per frame (None: 1.0; floats are cached on the device, a float32 GPU tensor is used as it is);
    ``bgr`` writes cv2.imwrite's channel order; ``return_matte`` also returns the fp32 (B,H,W) matte."""
    mode = _lib.COMPOSITE_MASK_LOGITS if logits else _lib.COMPOSITE_MASK_PROB
    return _composite(image_u8, occlusion, mode, multiplier=multiplier, virtual_rgba=virtual_rgba, colour=colour, fade=fade, bgr=bgr,
                      return_matte=return_matte)


def composite_depth(image_u8: torch.Tensor, depth: torch.Tensor, *, virtual_depth: Union[torch.Tensor, float], soft: bool = True,
                    virtual_rgba: Optional[torch.Tensor] = None, colour: Sequence[float] = COLOUR, fade=None, bgr: bool = False,
                    return_matte: bool = False):
    """The composited frame from a depth map (B,1,h,w) (``depth_pred_s0_b1hw`` or lidar).  ``virtual_depth`` is the render's fp32 (B,H,W)
    depth (valid where > 0, ``matte = 1 - get_mask * valid * fade``, composite.py:120-129) or a float plane distance
    (``matte = 1 - get_mask``, :131-134; no valid pixels, no fade).  ``soft`` selects the 0.2 m band or the hard compare (:19-24)."""
    if virtual_depth is None:
        raise _lib.IdhError("composite_depth needs virtual_depth: the render's depth map or a plane distance")
    mode = _lib.COMPOSITE_DEPTH_SOFT if soft else _lib.COMPOSITE_DEPTH_HARD
    return _composite(image_u8, depth, mode, virtual_depth=virtual_depth, virtual_rgba=virtual_rgba, colour=colour, fade=fade, bgr=bgr,
                      return_matte=return_matte)


class ARCompositor:
    """The per-sequence loop of the reference's ``composite()`` (composite.py:61-143).  ``frame`` returns None for frame 0 (:67-69),
    fades the asset in over the first 45 frames when ``fadein`` (:92-94, :124-126) and picks the method as ``determine_method`` does
    (:27-41): an occlusion mask xor a depth."""

    def __init__(self, fadein: bool = False, soft: bool = True, bgr: bool = False):
        self.fadein, self.soft, self.bgr = bool(fadein), bool(soft), bool(bgr)

    def frame(self, frame_idx: int, image_u8: torch.Tensor, outputs=None, *, mask: Optional[torch.Tensor] = None,
              depth: Optional[torch.Tensor] = None, logits: bool = True, multiplier: float = 1.0, virtual_rgba: Optional[torch.Tensor] = None,
              virtual_depth: Union[torch.Tensor, float, None] = None, colour: Sequence[float] = COLOUR, return_matte: bool = False):
        """``outputs``: the dict of ``fused_forward`` / ``HotPath`` (``pred_0`` logits, or ``depth_pred_s0_b1hw``), or a tensor taken as
        ``pred_0`` logits.  ``mask`` / ``depth`` give an occlusion map (logits or, with ``logits=False``, probabilities) or a depth
        directly.  Exactly one of the two must result."""
        if isinstance(outputs, dict):
            if "pred_0" in outputs:
                mask = outputs["pred_0"] if mask is None else mask
            if "depth_pred_s0_b1hw" in outputs:
                depth = outputs["depth_pred_s0_b1hw"] if depth is None else depth
        elif outputs is not None:
            mask = outputs if mask is None else mask
        if (mask is None) == (depth is None):
            raise _lib.IdhError("ARCompositor.frame: expected either an occlusion mask or a depth, but not both (composite.py:30-34)")
        if frame_idx == 0:
            return None
        fade = frame_idx / FADE_IN_FRAMES if self.fadein and frame_idx < FADE_IN_FRAMES else None
        if mask is not None:
            return composite_mask(image_u8, mask, logits=logits, multiplier=multiplier, virtual_rgba=virtual_rgba, colour=colour, fade=fade,
                                  bgr=self.bgr, return_matte=return_matte)
        return composite_depth(image_u8, depth, virtual_depth=virtual_depth, soft=self.soft, virtual_rgba=virtual_rgba, colour=colour, fade=fade,
                               bgr=self.bgr, return_matte=return_matte)
