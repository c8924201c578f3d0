"""Frame ingest on the GPU (csrc/ingest.hip, include/idh_ingest.h): from a camera's uint8 frame to the tensors the model reads.

The reference does this per frame in its dataset code on the CPU with Pillow and torchvision (datasets/generic_mvs_dataset.py:560-634,
utils/generic_utils.py:149-214, datasets/scannet_dataset.py:436-561).  Here:

``load_color``          ``Image.resize`` (BILINEAR / BICUBIC, antialiased) + ``to_tensor`` + ImageNet normalisation, bit-exact
``load_depth``          NEAREST resize of a uint16 depth, ``* value_scale``, validity masks, NaN where invalid, bit-exact
``intrinsics_pyramid``  ``load_intrinsics``' float32 host maths: K at the depth resolution, five levels, inverses
``FrameIngest``         all of it for a batch of frames: the ``cur_data`` / ``src_data`` dictionary with the reference's key names

Frames are ``uint8`` (B,H,W,3) RGB tensors on the GPU, the convention of ``compositing.py``; depths ``uint16`` (B,H,W).  Nothing is
cropped: ``read_image_file`` calls ``crop_image_to_target_ratio`` and drops its result (generic_utils.py:195-196), so the reference never
crops either.  A source more than 8 times the target in either dimension is refused.  File IO, PNG decoding, tuple selection and
training augmentation (``color_transform``, flip) are not covered.  Algorithm and dtype contract: DESIGN.md §4.10.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import functools
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib

FILTERS = {"bilinear": _lib.RESIZE_BILINEAR, "bicubic": _lib.RESIZE_BICUBIC}


def _size(name, size) -> Tuple[int, int]:
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise _lib.IdhError(f"{name} must be (height, width), got {size!r}") from None
    if h < 1 or w < 1:
        raise _lib.IdhError(f"{name} must be positive, got {size!r}")
    return h, w


def _filter(resample) -> int:
    if resample not in FILTERS:
        raise _lib.IdhError(f"resample must be one of {sorted(FILTERS)}, got {resample!r}")
    return FILTERS[resample]


def resize_coeffs(n_in: int, n_out: int, resample: str) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's coefficients of one dimension, on the host: ``bounds`` (n_out,2) int32 (first source index, tap count) and ``taps``
    (n_out,ksize) int32 in 22-bit fixed point (idh_resize_coeffs_pack; needs no GPU)."""
    L, filt = _lib.lib(), _filter(resample)
    nb, nt = C.c_int64(), C.c_int64()
    _lib.check(L.idh_resize_coeffs_sizes(int(n_in), int(n_out), filt, C.byref(nb), C.byref(nt)), "idh_resize_coeffs_sizes")
    bounds, taps = np.empty(nb.value, np.int32), np.empty(nt.value, np.int32)
    _lib.check(L.idh_resize_coeffs_pack(int(n_in), int(n_out), filt, bounds.ctypes.data, taps.ctypes.data), "idh_resize_coeffs_pack")
    return bounds.reshape(n_out, 2), taps.reshape(n_out, -1)


@functools.lru_cache(maxsize=64)
def _coeffs_on_device(n_in: int, n_out: int, resample: str, device: torch.device):
    """The two tables of one dimension on the device.  Cached: a stream of frames has one source and one target size."""
    bounds, taps = resize_coeffs(n_in, n_out, resample)
    return torch.from_numpy(bounds).to(device), torch.from_numpy(taps).to(device)


def load_color(frames_u8: torch.Tensor, size: Tuple[int, int], resample: str = "bilinear", normalize: bool = True, return_u8: bool = False):
    """(B,3,h,w) float32 ``image_b3hw`` of uint8 (B,H,W,3) RGB frames: ``img.resize((w, h), resample)``, ``to_tensor`` and, with
    ``normalize``, ``imagenet_normalize`` (generic_utils.py:210-212, :149-152), equal to the reference's floats bit for bit.  Frames that
    already have ``size`` are not resized (:202).  ``return_u8`` also returns Pillow's resized bytes, uint8 (B,h,w,3)."""
    t = frames_u8
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.IdhError("frames must be a tensor on the MI355X (there is no CPU fallback)")
    if t.dtype != torch.uint8:
        raise _lib.IdhError(f"frames must be uint8 (got {t.dtype})")
    if t.dim() != 4 or t.shape[-1] != 3 or t.shape[1] < 1 or t.shape[2] < 1:
        raise _lib.IdhError(f"frames {tuple(t.shape)} must be (B,H,W,3)")
    h, w = _size("size", size)
    filt = _filter(resample)
    t = t.contiguous()
    B, Hs, Ws, _ = t.shape
    if Hs > _lib.INGEST_MAX_RATIO * h or Ws > _lib.INGEST_MAX_RATIO * w:
        raise _lib.IdhError(f"frames of {Hs}x{Ws} are more than {_lib.INGEST_MAX_RATIO} times the target {h}x{w}: not covered by the ingest kernel")
    a = _lib.IngestColorArgs()
    keep = []
    if Ws != w:
        xb, xt = _coeffs_on_device(Ws, w, resample, t.device)
        keep += [xb, xt]
        a.x_bounds, a.x_taps = xb.data_ptr(), xt.data_ptr()
    if Hs != h:
        yb, yt = _coeffs_on_device(Hs, h, resample, t.device)
        keep += [yb, yt]
        a.y_bounds, a.y_taps = yb.data_ptr(), yt.data_ptr()
    image = torch.empty(B, 3, h, w, device=t.device)
    u8 = torch.empty(B, h, w, 3, dtype=torch.uint8, device=t.device) if return_u8 else None
    a.frames_bHW3, a.image_b3hw, a.resized_bhw3 = t.data_ptr(), image.data_ptr(), _lib.ptr(u8)
    a.filter, a.normalize = filt, int(bool(normalize))
    a.B, a.Hs, a.Ws, a.h, a.w = B, Hs, Ws, h, w
    _lib.check(_lib.lib().idh_ingest_color_fwd(a, _lib.stream_ptr()), "idh_ingest_color_fwd")
    return (image, u8) if return_u8 else image


def _depth(depth_u16, size, full, value_scale, min_valid, max_valid):
    """One launch: the target-size triple (``size`` not None), the full-resolution triple (``full``), or both."""
    t = depth_u16
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.IdhError("depth must be a tensor on the MI355X (there is no CPU fallback)")
    if t.dtype != torch.uint16:
        raise _lib.IdhError(f"depth must be uint16 (got {t.dtype})")
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3 or t.shape[1] < 1 or t.shape[2] < 1:
        raise _lib.IdhError(f"depth {tuple(t.shape)} must be (B,H,W)")
    t = t.contiguous()
    B, Hs, Ws = t.shape
    a = _lib.IngestDepthArgs()
    a.depth_bHW, a.value_scale, a.min_valid, a.max_valid = t.data_ptr(), float(value_scale), float(min_valid), float(max_valid)
    a.B, a.Hs, a.Ws = B, Hs, Ws

    def triple(h, w):
        return (torch.empty(B, 1, h, w, device=t.device), torch.empty(B, 1, h, w, device=t.device),
                torch.empty(B, 1, h, w, dtype=torch.bool, device=t.device))

    target = full_res = None
    if size is not None:
        a.h, a.w = _size("size", size)
        target = triple(a.h, a.w)
        a.depth_b1hw, a.mask_b1hw, a.mask_b_b1hw = (x.data_ptr() for x in target)
    if full:
        full_res = triple(Hs, Ws)
        a.full_depth_b1HW, a.full_mask_b1HW, a.full_mask_b_b1HW = (x.data_ptr() for x in full_res)
    _lib.check(_lib.lib().idh_ingest_depth_fwd(a, _lib.stream_ptr()), "idh_ingest_depth_fwd")
    return target, full_res


def load_depth(depth_u16: torch.Tensor, size: Optional[Tuple[int, int]] = None, value_scale: float = 1e-3, min_valid: float = 1e-3,
               max_valid: float = 10.0):
    """``(depth, mask, mask_b)``, each (B,1,h,w), of uint16 (B,H,W) depths: ``resize(NEAREST)`` to ``size`` (None: the source's resolution),
    ``float(v) * value_scale`` in fp32, ``mask_b = depth > min_valid & depth < max_valid``, ``mask`` its float form and NaN in ``depth``
    where invalid (scannet_dataset.py:515-530, :550-561).  Bit-exact."""
    target, full_res = _depth(depth_u16, size, size is None, value_scale, min_valid, max_valid)
    return full_res if size is None else target


def intrinsics_pyramid(K_44, native_size: Tuple[int, int], depth_size: Tuple[int, int], include_full_depth_K: bool = False) -> Dict[str, np.ndarray]:
    """``load_intrinsics`` (scannet_dataset.py:466-486) in numpy float32 on the host: ``K`` (4,4) or (B,4,4) holds for an image of
    ``native_size``; rows 0 and 1 are scaled to ``depth_size``, then ``K_s{i}_b44`` has ``[:2] /= 2**i`` and ``invK_s{i}_b44`` is its
    ``np.linalg.inv`` for i in 0..4.  ``include_full_depth_K`` adds ``K_full_depth_b44`` / ``invK_full_depth_b44`` of the unscaled matrix.
    The shape of ``K`` is kept."""
    K = np.array(K_44.detach().cpu().numpy() if isinstance(K_44, torch.Tensor) else K_44, dtype=np.float32, copy=True)
    if K.shape[-2:] != (4, 4) or K.ndim not in (2, 3):
        raise _lib.IdhError(f"K {K.shape} must be (4,4) or (B,4,4)")
    (H, W), (dh, dw) = _size("native_size", native_size), _size("depth_size", depth_size)
    out = {}
    if include_full_depth_K:
        out["K_full_depth_b44"] = K.copy()
        out["invK_full_depth_b44"] = np.linalg.inv(K)
    K[..., 0, :] *= dw / float(W)
    K[..., 1, :] *= dh / float(H)
    for i in range(5):
        Ks = K.copy()
        Ks[..., :2, :] /= 2 ** i
        out[f"K_s{i}_b44"] = Ks
        out[f"invK_s{i}_b44"] = np.linalg.inv(Ks)
    return out


class FrameIngest:
    """What ``get_frame`` (generic_mvs_dataset.py:560-634) returns for a batch of frames, computed from tensors instead of files: the
    dictionary ``fused_forward``'s ``forward`` takes as ``cur_data`` (or, with a view dimension added by the caller, ``src_data``).

    ``image_size`` / ``depth_size``: the model's image and depth resolutions; ``resample``: the dataset's colour filter ("bilinear":
    scannet, hypersim; "bicubic": arkit, vdr, 7scenes, colmap, scanniverse); ``high_res_size`` adds ``high_res_color_b3hw``;
    ``include_full_res_depth`` the ``full_res_*`` triple; ``include_full_depth_K`` the unscaled intrinsics."""

    def __init__(self, image_size: Tuple[int, int], depth_size: Tuple[int, int], resample: str = "bilinear",
                 high_res_size: Optional[Tuple[int, int]] = None, include_full_res_depth: bool = False, include_full_depth_K: bool = False,
                 value_scale: float = 1e-3, min_valid: float = 1e-3, max_valid: float = 10.0):
        self.image_size, self.depth_size = _size("image_size", image_size), _size("depth_size", depth_size)
        self.high_res_size = None if high_res_size is None else _size("high_res_size", high_res_size)
        _filter(resample)
        self.resample = resample
        self.include_full_res_depth, self.include_full_depth_K = bool(include_full_res_depth), bool(include_full_depth_K)
        self.value_scale, self.min_valid, self.max_valid = float(value_scale), float(min_valid), float(max_valid)

    def __call__(self, frames_u8: torch.Tensor, world_T_cam, K, depth_u16: Optional[torch.Tensor] = None,
                 native_size: Optional[Tuple[int, int]] = None) -> Dict[str, torch.Tensor]:
        """``frames_u8`` uint8 (B,H,W,3) on the GPU; ``world_T_cam`` (B,4,4) poses and ``K`` (4,4) or (B,4,4) intrinsics as host arrays
        (numpy or CPU tensors); ``depth_u16`` uint16 (B,Hd,Wd) on the GPU or None.  ``native_size``: the image size ``K`` holds for
        (default: the depth's when one is given, as ScanNet's intrinsic_depth.txt, otherwise the frames')."""
        out = {"image_b3hw": load_color(frames_u8, self.image_size, self.resample)}
        B, dev = frames_u8.shape[0], frames_u8.device
        if self.high_res_size is not None:
            out["high_res_color_b3hw"] = load_color(frames_u8, self.high_res_size, self.resample)
        if depth_u16 is not None:
            target, full_res = _depth(depth_u16, self.depth_size, self.include_full_res_depth, self.value_scale, self.min_valid, self.max_valid)
            out["depth_b1hw"], out["mask_b1hw"], out["mask_b_b1hw"] = target
            if full_res is not None:
                out["full_res_depth_b1hw"], out["full_res_mask_b1hw"], out["full_res_mask_b_b1hw"] = full_res
        elif self.include_full_res_depth:
            raise _lib.IdhError("include_full_res_depth needs a depth")
        if native_size is None:
            native_size = tuple(depth_u16.shape[-2:]) if depth_u16 is not None else tuple(frames_u8.shape[1:3])
        pose = np.array(world_T_cam.detach().cpu().numpy() if isinstance(world_T_cam, torch.Tensor) else world_T_cam, dtype=np.float32)
        if pose.shape != (B, 4, 4):
            raise _lib.IdhError(f"world_T_cam {pose.shape} must be ({B},4,4)")
        mats = {"world_T_cam_b44": pose, "cam_T_world_b44": np.linalg.inv(pose)}  # load_pose, scannet_dataset.py:579-580
        for k, v in intrinsics_pyramid(K, native_size, self.depth_size, self.include_full_depth_K).items():
            mats[k] = np.broadcast_to(v, (B, 4, 4))
        on_dev = torch.from_numpy(np.stack(list(mats.values()))).to(dev)  # one host-to-device copy for all of them
        out.update(zip(mats, on_dev.unbind(0)))
        return out
