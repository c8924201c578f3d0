"""TSDF fusion of depth maps and the ray cast of the fused surface into live cameras (include/idh_fusion.h, csrc/tsdf.hip).

``raster.warp_depth`` draws remembered depth maps as separate sheets: the nearest one wins, holes stay holes, and a map that has left
the ring is forgotten.  ``TSDFVolume`` averages every map into a dense truncated signed distance grid (Curless and Levoy) - the step
the reference's workflow takes off line with open3d before ``--temporal_eval`` - and ``raycast`` returns the fused surface in any camera.
``extract_mesh`` turns the volume into an indexed triangle mesh (marching cubes, csrc/tsdf_mesh.hip) that the mesh
consumers of ``raster`` and ``evaluation`` take as it is.  There is no CPU fallback: the tensors live on the GPU and every step is a
HIP kernel.

Colour: a volume made with ``color=True`` also holds ``colors``, (Nz,Ny,Nx,4) float32 {R, G, B, Wc}; ``integrate_depth``
then takes the camera frames that belong to the depth maps, ``raycast_volume(return_color=True)`` returns the surface's colour in the
live camera and ``extract_mesh(return_colors=True)`` the colour of every vertex.

A volume that follows the camera: ``TSDFVolume.shift`` moves the grid under its contents by whole voxels in one
launch, ``crop`` and ``leaving_boxes`` keep what such a move drops, and ``follow_shift`` is the rule ``StreamingSession.start_fusion(
follow=)`` moves by.

Pose alignment: ``align_depth`` fits the camera of one depth map to what the volume already holds - Gauss-Newton on
the signed distance field itself, two launches per iteration and no host synchronisation - and ``alignment_summary`` reads its records."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib

FLAG_HIT, FLAG_NONE_KNOWN, FLAG_SOME_KNOWN, FLAG_NO_NORMAL = _lib.TSDF_HIT, _lib.TSDF_NONE_KNOWN, _lib.TSDF_SOME_KNOWN, _lib.TSDF_NO_NORMAL
MESH_USE_BLOCK_FLAGS = True  # extract_mesh's default: skip blocks no map has touched (same tensors either way; DESIGN.md §4.22 has the timings)


def _mats(name, t, device) -> torch.Tensor:
    t = torch.as_tensor(t).to(device=device, dtype=torch.float32)
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or tuple(t.shape[1:]) != (4, 4):
        raise _lib.IdhError(f"{name} {tuple(t.shape)} must be (N,4,4)")
    return t.contiguous()


class TSDFVolume:
    """A dense TSDF grid of ``dims`` = (Nz, Ny, Nx) voxels of ``voxel_size`` metres, axis-aligned with the world; ``origin`` is the world
    (x, y, z) of the centre of voxel (0,0,0).  ``values`` is the (Nz,Ny,Nx,2) float32 tensor of {T, W} pairs - distance in units of the
    truncation ``trunc_voxels * voxel_size`` and observation count - ``{1, 0}`` when empty; ``block_flags`` the per-block bytes the ray
    cast's empty-space skipping reads (include/idh_fusion.h says what they guarantee).  ``max_weight`` caps W.  With ``color=True``
    ``colors`` is the (Nz,Ny,Nx,4) float32 tensor of {R, G, B, Wc} quads - channels in units of a uint8 channel and the number of colour
    observations - all zero when empty; otherwise it is None."""

    def __init__(self, dims: Sequence[int], voxel_size: float, origin: Sequence[float], trunc_voxels: float = 3.0, max_weight: float = 64.0,
                 device="cuda", _values: Optional[torch.Tensor] = None, color: bool = False, _colors: Optional[torch.Tensor] = None):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3:
            raise _lib.IdhError(f"TSDFVolume: dims {dims} must be (Nz, Ny, Nx)")
        self.voxel_size, self.trunc_voxels, self.max_weight = float(voxel_size), float(trunc_voxels), float(max_weight)
        self.origin = tuple(float(o) for o in np.asarray(origin, dtype=np.float64).reshape(3))
        nbytes = _lib.lib().idh_tsdf_block_flag_bytes(*self.dims)
        if nbytes == 0 or self.dims[0] * self.dims[1] * self.dims[2] >= 2 ** 31:
            raise _lib.IdhError(f"TSDFVolume: every dim of {self.dims} must be >= 2 and their product below 2^31")
        if _values is None:
            self.values = torch.empty(*self.dims, 2, device=device, dtype=torch.float32)
        else:
            _lib.require_cuda_f32(_values)
            if tuple(_values.shape) != (*self.dims, 2) or not _values.is_contiguous():
                raise _lib.IdhError(f"TSDFVolume.from_values: values {tuple(_values.shape)} must be contiguous {(*self.dims, 2)}")
            self.values = _values
        self.block_flags = torch.empty(nbytes, device=self.values.device, dtype=torch.uint8)
        self.colors: Optional[torch.Tensor] = None
        self._spare: Optional[tuple] = None  # shift()'s second set of (values, block_flags, colors), made at its first call
        if _colors is not None:
            _lib.require_cuda_f32(_colors)
            if tuple(_colors.shape) != (*self.dims, 4) or not _colors.is_contiguous() or _colors.device != self.values.device or _colors.data_ptr() % 16:
                raise _lib.IdhError(f"TSDFVolume: colors {tuple(_colors.shape)} must be contiguous {(*self.dims, 4)}, 16-byte aligned, on the values' device")
            self.colors = _colors
        elif color:
            self.colors = torch.zeros(*self.dims, 4, device=self.values.device, dtype=torch.float32)
        if _values is None:
            self.reset()
        else:
            _lib.check(_lib.lib().idh_tsdf_flags_fwd(C.byref(self._struct()), _lib.stream_ptr()), "idh_tsdf_flags_fwd")

    @classmethod
    def from_values(cls, values: torch.Tensor, voxel_size: float, origin: Sequence[float], trunc_voxels: float = 3.0,
                    max_weight: float = 64.0, colors: Optional[torch.Tensor] = None) -> "TSDFVolume":
        """Adopt a (Nz,Ny,Nx,2) pair tensor made elsewhere (it is not copied) and rebuild the block flags from it (idh_tsdf_flags_fwd);
        ``colors`` adopts a (Nz,Ny,Nx,4) quad tensor the same way."""
        return cls(tuple(values.shape[:3]), voxel_size, origin, trunc_voxels, max_weight, device=values.device, _values=values, _colors=colors)

    def _struct(self) -> "_lib.TsdfVolume":
        v = _lib.TsdfVolume()
        v.values, v.block_flags, v.block_flag_bytes = self.values.data_ptr(), self.block_flags.data_ptr(), self.block_flags.numel()
        v.origin[0], v.origin[1], v.origin[2] = self.origin
        v.voxel_size, v.trunc_voxels = self.voxel_size, self.trunc_voxels
        v.Nz, v.Ny, v.Nx = self.dims
        return v

    def reset(self) -> None:
        """Every voxel back to {1, 0}, every block flag to 0, every colour quad to zero; the storage is kept."""
        _lib.check(_lib.lib().idh_tsdf_reset_fwd(C.byref(self._struct()), _lib.stream_ptr()), "idh_tsdf_reset_fwd")
        if self.colors is not None:
            self.colors.zero_()

    def integrate(self, depth_m1hw: torch.Tensor, K_m44, cam_T_world_m44, color_u8: Optional[torch.Tensor] = None, color_K=None,
                  weight: Optional[torch.Tensor] = None) -> None:
        integrate_depth(self, depth_m1hw, K_m44, cam_T_world_m44, color_u8, color_K, weight_m1hw=weight)

    def raycast(self, world_T_cam_b44, invK_b44, size: Sequence[int], near: float = 0.25, far: float = 8.0, step_voxels: float = 1.0,
                empty_depth: float = -1.0, return_normals: bool = False, world_normals: bool = True, skip: bool = False,
                return_color: bool = False) -> Dict[str, torch.Tensor]:
        """``raycast_volume`` with ``max_steps = ceil((far - near) / (step_voxels * voxel_size))`` formed on the host."""
        step = float(np.float32(step_voxels) * np.float32(self.voxel_size))
        if not (step > 0 and far > near):
            raise _lib.IdhError(f"TSDFVolume.raycast: far = {far} must exceed near = {near} and the step be positive")
        return raycast_volume(self, world_T_cam_b44, invK_b44, size, near=near, step_voxels=step_voxels, max_steps=int(math.ceil((far - near) / step)),
                              empty_depth=empty_depth, return_normals=return_normals, world_normals=world_normals, skip=skip, return_color=return_color)

    def extract_mesh(self, min_weight: float = 0.0, return_weights: bool = False, use_block_flags: bool = MESH_USE_BLOCK_FLAGS,
                     return_colors: bool = False) -> Dict[str, torch.Tensor]:
        return extract_mesh(self, min_weight, return_weights, use_block_flags, return_colors)

    def align(self, depth_11hw: torch.Tensor, invK, world_T_cam, **kw) -> Dict[str, torch.Tensor]:
        """``align_depth`` of this volume."""
        return align_depth(self, depth_11hw, invK, world_T_cam, **kw)

    def _origin_after(self, voxels_xyz) -> tuple:
        """``origin + voxel_size * voxels`` per axis in float32 (one multiply, one add): the arithmetic idh_tsdf_shift_fwd checks bit for bit."""
        v = np.float32(self.voxel_size)
        return tuple(float(np.float32(o) + v * np.float32(k)) for o, k in zip(self.origin, voxels_xyz))

    def shift(self, shift_xyz: Sequence[int]) -> None:
        """Move the grid ``shift_xyz`` = (sx, sy, sz) whole voxels along the world's axes under its contents (idh_tsdf_shift_fwd, one
        launch): ``origin`` becomes ``origin + voxel_size * shift`` (formed in float32), every world lattice point the
        old and the new grid share keeps its {T, W} pair and its colour bit for bit, what comes in is empty and what leaves is dropped -
        ``crop`` the ``leaving_boxes`` first to keep it.  Voxels never observed (W == 0) arrive as ``{1, 0}`` with a zero colour
        whatever they held, and ``block_flags`` are rebuilt.  Any integers are allowed: a zero shift is a normalising copy, a shift of
        a whole dim or more empties the volume.

        The shift writes into a second set of ``values`` / ``block_flags`` / ``colors`` tensors, allocated at the first call and kept:
        a volume that has been shifted holds TWICE its memory (8 + 16 bytes more per voxel with colours).  Afterwards the attributes
        name the tensors just written and the previous ones are the spare: a reference to ``values``, ``block_flags`` or ``colors``
        taken before the call now names the spare, which the next ``shift`` overwrites."""
        s = tuple(int(k) for k in shift_xyz)
        if len(s) != 3 or any(not -2 ** 31 <= k < 2 ** 31 for k in s):
            raise _lib.IdhError(f"TSDFVolume.shift: shift {shift_xyz} must be three int32 (sx, sy, sz)")
        if self._spare is None:
            self._spare = (torch.empty_like(self.values), torch.empty_like(self.block_flags),
                           None if self.colors is None else torch.empty_like(self.colors))
        values, flags, colors = self._spare
        origin = self._origin_after(s)
        a = _lib.TsdfShiftArgs()
        a.src = self._struct()
        a.dst = self._struct()
        a.dst.values, a.dst.block_flags = values.data_ptr(), flags.data_ptr()
        a.dst.origin[0], a.dst.origin[1], a.dst.origin[2] = origin
        a.src_colors_zyx4, a.dst_colors_zyx4 = _lib.ptr(self.colors), _lib.ptr(colors)
        a.shift[0], a.shift[1], a.shift[2] = s
        _lib.check(_lib.lib().idh_tsdf_shift_fwd(C.byref(a), _lib.stream_ptr()), "idh_tsdf_shift_fwd")
        self._spare = (self.values, self.block_flags, self.colors)
        self.values, self.block_flags, self.colors = values, flags, colors
        self.origin = origin

    def crop(self, lo_xyz: Sequence[int], hi_xyz: Sequence[int]) -> "TSDFVolume":
        """A new ``TSDFVolume`` holding a COPY of the voxels ``lo_xyz`` .. ``hi_xyz`` (inclusive, (x, y, z), at least two per axis): their
        pairs, their colours if the volume has any, ``origin + voxel_size * lo`` (in float32) as its origin and block flags rebuilt from
        the copy (idh_tsdf_flags_fwd).  What a caller uses to keep - mesh, save - the ``leaving_boxes`` before a ``shift`` drops them."""
        lo, hi = tuple(int(k) for k in lo_xyz), tuple(int(k) for k in hi_xyz)
        nz, ny, nx = self.dims
        if len(lo) != 3 or len(hi) != 3 or any(not 0 <= a < b < n for a, b, n in zip(lo, hi, (nx, ny, nz))):
            raise _lib.IdhError(f"TSDFVolume.crop: {lo_xyz} .. {hi_xyz} must be an inclusive (x, y, z) box of at least two voxels per axis inside {(nx, ny, nz)}")
        box = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
        values = self.values[box].clone(memory_format=torch.contiguous_format)
        colors = None if self.colors is None else self.colors[box].clone(memory_format=torch.contiguous_format)
        return TSDFVolume.from_values(values, self.voxel_size, self._origin_after(lo), self.trunc_voxels, self.max_weight, colors=colors)


def leaving_boxes(dims: Sequence[int], shift_xyz: Sequence[int]) -> list:
    """The voxels of a volume of ``dims`` = (Nz, Ny, Nx) that ``TSDFVolume.shift(shift_xyz)`` drops, as at most three disjoint inclusive
    boxes ``(lo_xyz, hi_xyz)`` of the CURRENT (unshifted) volume whose union is exactly that set: the slab that leaves along x over all
    y and z, then the slab along y over the x that stay, then the slab along z over the x and y that stay.  Empty for a zero shift; one
    box, the whole volume, when the shift is a whole dim or more on an axis.  Pure host arithmetic."""
    n = (int(dims[2]), int(dims[1]), int(dims[0]))
    s = tuple(int(k) for k in shift_xyz)
    if len(s) != 3 or len(dims) != 3 or min(n) < 1:
        raise _lib.IdhError(f"leaving_boxes: dims {dims} must be (Nz, Ny, Nx) and shift {shift_xyz} (sx, sy, sz)")
    if any(abs(k) >= m for k, m in zip(s, n)):
        return [((0, 0, 0), (n[0] - 1, n[1] - 1, n[2] - 1))]
    # voxel a stays when 0 <= a - s < N: per axis the range that stays and the range that leaves (s > 0 drops the low end)
    stay = [(max(k, 0), m - 1 + min(k, 0)) for k, m in zip(s, n)]
    leave = [None if k == 0 else (0, k - 1) if k > 0 else (m + k, m - 1) for k, m in zip(s, n)]
    boxes = []
    for axis in range(3):
        if leave[axis] is None:
            continue
        r = [stay[i] if i < axis else leave[i] if i == axis else (0, n[i] - 1) for i in range(3)]
        boxes.append((tuple(a for a, _ in r), tuple(b for _, b in r)))
    return boxes


def follow_shift(cam_xyz: Sequence[float], origin: Sequence[float], dims: Sequence[int], voxel_size: float, slack: float) -> tuple:
    """The shift (sx, sy, sz) that brings a volume of ``dims`` = (Nz, Ny, Nx) back under a camera at ``cam_xyz``, in float64 on the host.
    Per axis c = (cam - centre) / voxel_size with centre = origin + voxel_size * (N - 1) / 2.  While no |c| exceeds
    ``slack / voxel_size`` the answer is (0, 0, 0); otherwise every axis moves by ``8 * floor(c / 8 + 0.5)``: whole 8-voxel blocks, so
    the block grid of a scrolled volume stays aligned with its contents, and the camera ends within 4 voxels of the centre."""
    v = float(voxel_size)
    n = np.array([dims[2], dims[1], dims[0]], dtype=np.float64)
    centre = np.asarray(origin, dtype=np.float64).reshape(3) + v * (n - 1.0) / 2.0
    c = (np.asarray(cam_xyz, dtype=np.float64).reshape(3) - centre) / v
    if not (np.abs(c) > float(slack) / v).any():
        return (0, 0, 0)
    return tuple(int(k) for k in 8 * np.floor(c / 8.0 + 0.5))


def integrate_depth(volume: TSDFVolume, depth_m1hw: torch.Tensor, K_m44, cam_T_world_m44, color_u8: Optional[torch.Tensor] = None,
                    color_K=None, weight_m1hw: Optional[torch.Tensor] = None) -> None:
    """Average M depth maps (M,1,h,w) into ``volume`` in one launch (idh_tsdf_integrate_fwd): ``K_m44`` their intrinsics at h x w,
    ``cam_T_world_m44`` their poses ((4,4) or (M,4,4), tensors or arrays).  Taps that are not finite and positive are holes.  M is at most
    ``pipeline.MAX_RING_CAPACITY``.  One call with M maps equals M calls with one map each, bit for bit.

    ``color_u8``: the M camera frames of the maps, uint8 (M,hc,wc,3) RGB on the GPU, averaged into ``volume.colors`` in the same launch
    (idh_tsdf_integrate_color_fwd; ``values`` and ``block_flags`` get the same bits as without).  ``color_K`` their intrinsics at
    hc x wc; None is allowed only when (hc, wc) == (h, w) and then means ``K_m44``.  Without ``color_u8`` the colours are left as they
    are (depth-only maps).

    ``weight_m1hw`` (M,1,h,w): a weight per depth sample (idh_tsdf_integrate_weighted_fwd), e.g. the "weight" of
    ``geometry.depth_consistency``: a sample enters the averages of T and of the colour with that weight and adds it to W and Wc; one
    whose weight is not finite and positive is skipped like a hole.  Weights of 1 give the bits of the call without weights."""
    _lib.require_cuda_f32(depth_m1hw, weight_m1hw)
    if weight_m1hw is not None and weight_m1hw.shape != depth_m1hw.shape:
        raise _lib.IdhError(f"integrate_depth: weight {tuple(weight_m1hw.shape)} must be {tuple(depth_m1hw.shape)}")
    if depth_m1hw.dim() != 4 or depth_m1hw.shape[1] != 1:
        raise _lib.IdhError(f"integrate_depth: depth {tuple(depth_m1hw.shape)} must be (M,1,h,w)")
    M, _, h, w = depth_m1hw.shape
    dev = volume.values.device
    d, K, T = depth_m1hw.contiguous(), _mats("K", K_m44, dev), _mats("cam_T_world", cam_T_world_m44, dev)
    if K.shape[0] != M or T.shape[0] != M:
        raise _lib.IdhError(f"integrate_depth: {M} maps need ({M},4,4) intrinsics and poses, got {tuple(K.shape)} and {tuple(T.shape)}")
    if color_u8 is None and color_K is not None:
        raise _lib.IdhError("integrate_depth: color_K without color_u8")
    if color_u8 is not None:
        if volume.colors is None:
            raise _lib.IdhError("integrate_depth: colour frames for a volume without colors (TSDFVolume(..., color=True))")
        if color_u8.dtype != torch.uint8 or not color_u8.is_cuda or color_u8.dim() != 4 or color_u8.shape[0] != M or color_u8.shape[3] != 3:
            raise _lib.IdhError(f"integrate_depth: color_u8 {tuple(color_u8.shape)} {color_u8.dtype} must be uint8 ({M},hc,wc,3) on the GPU")
        hc, wc = int(color_u8.shape[1]), int(color_u8.shape[2])
        if color_K is None:
            if (hc, wc) != (h, w):
                raise _lib.IdhError(f"integrate_depth: frames of {(hc, wc)} for maps of {(h, w)} need color_K")
            Kc = K
        else:
            Kc = _mats("color_K", color_K, dev)
            if Kc.shape[0] != M:
                raise _lib.IdhError(f"integrate_depth: {M} frames need ({M},4,4) color_K, got {tuple(Kc.shape)}")
        frames = color_u8.contiguous()
        a = _lib.TsdfIntegrateColorArgs() if weight_m1hw is None else _lib.TsdfIntegrateWeightedArgs()
        a.colors_zyx4, a.color_mhw3, a.color_K_m44, a.hc, a.wc = volume.colors.data_ptr(), frames.data_ptr(), Kc.data_ptr(), hc, wc
        fn, name = _lib.lib().idh_tsdf_integrate_color_fwd, "idh_tsdf_integrate_color_fwd"
    else:
        a = _lib.TsdfIntegrateArgs() if weight_m1hw is None else _lib.TsdfIntegrateWeightedArgs()
        fn, name = _lib.lib().idh_tsdf_integrate_fwd, "idh_tsdf_integrate_fwd"
    if weight_m1hw is not None:
        wgt = weight_m1hw.contiguous()
        a.weight_m1hw = wgt.data_ptr()
        fn, name = _lib.lib().idh_tsdf_integrate_weighted_fwd, "idh_tsdf_integrate_weighted_fwd"
    a.volume = volume._struct()
    a.depth_m1hw, a.K_m44, a.cam_T_world_m44 = d.data_ptr(), K.data_ptr(), T.data_ptr()
    a.max_weight, a.M, a.h, a.w = volume.max_weight, M, h, w
    _lib.check(fn(C.byref(a), _lib.stream_ptr()), name)


def raycast_volume(volume: TSDFVolume, world_T_cam_b44, invK_b44, size: Sequence[int], *, near: float = 0.25, step_voxels: float = 1.0,
                   max_steps: int = 194, empty_depth: float = -1.0, return_normals: bool = False, world_normals: bool = True,
                   skip: bool = False, return_color: bool = False) -> Dict[str, torch.Tensor]:
    """The fused surface in B cameras in one launch (idh_tsdf_raycast_fwd).  ``world_T_cam_b44`` / ``invK_b44``: (4,4) or (B,4,4), the
    inverse intrinsics at ``size`` = (H, W).  Every pixel's ray is sampled at ``t_k = near + k * step_voxels * voxel_size``, k below
    ``max_steps``; the first sign change from positive to non-positive between two known samples is the hit.  Returns

    * ``"depth"`` (B,1,H,W): the live camera's z of the hit, ``empty_depth`` where there is none;
    * ``"flags"`` (B,H,W) uint8: ``FLAG_HIT``, ``FLAG_NONE_KNOWN`` (nothing is known along the ray), ``FLAG_SOME_KNOWN`` (part of it is);
      0 is a ray through observed free space;
    * ``"normals"`` (B,3,H,W) with ``return_normals``: unit normals facing the camera, in the world's frame or (``world_normals=False``)
      the camera's; zero where there is no hit or ``FLAG_NO_NORMAL`` is set;
    * ``"rgba"`` (B,H,W,4) uint8 with ``return_color`` (idh_tsdf_raycast_color_fwd, a volume with ``colors``; the layout of
      ``render_shaded``'s "rgba"): the colour of the hit from the coloured corners of its cell, alpha 255; four zero bytes where there
      is no hit or no coloured corner.  The other outputs keep their bits.

    ``skip=False`` (the default) marches every sample; ``skip=True`` clips the range to the volume and jumps unobserved blocks, and returns
    the same bits.  Measured, it is faster where most rays cross unobserved space and slower in a room that has been seen (DESIGN.md
    §4.21), which is why it is not the default."""
    dev = volume.values.device
    T, iK = _mats("world_T_cam", world_T_cam_b44, dev), _mats("invK", invK_b44, dev)
    B, (H, W) = T.shape[0], (int(s) for s in size)
    if iK.shape[0] != B:
        raise _lib.IdhError(f"raycast_volume: {B} poses need ({B},4,4) inverse intrinsics, got {tuple(iK.shape)}")
    if B <= 0 or H <= 0 or W <= 0:
        raise _lib.IdhError(f"raycast_volume: B = {B}, H = {H} and W = {W} must be positive")
    out = {"depth": torch.empty(B, 1, H, W, device=dev), "flags": torch.empty(B, H, W, device=dev, dtype=torch.uint8)}
    if return_normals:
        out["normals"] = torch.empty(B, 3, H, W, device=dev)
    if return_color:
        if volume.colors is None:
            raise _lib.IdhError("raycast_volume: return_color needs a volume with colors (TSDFVolume(..., color=True))")
        out["rgba"] = torch.empty(B, H, W, 4, device=dev, dtype=torch.uint8)
        a = _lib.TsdfRaycastColorArgs()
        a.colors_zyx4, a.rgba_bhw4 = volume.colors.data_ptr(), out["rgba"].data_ptr()
        fn, name = _lib.lib().idh_tsdf_raycast_color_fwd, "idh_tsdf_raycast_color_fwd"
    else:
        a = _lib.TsdfRaycastArgs()
        fn, name = _lib.lib().idh_tsdf_raycast_fwd, "idh_tsdf_raycast_fwd"
    a.volume = volume._struct()
    a.world_T_cam_b44, a.invK_b44 = T.data_ptr(), iK.data_ptr()
    a.depth_b1hw, a.flags_bhw, a.normals_b3hw = out["depth"].data_ptr(), out["flags"].data_ptr(), _lib.ptr(out.get("normals"))
    a.near, a.step_voxels, a.empty_depth, a.max_steps = float(near), float(step_voxels), float(empty_depth), int(max_steps)
    a.world_normals, a.skip, a.B, a.H, a.W = int(bool(world_normals)), int(bool(skip)), B, H, W
    _lib.check(fn(C.byref(a), _lib.stream_ptr()), name)
    return out


def _mesh_args(volume: TSDFVolume, workspace: torch.Tensor, min_weight: float, use_block_flags: bool) -> "_lib.TsdfMeshArgs":
    a = _lib.TsdfMeshArgs()
    a.volume = volume._struct()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    a.min_weight, a.use_block_flags = float(min_weight), int(bool(use_block_flags))
    return a


def mesh_count(volume: TSDFVolume, min_weight: float = 0.0, use_block_flags: bool = MESH_USE_BLOCK_FLAGS):
    """The first half of ``extract_mesh`` (idh_tsdf_mesh_count_fwd): classify every cell and scan the counts.  Returns ``(workspace,
    totals)``: the uint8 workspace ``mesh_emit`` reads and the int32 device tensor ``{V, F}``; nothing is read back to the host."""
    nbytes = _lib.lib().idh_tsdf_mesh_workspace_bytes(*volume.dims)
    if nbytes == 0:
        raise _lib.IdhError(f"extract_mesh: a volume of {volume.dims} has more than 2^28 voxels")
    dev = volume.values.device
    workspace, totals = torch.empty(nbytes, device=dev, dtype=torch.uint8), torch.empty(2, device=dev, dtype=torch.int32)
    a = _mesh_args(volume, workspace, min_weight, use_block_flags)
    a.totals = totals.data_ptr()
    _lib.check(_lib.lib().idh_tsdf_mesh_count_fwd(C.byref(a), _lib.stream_ptr()), "idh_tsdf_mesh_count_fwd")
    return workspace, totals


def mesh_emit(volume: TSDFVolume, workspace: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, weights: Optional[torch.Tensor] = None,
              min_weight: float = 0.0, vert_capacity: Optional[int] = None, face_capacity: Optional[int] = None) -> None:
    """The second half (idh_tsdf_mesh_emit_fwd): the first ``vert_capacity`` vertices into ``verts`` (rows, 3) float32 (and ``weights``
    (rows,)), the first ``face_capacity`` faces into ``faces`` (rows, 3) int32, after ``mesh_count`` on the same volume.  The capacities
    default to the tensors' rows and may not exceed them; nothing is written past them whatever the totals are."""
    _lib.require_cuda_f32(verts, weights)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32 or not faces.is_cuda:
        raise _lib.IdhError(f"mesh_emit: verts {tuple(verts.shape)} must be (V,3) float32 and faces {tuple(faces.shape)} {faces.dtype} (F,3) int32 on the GPU")
    if not (verts.is_contiguous() and faces.is_contiguous() and (weights is None or weights.is_contiguous())):
        raise _lib.IdhError("mesh_emit: the outputs must be contiguous")
    vcap = verts.shape[0] if vert_capacity is None else int(vert_capacity)
    fcap = faces.shape[0] if face_capacity is None else int(face_capacity)
    if vcap > verts.shape[0] or fcap > faces.shape[0] or (weights is not None and (weights.dim() != 1 or vcap > weights.shape[0])):
        raise _lib.IdhError(f"mesh_emit: capacities ({vcap}, {fcap}) exceed the tensors' rows")
    a = _mesh_args(volume, workspace, min_weight, False)
    # a tensor of no rows may have a null pointer: the C call wants an address even when it stores nothing there
    a.verts_v3, a.faces_f3, a.weights_v = verts.data_ptr() or workspace.data_ptr(), faces.data_ptr() or workspace.data_ptr(), _lib.ptr(weights)
    a.vert_capacity, a.face_capacity = vcap, fcap
    _lib.check(_lib.lib().idh_tsdf_mesh_emit_fwd(C.byref(a), _lib.stream_ptr()), "idh_tsdf_mesh_emit_fwd")


def mesh_colors(volume: TSDFVolume, workspace: torch.Tensor, rgba: torch.Tensor, min_weight: float = 0.0, vert_capacity: Optional[int] = None) -> None:
    """The colours of ``mesh_emit``'s vertices (idh_tsdf_mesh_colors_fwd): the first ``vert_capacity`` of them into ``rgba`` (rows, 4)
    uint8, after ``mesh_count`` on the same volume.  The capacity defaults to the tensor's rows and may not exceed them."""
    if volume.colors is None:
        raise _lib.IdhError("mesh_colors needs a volume with colors (TSDFVolume(..., color=True))")
    if rgba.dim() != 2 or rgba.shape[1] != 4 or rgba.dtype != torch.uint8 or not rgba.is_cuda or not rgba.is_contiguous():
        raise _lib.IdhError(f"mesh_colors: rgba {tuple(rgba.shape)} {rgba.dtype} must be contiguous (V,4) uint8 on the GPU")
    vcap = rgba.shape[0] if vert_capacity is None else int(vert_capacity)
    if vcap > rgba.shape[0]:
        raise _lib.IdhError(f"mesh_colors: capacity {vcap} exceeds the tensor's rows")
    a = _lib.TsdfMeshColorsArgs()
    a.mesh = _mesh_args(volume, workspace, min_weight, False)
    a.mesh.vert_capacity = vcap
    a.colors_zyx4, a.rgba_v4 = volume.colors.data_ptr(), rgba.data_ptr() or workspace.data_ptr()
    _lib.check(_lib.lib().idh_tsdf_mesh_colors_fwd(C.byref(a), _lib.stream_ptr()), "idh_tsdf_mesh_colors_fwd")


def extract_mesh(volume: TSDFVolume, min_weight: float = 0.0, return_weights: bool = False,
                 use_block_flags: bool = MESH_USE_BLOCK_FLAGS, return_colors: bool = False) -> Dict[str, torch.Tensor]:
    """The fused surface as an indexed triangle mesh: marching cubes over the cells whose eight voxels have ``W > min_weight``, a voxel
    being inside where ``T <= 0`` (include/idh_fusion.h states vertex positions, orders and orientation).  Returns ``"verts"`` (V,3)
    float32 in the world, ``"faces"`` (F,3) int32 with normals towards free space - what ``MeshDepthRasterizer.load_gt_mesh(verts=,
    faces=)``, ``raster.render_depth``, ``render_shaded`` and ``save_ply`` take - and with ``return_weights`` ``"weights"`` (V,), the
    observation count interpolated like the position.  Order and bits are deterministic.  Two groups of launches with one host read of the
    two totals between them; an empty result has shapes (0,3).  ``use_block_flags`` skips the blocks no map has touched and changes no
    bit.  With ``return_colors`` (a volume with ``colors``) ``"colors"`` (V,4) uint8 RGBA, what ``render_shaded(colors=)`` and
    ``save_ply(colors=)`` take: the endpoints' colours interpolated like the position, alpha 0 where neither endpoint has one; (0,4)
    for an empty mesh."""
    if return_colors and volume.colors is None:
        raise _lib.IdhError("extract_mesh: return_colors needs a volume with colors (TSDFVolume(..., color=True))")
    workspace, totals = mesh_count(volume, min_weight, use_block_flags)
    V, F = totals.tolist()  # the one host read
    dev = volume.values.device
    out = {"verts": torch.empty(V, 3, device=dev), "faces": torch.empty(F, 3, device=dev, dtype=torch.int32)}
    if return_weights:
        out["weights"] = torch.empty(V, device=dev)
    if V or F:
        mesh_emit(volume, workspace, out["verts"], out["faces"], out.get("weights"), min_weight)
    if return_colors:
        out["colors"] = torch.empty(V, 4, device=dev, dtype=torch.uint8)
        if V:
            mesh_colors(volume, workspace, out["colors"], min_weight)
    return out


ALIGN_RECORD = 40  # doubles per iteration: A (21, row-major upper triangle), b (6), cost, count, status, |v|, |w|, xi (6), two zeros
ALIGN_OK, ALIGN_TOO_FEW, ALIGN_DEGENERATE, ALIGN_STOPPED = 0, 1, 2, 3  # a record's status


def align_depth(volume: TSDFVolume, depth_11hw: torch.Tensor, invK, world_T_cam, *, iters: int = 8, stride: int = 1, huber: float = 0.0,
                damping: float = 0.0, min_step: float = 0.0, min_count: int = 64, weight_11hw: Optional[torch.Tensor] = None,
                return_rows: bool = False, schedule: Optional[Sequence[Sequence[int]]] = None, min_pivot_ratio: float = 1e-6,
                max_workgroups: int = 0) -> Dict[str, torch.Tensor]:
    """Fit the camera of one depth map (1,1,h,w) to the surface ``volume`` holds (idh_tsdf_align_fwd; include/idh_fusion.h states the
    arithmetic): Gauss-Newton on the sum of ``f(T p)^2`` over the map's back-projected points, starting from ``world_T_cam`` ((4,4) or
    (1,4,4)), with ``invK`` the inverse intrinsics at h x w.  The increment translates the camera and rotates it about its own centre.
    It converges from about a truncation distance (``trunc_voxels * voxel_size``) away, not further.

    ``iters`` (1..64) iterations of two launches each over the pixels with ``i % stride == 0 and j % stride == 0``; ``huber`` (metres,
    <= 0: none) down-weights residuals beyond it; ``damping`` adds that share of the diagonal to the normal matrix; once a step is shorter
    than ``min_step`` (metres and radians) the remaining iterations do nothing; fewer than ``min_count`` usable pixels, or a normal
    matrix with a pivot below ``min_pivot_ratio`` of its diagonal entry (a plane, say), end the fit with the pose as it is.
    ``weight_11hw``: a weight per depth sample, e.g. the "weight" of ``geometry.depth_consistency``; one that is not finite and positive
    makes the pixel a hole.  ``schedule=((stride, iters), ...)`` chains calls coarse to fine on the device instead of ``stride`` / ``iters``.

    Returns ``"world_T_cam"`` (1,4,4) float32 and ``"records"`` (iterations, 40) float64 on the device (``ALIGN_RECORD``; status 0 a step
    taken, 1 too few pixels, 2 degenerate, 3 an iteration skipped after the fit had ended) and with ``return_rows`` ``"rows"`` (h,w,8):
    ``(J[6], r, weight)`` per pixel at the input pose - ``r`` the signed distance of the pixel's point in metres, all zero where the pixel
    was not used.  Nothing is read back and nothing synchronises: ``alignment_summary`` does."""
    if schedule is None:
        schedule = ((stride, iters),)
    schedule = tuple((int(s), int(n)) for s, n in schedule)
    if not schedule or any(s < 1 or not 1 <= n <= 64 for s, n in schedule):
        raise _lib.IdhError(f"align_depth: schedule {schedule} must be (stride >= 1, iters in 1..64) pairs")
    for name, t in (("depth", depth_11hw), ("weight", weight_11hw), ("invK", invK), ("world_T_cam", world_T_cam)):
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise _lib.IdhError(f"align_depth: {name} requires grad; the alignment is not differentiable")
    if depth_11hw.dim() != 4 or depth_11hw.shape[0] != 1 or depth_11hw.shape[1] != 1:
        raise _lib.IdhError(f"align_depth: depth {tuple(depth_11hw.shape)} must be (1,1,h,w)")
    if weight_11hw is not None and weight_11hw.shape != depth_11hw.shape:
        raise _lib.IdhError(f"align_depth: weight {tuple(weight_11hw.shape)} must be {tuple(depth_11hw.shape)}")
    _lib.require_cuda_f32(depth_11hw, weight_11hw)
    dev = volume.values.device
    h, w = int(depth_11hw.shape[2]), int(depth_11hw.shape[3])
    iK, T = _mats("invK", invK, dev), _mats("world_T_cam", world_T_cam, dev)
    if iK.shape[0] != 1 or T.shape[0] != 1:
        raise _lib.IdhError(f"align_depth: one map needs one invK and one pose, got {tuple(iK.shape)} and {tuple(T.shape)}")
    d = depth_11hw.contiguous()
    wgt = None if weight_11hw is None else weight_11hw.contiguous()
    records = torch.empty(sum(n for _, n in schedule), ALIGN_RECORD, device=dev, dtype=torch.float64)
    out = {"records": records}
    if return_rows:
        out["rows"] = torch.empty(h, w, 8, device=dev)
    pose, done = T, 0
    for k, (s, n) in enumerate(schedule):
        nbytes = _lib.lib().idh_tsdf_align_workspace_bytes(h, w, s, n)
        if nbytes == 0:
            raise _lib.IdhError(f"align_depth: a map of {(h, w)} has 2^31 pixels or more")
        workspace = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
        nxt = torch.empty(1, 4, 4, device=dev)
        a = _lib.TsdfAlignArgs()
        a.volume = volume._struct()
        a.depth_11hw, a.invK_44, a.weight_11hw = d.data_ptr(), iK.data_ptr(), _lib.ptr(wgt)
        a.world_T_cam_in_44, a.world_T_cam_out_44 = pose.data_ptr(), nxt.data_ptr()
        a.records_i40 = records[done:].data_ptr()
        a.rows_hw8 = out["rows"].data_ptr() if return_rows and k == 0 else None
        a.workspace, a.workspace_bytes = workspace.data_ptr(), nbytes
        a.damping, a.min_step, a.min_pivot_ratio, a.huber = float(damping), float(min_step), float(min_pivot_ratio), float(huber)
        a.h, a.w, a.iters, a.stride, a.min_count, a.max_workgroups = h, w, n, s, int(min_count), int(max_workgroups)
        _lib.check(_lib.lib().idh_tsdf_align_fwd(C.byref(a), _lib.stream_ptr()), "idh_tsdf_align_fwd")
        pose, done = nxt, done + n
    out["world_T_cam"] = pose
    return out


def alignment_summary(records) -> Dict[str, float]:
    """What an ``align_depth`` call came to, from its ``"records"``.  A HOST helper: a device tensor is copied to the host, which
    SYNCHRONISES with the stream.  Returns ``"status"`` - that of the last iteration that ran (0 a step taken, 1 too few pixels,
    2 degenerate) -, its ``"count"`` of pixels and ``"rms"`` = sqrt(cost / count) in metres, the weighted cost per counted pixel (with
    unit weights the root mean square distance of the map's points from the surface, BEFORE that iteration's step), ``"iterations"``,
    how many ran, ``"stopped"``, whether later ones were skipped, and ``"translation"`` / ``"rotation"``: the sums of the steps' |v|
    (metres) and |w| (radians), an upper bound of the total correction."""
    r = records.detach().cpu().numpy() if isinstance(records, torch.Tensor) else np.asarray(records, dtype=np.float64)
    r = r.reshape(-1, ALIGN_RECORD)
    ran = r[r[:, 29] != ALIGN_STOPPED]
    if len(ran) == 0:
        raise _lib.IdhError("alignment_summary: no iteration ran")
    last = ran[-1]
    count = float(last[28])
    return {"status": int(last[29]), "count": int(count), "rms": float(np.sqrt(last[27] / count)) if count > 0 else float("nan"),
            "iterations": int(len(ran)), "stopped": bool(len(ran) < len(r)), "translation": float(ran[:, 30].sum()), "rotation": float(ran[:, 31].sum())}
