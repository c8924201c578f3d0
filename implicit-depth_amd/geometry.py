"""Buffer-compatible stand-ins for the reference's geometry modules.

The fused kernels do the back-projection / projection arithmetic themselves; these classes
exist so that a drop-in ``CostVolumeManager`` exposes the same ``state_dict`` buffers as the
reference (``backprojector.pix_coords_13N``, ``projector.eps`` — SURVEY.md §5 checkpoint
row; reference utils/geometry_utils.py:22-89) and loads reference checkpoints unchanged.

``NormalGenerator`` is not a stand-in: it is the reference's module (utils/geometry_utils.py:92-138) on one fused kernel
(csrc/normals.hip, include/idh_geometry.h).  ``depth_normals`` is the same kernel with its options (rotation into world
space, orientation towards the camera, a validity map from per-pixel flags); ``patch_normals`` the sparse form for 3x3 patches of points.
There is no CPU fallback.

``depth_consistency`` checks a depth map against source depth maps of other cameras in one launch (csrc/mv_consistency.hip, DESIGN.md
§4.25) with the arithmetic of the reference's ``MVDepthLoss`` (losses.py:143-261); ``MVDepthLoss`` is that module's forward value on it.

``edge_mask`` is the reference's ``get_edge_mask`` (utils/generic_utils.py:286-292, and the dataset's variant,
datasets/generic_mvs_dataset.py:650-658) without kornia and without a sort (csrc/edge_mask.hip).
"""
from typing import Optional, Tuple

import torch
from torch import nn

from . import _lib

KERNEL_SIZES = (1, 3, 5, 7)


class BackprojectDepth(nn.Module):
    def __init__(self, height: int, width: int):
        super().__init__()
        self.height, self.width = height, width
        ys, xs = torch.meshgrid(torch.arange(height), torch.arange(width), indexing="ij")
        pix = torch.stack([xs + 0.5, ys + 0.5, torch.ones_like(xs, dtype=torch.float32)], 0)
        self.register_buffer("pix_coords_13N", pix.reshape(1, 3, -1).float())


class Project3D(nn.Module):
    def __init__(self, eps: float = 1e-5):
        super().__init__()
        self.register_buffer("eps", torch.tensor(eps).view(1, 1, 1))


def _flags(name, t, shape):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.IdhError(f"{name} must be a tensor on the MI355X (there is no CPU fallback)")
    if t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape):
        raise _lib.IdhError(f"{name} must be uint8 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def depth_normals(depth_b1hw: torch.Tensor, invK_b44: torch.Tensor, *, kernel_size: int = 5, std: float = 2.0,
                  world_R_cam: Optional[torch.Tensor] = None, orient: bool = False, flags: Optional[torch.Tensor] = None,
                  need: int = 3) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Surface normals (B,3,H,W) of a depth map (B,1,H,W) as the reference's ``NormalGenerator.forward`` computes them
    (utils/geometry_utils.py:121-138; contract: include/idh_geometry.h), in one launch.  ``invK_b44`` (B,4,4): only ``[:3,:3]`` is read.
    With everything else at its default the result is the reference's, in camera space, pointing away from the camera on a fronto-parallel
    plane.  ``world_R_cam`` (B,3,3) rotates the stored normal; ``orient`` negates it where it points away from the camera (``n . p > 0``);
    ``flags`` uint8 (B,1,H,W) with ``need``: a pixel is valid iff every depth its normal read - a ``(2 (k // 2) + 3)^2`` footprint under
    the border maps - has ``flags == need``, invalid pixels hold (0,0,0).  Returns ``(normals, valid)``: ``valid`` uint8 (B,1,H,W), or
    None without ``flags``."""
    _lib.require_cuda_f32(depth_b1hw, invK_b44, world_R_cam)
    if depth_b1hw.dim() != 4 or depth_b1hw.shape[1] != 1:
        raise _lib.IdhError(f"depth {tuple(depth_b1hw.shape)} must be (B,1,H,W)")
    B, _, H, W = depth_b1hw.shape
    if tuple(invK_b44.shape) != (B, 4, 4):
        raise _lib.IdhError(f"invK {tuple(invK_b44.shape)} must be ({B},4,4)")
    if int(kernel_size) not in KERNEL_SIZES:
        raise _lib.IdhError(f"kernel_size must be one of {KERNEL_SIZES}, got {kernel_size}")
    depth, invK = depth_b1hw.contiguous(), invK_b44.contiguous()
    keep = [depth, invK]
    a = _lib.NormalsArgs()
    a.depth_b1hw, a.invK_b44 = depth.data_ptr(), invK.data_ptr()
    a.smoothing_std, a.kernel_size, a.orient, a.need = float(std), int(kernel_size), int(bool(orient)), int(need)
    a.B, a.H, a.W = B, H, W
    if world_R_cam is not None:
        if tuple(world_R_cam.shape) != (B, 3, 3):
            raise _lib.IdhError(f"world_R_cam {tuple(world_R_cam.shape)} must be ({B},3,3)")
        rot = world_R_cam.contiguous()
        keep.append(rot)
        a.world_R_cam_b33 = rot.data_ptr()
    out = torch.empty(B, 3, H, W, device=depth.device)
    valid = None
    if flags is not None:
        f = _flags("flags", flags, (B, 1, H, W))
        keep.append(f)
        valid = torch.empty(B, 1, H, W, dtype=torch.uint8, device=depth.device)
        a.flags_b1hw, a.valid_b1hw = f.data_ptr(), valid.data_ptr()
    a.normals_b3hw = out.data_ptr()
    if B == 0:  # nothing to launch (an empty tensor has no storage to point at)
        return out, valid
    _lib.check(_lib.lib().idh_depth_normals_fwd(a, _lib.stream_ptr()), "idh_depth_normals_fwd")
    return out, valid


def patch_normals(points_bn93: torch.Tensor, *, cam_centre: Optional[torch.Tensor] = None, orient: bool = False,
                  flags: Optional[torch.Tensor] = None, need: int = 3) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Normals (B,N,3) at the centres of 3x3 patches of points (B,N,9,3), row-major: the reference's gradient, cross product and
    normalisation (utils/geometry_utils.py:129-138) through the device function ``depth_normals`` uses.  ``orient`` negates a normal where
    it points along ``centre point - cam_centre`` (``cam_centre`` (B,3), required then); ``flags`` uint8 (B,N,9) with ``need``: a query is
    valid iff all nine flags equal ``need``, invalid ones hold (0,0,0).  Returns ``(normals, valid)``: ``valid`` uint8 (B,N), or None."""
    _lib.require_cuda_f32(points_bn93, cam_centre)
    if points_bn93.dim() != 4 or tuple(points_bn93.shape[2:]) != (9, 3):
        raise _lib.IdhError(f"points {tuple(points_bn93.shape)} must be (B,N,9,3)")
    B, N = points_bn93.shape[:2]
    pts = points_bn93.contiguous()
    keep = [pts]
    a = _lib.PatchNormalsArgs()
    a.points_bn93, a.orient, a.need, a.B, a.N = pts.data_ptr(), int(bool(orient)), int(need), B, N
    if orient:
        if cam_centre is None or tuple(cam_centre.shape) != (B, 3):
            raise _lib.IdhError(f"orient needs cam_centre ({B},3)")
        cc = cam_centre.contiguous()
        keep.append(cc)
        a.cam_centre_b3 = cc.data_ptr()
    out = torch.empty(B, N, 3, device=pts.device)
    valid = None
    if flags is not None:
        f = _flags("flags", flags, (B, N, 9))
        keep.append(f)
        valid = torch.empty(B, N, dtype=torch.uint8, device=pts.device)
        a.flags_bn9, a.valid_bn = f.data_ptr(), valid.data_ptr()
    a.normals_bn3 = out.data_ptr()
    if B == 0 or N == 0:
        return out, valid
    _lib.check(_lib.lib().idh_patch_normals_fwd(a, _lib.stream_ptr()), "idh_patch_normals_fwd")
    return out, valid


class NormalGenerator(nn.Module):
    """The reference's ``NormalGenerator`` (utils/geometry_utils.py:92-138): same constructor, same ``backproject.pix_coords_13N`` buffer
    in the state dict, ``forward(depth_b1hw, invK_b44) -> (B,3,H,W)`` - on the fused kernel, without kornia."""

    def __init__(self, height: int, width: int, smoothing_kernel_size: int = 5, smoothing_kernel_std: float = 2.0):
        super().__init__()
        if int(smoothing_kernel_size) not in KERNEL_SIZES:
            raise _lib.IdhError(f"smoothing_kernel_size must be one of {KERNEL_SIZES}, got {smoothing_kernel_size}")
        self.height, self.width = int(height), int(width)
        self.backproject = BackprojectDepth(self.height, self.width)
        self.kernel_size, self.std = int(smoothing_kernel_size), float(smoothing_kernel_std)

    def forward(self, depth_b1hw: torch.Tensor, invK_b44: torch.Tensor) -> torch.Tensor:
        _lib.require_cuda_f32(depth_b1hw, invK_b44)
        if tuple(depth_b1hw.shape[-2:]) != (self.height, self.width):
            raise _lib.IdhError(f"depth {tuple(depth_b1hw.shape)} must be (B,1,{self.height},{self.width})")
        return depth_normals(depth_b1hw, invK_b44, kernel_size=self.kernel_size, std=self.std)[0]


def _src_mats(name, t, B, K):
    _lib.require_cuda_f32(t)
    if tuple(t.shape) != (B, K, 4, 4):
        raise _lib.IdhError(f"{name} {tuple(t.shape)} must be ({B},{K},4,4)")
    return t.contiguous()


def depth_consistency(depth_b1hw: torch.Tensor, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor, src_depth_bk1hw: torch.Tensor,
                      src_K_bk44: torch.Tensor, src_cam_T_world_bk44: torch.Tensor, *, gate_depth: Optional[torch.Tensor] = None,
                      ratio: float = 1.05, log_tol: float = 0.05, min_consistent: int = 1, max_conflict: int = 0,
                      return_per_source: bool = False, return_loss: bool = False) -> dict:
    """Check a depth map (B,1,h,w) against K source depth maps (B,K,1,h,w) of other cameras, in one launch (idh_mv_consistency_fwd;
    contract: include/idh_geometry.h).  Every pixel is back-projected with ``invK_b44`` and ``world_T_cam_b44``,
    projected into each source with ``src_K_bk44 @ src_cam_T_world_bk44`` and compared with the nearest tap of that source's depth - the
    arithmetic of the reference's ``MVDepthLoss`` (losses.py:143-261).  A source *sees* the point when the point is not behind the
    source's surface by more than ``ratio``; it is *consistent* when the two depths agree within ``log_tol`` in log space, and in
    *conflict* when the point lies in front of the source's surface by more than that - in space the source saw through.  Returns

    * ``"counts"`` (B,3,h,w) uint8: the number of sources that see / are consistent with / conflict with the pixel;
    * ``"weight"`` (B,1,h,w): ``1 + consistent`` where the pixel is kept - its depth finite and positive, ``consistent >= min_consistent``
      and ``conflict <= max_conflict`` - else 0: what ``fusion.integrate_depth(weight_m1hw=)`` takes;
    * ``"filtered_depth"`` (B,1,h,w): the depth where kept, 0 (a hole) elsewhere;
    * with ``return_per_source`` ``"visible"`` (B,K,h,w) uint8 and ``"err"`` (B,K,h,w), ``|log sampled - log projected|``, NaN where
      not visible;
    * with ``return_loss`` ``"loss"`` (a 0-d tensor): the forward value of the reference's ``MVDepthLoss`` - NaN when a source sees no
      pixel - and ``"loss_sum"`` (K,) float64, ``"loss_count"`` (K,) int64 behind it.  Deterministic: two calls return the same bits.

    ``gate_depth`` (B,1,h,w): the map visibility is computed from (the reference's ``cur_depth_b1hw``); None: the tested map itself.
    Sources must have the tested map's size; 1 <= K <= 16, B <= 128.  There is no CPU fallback and no backward pass."""
    _lib.require_cuda_f32(depth_b1hw, invK_b44, world_T_cam_b44, src_depth_bk1hw, gate_depth)
    if depth_b1hw.dim() != 4 or depth_b1hw.shape[1] != 1:
        raise _lib.IdhError(f"depth {tuple(depth_b1hw.shape)} must be (B,1,h,w)")
    B, _, h, w = depth_b1hw.shape
    if src_depth_bk1hw.dim() != 5 or src_depth_bk1hw.shape[0] != B or src_depth_bk1hw.shape[2] != 1:
        raise _lib.IdhError(f"src_depth {tuple(src_depth_bk1hw.shape)} must be ({B},K,1,h,w)")
    K, (sh, sw) = int(src_depth_bk1hw.shape[1]), (int(s) for s in src_depth_bk1hw.shape[3:])
    if tuple(invK_b44.shape) != (B, 4, 4) or tuple(world_T_cam_b44.shape) != (B, 4, 4):
        raise _lib.IdhError(f"invK {tuple(invK_b44.shape)} and world_T_cam {tuple(world_T_cam_b44.shape)} must be ({B},4,4)")
    if gate_depth is not None and gate_depth.shape != depth_b1hw.shape:
        raise _lib.IdhError(f"gate_depth {tuple(gate_depth.shape)} must be {tuple(depth_b1hw.shape)}")
    dev = depth_b1hw.device
    keep = [depth_b1hw.contiguous(), invK_b44.contiguous(), world_T_cam_b44.contiguous(), src_depth_bk1hw.contiguous(),
            _src_mats("src_K", src_K_bk44, B, K), _src_mats("src_cam_T_world", src_cam_T_world_bk44, B, K)]
    a = _lib.MvConsistencyArgs()
    a.depth_b1hw, a.invK_b44, a.world_T_cam_b44, a.src_depth_bk1hw, a.src_K_bk44, a.src_cam_T_world_bk44 = (t.data_ptr() for t in keep)
    if gate_depth is not None:
        keep.append(gate_depth.contiguous())
        a.gate_depth_b1hw = keep[-1].data_ptr()
    out = {"counts": torch.empty(B, 3, h, w, device=dev, dtype=torch.uint8), "weight": torch.empty(B, 1, h, w, device=dev),
           "filtered_depth": torch.empty(B, 1, h, w, device=dev)}
    a.counts_b3hw, a.weight_b1hw, a.filtered_depth_b1hw = out["counts"].data_ptr(), out["weight"].data_ptr(), out["filtered_depth"].data_ptr()
    if return_per_source:
        out["visible"] = torch.empty(B, K, h, w, device=dev, dtype=torch.uint8)
        out["err"] = torch.empty(B, K, h, w, device=dev)
        a.visible_bkhw, a.err_bkhw = out["visible"].data_ptr(), out["err"].data_ptr()
    if return_loss:
        out["loss"] = torch.full((), float("nan"), device=dev)
        out["loss_sum"] = torch.zeros(K, device=dev, dtype=torch.float64)
        out["loss_count"] = torch.zeros(K, device=dev, dtype=torch.int64)
        nbytes = _lib.lib().idh_mv_consistency_workspace_bytes(B, K, h, w)
        workspace = torch.empty(max(nbytes, 8) // 8, device=dev, dtype=torch.float64)
        keep.append(workspace)
        a.loss, a.loss_sum_k, a.loss_count_k = out["loss"].data_ptr(), out["loss_sum"].data_ptr(), out["loss_count"].data_ptr()
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * 8
    a.ratio, a.log_tol, a.min_consistent, a.max_conflict = float(ratio), float(log_tol), int(min_consistent), int(max_conflict)
    a.B, a.K, a.h, a.w, a.src_h, a.src_w = B, K, h, w, sh, sw
    if B == 0:
        return out
    _lib.check(_lib.lib().idh_mv_consistency_fwd(a, _lib.stream_ptr()), "idh_mv_consistency_fwd")
    return out


class MVDepthLoss(nn.Module):
    """The forward value of the reference's ``MVDepthLoss`` (losses.py:143-261) - same constructor, same ``forward`` signature - on the
    fused kernel of ``depth_consistency``: one launch and a small finalise launch instead of K rounds of back-projection, projection,
    ``grid_sample`` and ``nanmean``.  A score of a predicted depth map against its source views that needs no ground truth.
    Forward only: there is no backward pass, and an input that requires grad raises ``IdhError`` instead of returning a value that
    silently carries no gradient."""

    def __init__(self, height: int, width: int):
        super().__init__()
        self.height, self.width = int(height), int(width)
        self.backproject = BackprojectDepth(self.height, self.width)
        self.project = Project3D()

    def forward(self, depth_pred_b1hw, cur_depth_b1hw, src_depth_bk1hw, cur_invK_b44, src_K_bk44, cur_world_T_cam_b44, src_cam_T_world_bk44):
        tensors = (depth_pred_b1hw, cur_depth_b1hw, src_depth_bk1hw, cur_invK_b44, src_K_bk44, cur_world_T_cam_b44, src_cam_T_world_bk44)
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            raise _lib.IdhError("MVDepthLoss is forward only (no backward pass): detach the inputs or call it under torch.no_grad()")
        if tuple(cur_depth_b1hw.shape[-2:]) != (self.height, self.width):
            raise _lib.IdhError(f"depth {tuple(cur_depth_b1hw.shape)} must be (B,1,{self.height},{self.width})")
        return depth_consistency(depth_pred_b1hw, cur_invK_b44, cur_world_T_cam_b44, src_depth_bk1hw, src_K_bk44, src_cam_T_world_bk44,
                                 gate_depth=cur_depth_b1hw, return_loss=True)["loss"]


def edge_mask(depth_b1hw: torch.Tensor, threshold: float = 0.95, dilate: bool = True, *, as_bool: bool = False, return_sobel: bool = False,
              return_threshold: bool = False):
    """The reference's ``get_edge_mask(depth_b1hw, threshold=0.95, dilate=True)`` (utils/generic_utils.py:286-292) on the gfx950 kernels
    (idh_edge_mask_fwd; contract: include/idh_geometry.h): the Sobel magnitude ``S`` of the disparity ``1 / depth``, per
    image the exact ``torch.nanquantile(S, threshold)`` by a radix select, ``S > quantile`` and - with ``dilate`` - the 5x5 max-pool.
    Returns the mask (B,1,H,W) as float 0 / 1, or as bool with ``as_bool``.  ``edge_mask(depth_1hw, 0.975, False, as_bool=True)`` on a
    (1,H,W) map is the dataset's variant (datasets/generic_mvs_dataset.py:650-658); a 3-D input returns a 3-D mask.
    ``return_sobel`` / ``return_threshold`` append ``S`` (the input's shape) / the per-image thresholds (B,) to the result, which is then
    a tuple.  Deterministic: two calls return the same bits.  There is no CPU fallback, no backward pass, and nothing is synchronised."""
    _lib.require_cuda_f32(depth_b1hw)
    squeeze = depth_b1hw.dim() == 3
    d = depth_b1hw.unsqueeze(0) if squeeze else depth_b1hw
    if d.dim() != 4 or d.shape[1] != 1:
        raise _lib.IdhError(f"depth {tuple(depth_b1hw.shape)} must be (B,1,H,W) or (1,H,W)")
    q = float(threshold)
    if not 0.0 <= q <= 1.0:
        raise _lib.IdhError(f"threshold must be a quantile in [0, 1], got {threshold}")
    B, _, H, W = d.shape
    if H < 1 or W < 1:
        raise _lib.IdhError(f"depth {tuple(depth_b1hw.shape)} has no pixels")
    d = d.contiguous()
    dev = d.device
    mask = torch.empty(B, 1, H, W, device=dev, dtype=torch.uint8 if as_bool else torch.float32)
    sobel = torch.empty(B, 1, H, W, device=dev) if return_sobel else None
    thr = torch.empty(B, device=dev) if return_threshold else None
    if B > 0:
        nbytes = _lib.lib().idh_edge_mask_workspace_bytes(B, H, W)
        workspace = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
        a = _lib.EdgeMaskArgs()
        a.depth_b1hw, a.mask_b1hw, a.sobel_b1hw, a.threshold_b = d.data_ptr(), mask.data_ptr(), _lib.ptr(sobel), _lib.ptr(thr)
        a.workspace, a.workspace_bytes = workspace.data_ptr(), nbytes
        a.q, a.dilate, a.mask_u8, a.B, a.H, a.W = q, int(bool(dilate)), int(bool(as_bool)), B, H, W
        _lib.check(_lib.lib().idh_edge_mask_fwd(a, _lib.stream_ptr()), "idh_edge_mask_fwd")
    if as_bool:
        mask = mask.view(torch.bool)
    if squeeze:
        mask, sobel = mask[0], None if sobel is None else sobel[0]
    extra = tuple(t for t in (sobel, thr) if t is not None)
    return (mask, *extra) if extra else mask
