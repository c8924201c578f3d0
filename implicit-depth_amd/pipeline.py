"""The hot path of ``BDModel.forward`` / ``DepthModel.forward`` as one NHWC pipeline.

Covers reference experiment_modules/bd_model.py:231-311 (and depth_model.py:378-433) from
the matching features onwards:

    [matching backbone layer1 map --> encoder head (1x1 conv, InstanceNorm, LeakyReLU, 3x3 conv, InstanceNorm)]
    matching feats (NHWC) --> fused warp+match (cost volume, NHWC out)
        --> CVEncoder --> UNet++ decoder --> per-pixel occlusion MLP over all query planes
                                         \\-> (DepthModel) 1x1 log-depth heads, exp

Everything between the NCHW inputs and the NCHW outputs stays channels-last in HBM; the only
layout conversions are the imports of the caller's NCHW tensors.  The module-level drop-ins
in cost_volume.py / networks.py do the same work one module at a time (with a conversion at
every module boundary) for callers that only swap attributes.

The image encoder (timm EfficientNetV2-S) and the ResNet18 stem of the matching encoder are
third-party code that is neither in the reference tree nor in scope: their
outputs are inputs of this pipeline.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _lib, nhwc
from .cost_volume import CostVolumeManager, ZeroCostVolumeManager, volume_opts
from .mlp import occlusion_logits


MAX_RING_CAPACITY = 16  # idh_binary_mlp_view_keys_fwd asks at most 16 keys


class PredictionRing:
    """The last ``capacity`` predictions a caller chose to remember, for the multi-key queries (``mlp.view_keys_logits`` /
    ``view_keys_depths``): a dense (capacity,B,H,W,Cf) ring of scale-0 decoder features, their cameras (capacity,B,4,4) and - once a
    prediction is pushed with one - a prior ring (capacity,B,1,H,W) with its cameras.  Storage is allocated on the first ``push``.  A
    prediction pushed without a prior into a ring that has one holds the constant -1 there, which is what a prior-enabled network
    sees where no prior prediction exists (reference bd_model.py:433-434)."""

    def __init__(self, capacity: int = 4):
        capacity = int(capacity)
        if not 1 <= capacity <= MAX_RING_CAPACITY:
            raise _lib.IdhError(f"ring capacity must be in [1, {MAX_RING_CAPACITY}], got {capacity}")
        self.capacity = capacity
        self.feat = self.cam_T_world = self.K = self.prior = self.prior_cam_T_world = self.prior_K = None
        self._next, self._count = 0, 0

    def __len__(self) -> int:
        return self._count

    @property
    def B(self) -> Optional[int]:
        return None if self.feat is None else self.feat.shape[1]

    def clear(self) -> None:
        """Forget every prediction; the storage is kept."""
        self._next, self._count = 0, 0

    def push(self, final0_view: nhwc.View, cam_T_world_b44: torch.Tensor, K_s0_b44: torch.Tensor, prior=None) -> int:
        """Copy the scale-0 ``View`` of a forward - one strided device copy on the current stream, so it is ordered before any later
        replay of the plan that owns the view - and its camera into the next slot (the oldest once the ring is full); ``prior``: None or
        (prior_pred (B,1,H,W), prior_cam_T_world (B,4,4), prior_K (B,4,4)).  Returns the slot."""
        v = final0_view
        B, H, W, C = v.N, v.H, v.W, v.C
        _lib.require_cuda_f32(v.buf, cam_T_world_b44, K_s0_b44, *(prior if prior is not None else ()))
        for m in (cam_T_world_b44, K_s0_b44) + (tuple(prior[1:]) if prior is not None else ()):
            if tuple(m.shape) != (B, 4, 4):
                raise _lib.IdhError(f"cam_T_world / K_s0 (and the prior's) must be ({B}, 4, 4), got {tuple(m.shape)}")
        if prior is not None and tuple(prior[0].shape) != (B, 1, H, W):
            raise _lib.IdhError(f"prior prediction {tuple(prior[0].shape)} must be ({B}, 1, {H}, {W})")
        dev = v.buf.device
        if self.feat is None or tuple(self.feat.shape[1:]) != (B, H, W, C) or self.feat.device != dev:
            self.feat = torch.empty(self.capacity, B, H, W, C, device=dev)
            self.cam_T_world, self.K = torch.empty(self.capacity, B, 4, 4, device=dev), torch.empty(self.capacity, B, 4, 4, device=dev)
            self.prior = self.prior_cam_T_world = self.prior_K = None
            self.clear()
        if prior is not None and self.prior is None:
            self.prior = torch.full((self.capacity, B, 1, H, W), -1.0, device=dev)
            self.prior_cam_T_world, self.prior_K = self.cam_T_world.clone(), self.K.clone()
        slot = self._next
        self.feat[slot].copy_(v.dense())
        self.cam_T_world[slot].copy_(cam_T_world_b44)
        self.K[slot].copy_(K_s0_b44)
        if self.prior is not None:
            if prior is not None:
                self.prior[slot].copy_(prior[0])
                self.prior_cam_T_world[slot].copy_(prior[1])
                self.prior_K[slot].copy_(prior[2])
            else:
                self.prior[slot].fill_(-1.0)
                self.prior_cam_T_world[slot].copy_(cam_T_world_b44)
                self.prior_K[slot].copy_(K_s0_b44)
        self._next = (slot + 1) % self.capacity
        self._count = min(self._count + 1, self.capacity)
        return slot

    def slots_newest_first(self) -> List[int]:
        return [(self._next - 1 - i) % self.capacity for i in range(self._count)]

    def prior_rings(self):
        return None if self.prior is None else (self.prior, self.prior_cam_T_world, self.prior_K)


class HotPath(nn.Module):
    """Owns (or shares) the hot-path modules of a BDModel / DepthModel: the cost volume, the CVEncoder, the
    depth decoder, the occlusion MLP and — optionally — the matching encoder, whose head then runs inside the
    same plan and hands its features to the volume kernel channels-last without a copy."""

    def __init__(self, cost_volume: nn.Module, cost_volume_net: nn.Module, depth_decoder: nn.Module,
                 binary_mlp: Optional[nn.Module] = None, min_depth: float = 0.25, max_depth: float = 5.0,
                 conv_math: Optional[str] = None, matching_model: Optional[nn.Module] = None):
        super().__init__()
        self.conv_math = conv_math  # None = nhwc.DEFAULT_MATH ("fp32"); "f16x3": see nhwc.MATH_MODES
        self.cost_volume = cost_volume
        self.cost_volume_net = cost_volume_net
        self.depth_decoder = depth_decoder
        self.binary_mlp = binary_mlp
        self.matching_model = matching_model  # ResnetMatchingEncoder (drop-in or reference): its net[5:] head runs here
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self.thresholder = None  # like BDModel.thresholder (bd_model.py:141): per-depth thresholds of the infer_depth search
        self._plans = nhwc.PlanCache()  # LRU: a ragged last batch / alternating shapes replay instead of rebuilding
        self._last = None  # decoder output of the last forward (plan-owned final[i] views): what query_rays / query_points / query_view read
        self._ring: Optional[PredictionRing] = None  # predictions kept by remember(): what query_view_keys / query_view_depths_keys read
        _lib.watch_state_dict_loads(self)

    # ------------------------------------------------------------------------------------
    def _scales(self, return_features: bool, query_scales: Sequence[int] = ()) -> int:
        """The decoder scales a call reads (nhwc.build_decoder): the occlusion MLP takes scale 0 only, so a BDDecoderPP behind it builds
        output_1..3 just for the callers that ask for the feature maps or for ray queries at those scales; depth / regression heads are
        outputs at every scale."""
        dec = self.depth_decoder
        if return_features or any(s != 0 for s in query_scales) or self.binary_mlp is None or getattr(dec, "depth_head", False) or hasattr(dec, "out1"):
            return nhwc.ALL_SCALES
        return 0b0001

    @staticmethod
    def _check_query_scales(scales) -> tuple:
        scales = tuple(int(s) for s in scales)
        if not scales or any(s not in (0, 1, 2, 3) for s in scales):
            raise _lib.IdhError(f"query_scales must be a non-empty subset of (0, 1, 2, 3), got {scales}")
        return scales

    def query_rays(self, rays: torch.Tensor, depths: torch.Tensor, prior=None, grid: Optional[Sequence[int]] = None,
                   scales: Sequence[int] = (0,)) -> Dict[str, torch.Tensor]:
        """Occlusion logits at sparse rays against the decoder output of the LAST ``forward`` on this HotPath (the plan-owned buffers stay
        valid until that plan is replayed): no conv runs, one ``mlp.ray_logits`` launch per scale.  ``rays`` (B,N,2) in pixel-centre units
        of ``grid`` = (h, w) (None: the scale-0 map's own shape), ``depths`` (B,N,S), ``prior`` None | float | (B,N,S).  Scale s takes every
        (s+1)-th ray, as the reference's run_mlp_train (bd_model.py:352-353).  Returns {"ray_pred_{s}": (B,1,ceil(N/(s+1)),S)}.
        ``IdhError`` when no forward has run, when B differs, or when that forward did not build a requested scale."""
        from .mlp import ray_logits

        scales = self._check_query_scales(scales)
        final = _last_final(self, rays.shape[0], scales)
        _lib.require_cuda_f32(rays, depths, prior if isinstance(prior, torch.Tensor) else None)
        if grid is None:
            grid = (final[0].H, final[0].W)
        return {f"ray_pred_{s}": ray_logits(self.binary_mlp, final[s], rays, depths, prior, scale=s, grid=grid, ray_step=s + 1) for s in scales}

    def query_ray_depths(self, rays: torch.Tensor, prior=None, grid: Optional[Sequence[int]] = None, thresholder=None,
                         invK_s0_b44: Optional[torch.Tensor] = None, world_T_cam_b44: Optional[torch.Tensor] = None, iters: int = 12,
                         lo: float = 0.5, hi: float = 8.0, threshold: float = 0.5) -> Dict[str, torch.Tensor]:
        """Where sparse rays hit the scene, against the scale-0 decoder output of the LAST ``forward`` (valid as for ``query_rays``): the
        ``infer_depth`` search (bd_model.py:273-292) per ray in one ``mlp.ray_depths`` launch, no conv runs.  ``rays`` (B,N,2) in
        pixel-centre units of ``grid`` = (h, w) (None: the scale-0 map's own shape); ``prior`` None | float | (B,N); ``thresholder``: None =
        this HotPath's ``thresholder`` (None there: the constant ``threshold``).  ``invK_s0_b44`` (B,4,4), the inverse intrinsics at the
        resolution of ``grid``, adds the hit points; ``world_T_cam_b44`` takes them to the world.  Returns {"ray_depth" (B,N), "ray_pred"
        (B,N) logits of the last evaluation, "ray_hit" (B,N) uint8 (3 = bracketed inside [lo, hi]; 1 / 2 = ran into lo / hi), "ray_points"
        (B,N,3) | None}."""
        from .mlp import ray_depths

        final = _last_final(self, rays.shape[0], (0,))
        depth, pred, hit, points = ray_depths(self.binary_mlp, final[0], rays, prior, grid, iters, lo, hi, threshold,
                                              self.thresholder if thresholder is None else thresholder, invK_s0_b44, world_T_cam_b44)
        return {"ray_depth": depth, "ray_pred": pred, "ray_hit": hit, "ray_points": points}

    def query_points(self, points_bn3: torch.Tensor, cam_T_world_b44: torch.Tensor, K_s0_b44: torch.Tensor,
                     prior_inputs: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """Occlusion of world points (B,N,3) against the LAST forward: each point is projected into the scale-0 map with ``K_s0_b44`` /
        ``cam_T_world_b44`` (``mlp.project_points``) and asked at its own depth along its ray.  ``prior_inputs``: {"prior_prediction"
        (B,1,H/2,W/2), "prior_cam_T_world" (B,4,4)} (and optionally the prior view's own "K_s0_b44") - the point is projected into that
        camera and the prediction sampled there (nearest, -1 outside), as BDModel.sample_prior does per pixel.  Returns {"point_pred"
        (B,1,N,1) logits, "point_valid" (B,N) bool: in front of the camera and inside the image, "point_depth" (B,N), "point_rays" (B,N,2)}."""
        from .mlp import project_points, ray_logits

        final = _last_final(self, points_bn3.shape[0], (0,))
        _lib.require_cuda_f32(points_bn3, cam_T_world_b44, K_s0_b44)
        f0 = final[0]
        pp = pc = pk = None
        if prior_inputs is not None and prior_inputs.get("prior_prediction") is not None:
            pp, pc, pk = prior_inputs["prior_prediction"], prior_inputs["prior_cam_T_world"], prior_inputs.get("K_s0_b44", K_s0_b44)
        rays, depth, valid, prior = project_points(points_bn3, cam_T_world_b44, K_s0_b44, f0.H, f0.W, pp, pc, pk)
        pred = ray_logits(self.binary_mlp, f0, rays, depth.unsqueeze(-1), None if prior is None else prior.unsqueeze(-1), scale=0)
        return {"point_pred": pred, "point_valid": valid, "point_depth": depth, "point_rays": rays}

    def query_view(self, rendered_depth: torch.Tensor, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor, cam_T_world_b44: torch.Tensor,
                   K_s0_b44: torch.Tensor, prior_inputs: Optional[Dict[str, torch.Tensor]] = None, fill: float = 0.0,
                   return_points: bool = False) -> Dict[str, Optional[torch.Tensor]]:
        """Dense occlusion of an asset seen from ANOTHER camera against the LAST forward (valid as for ``query_rays``): ``rendered_depth``
        (B,P,h,w) is the asset's depth in the view of ``invK_b44`` (at h x w) / ``world_T_cam_b44``; every pixel is back-projected, projected
        into the scale-0 map with ``K_s0_b44`` / ``cam_T_world_b44`` - the camera of that forward - and asked at its own depth there, in
        one ``mlp.view_logits`` launch.  The same answers as ``query_points`` on the back-projected pixels, bit for bit.  ``prior_inputs`` as
        ``query_points``.  Returns {"view_pred" (B,P,h,w) logits, ``fill`` where "view_valid" (B,P,h,w) bool is False (no finite positive
        depth, behind the camera or outside its image), "view_depth" (B,P,h,w): depth in the forward's camera, "view_points" (B,P,h,w,3)
        world points with ``return_points``, else None}."""
        from .mlp import view_logits

        final = _last_final(self, rendered_depth.shape[0], (0,))
        _lib.require_cuda_f32(rendered_depth, invK_b44, world_T_cam_b44, cam_T_world_b44, K_s0_b44)
        prior = None
        if prior_inputs is not None and prior_inputs.get("prior_prediction") is not None:
            prior = (prior_inputs["prior_prediction"], prior_inputs["prior_cam_T_world"], prior_inputs.get("K_s0_b44", K_s0_b44))
        pred, valid, depth, points = view_logits(self.binary_mlp, final[0], rendered_depth, invK_b44, world_T_cam_b44, cam_T_world_b44, K_s0_b44,
                                                 prior, fill, return_points)
        return {"view_pred": pred, "view_valid": valid, "view_depth": depth, "view_points": points}

    def query_view_depths(self, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor, cam_T_world_b44: torch.Tensor, K_s0_b44: torch.Tensor,
                          size: Optional[Sequence[int]] = None, rays: Optional[torch.Tensor] = None,
                          prior_inputs: Optional[Dict[str, torch.Tensor]] = None, thresholder=None, iters: int = 12, lo: float = 0.5,
                          hi: float = 8.0, threshold: float = 0.5, fill: float = 0.0, return_points: bool = False) -> Dict[str, Optional[torch.Tensor]]:
        """Depth seen from ANOTHER camera against the LAST forward (valid as for ``query_rays``): the ``infer_depth`` search (bd_model.py:273-292)
        along the rays of the view of ``invK_b44`` / ``world_T_cam_b44`` - every pixel centre of ``size`` = (h, w), or ``rays`` (B,N,2) in
        pixel-centre units of that view (exactly one of the two) - with every probe projected into the scale-0 map through ``K_s0_b44`` /
        ``cam_T_world_b44``, the camera of that forward, as ``query_view`` does, in one ``mlp.view_depths`` launch.  The query is the
        z-depth in the VIEW; the threshold of a step is looked up at the probe's depth in the forward's camera.  ``prior_inputs`` as
        ``query_points`` (the map is sampled per probe); ``thresholder``: None = this HotPath's ``thresholder`` (None there: the constant
        ``threshold``).  A probe outside the forward's image or behind its camera has the logit ``fill``.  Returns {"view_search_depths"
        (B,1,h,w) | (B,N), "view_search_logits": logits of the last step, "view_search_flags" uint8 (bit 0 / 1: the far / near bound
        moved, 3 = bracketed inside [lo, hi]; bit 2: some probe was invalid), "view_search_points" (...,3) world points with
        ``return_points``, else None}.  The occlusion is the one seen from the forward's camera: the depth is where the view's ray
        enters the region hidden from THAT camera."""
        from .mlp import view_depths

        if (size is None) == (rays is None):
            raise _lib.IdhError("query_view_depths takes exactly one of size=(h, w) and rays=(B,N,2)")
        final = _last_final(self, invK_b44.shape[0], (0,))
        _lib.require_cuda_f32(invK_b44, world_T_cam_b44, cam_T_world_b44, K_s0_b44, rays)
        prior = None
        if prior_inputs is not None and prior_inputs.get("prior_prediction") is not None:
            prior = (prior_inputs["prior_prediction"], prior_inputs["prior_cam_T_world"], prior_inputs.get("K_s0_b44", K_s0_b44))
        depth, pred, flags, points = view_depths(self.binary_mlp, final[0], invK_b44, world_T_cam_b44, cam_T_world_b44, K_s0_b44, size, rays, prior,
                                                 iters, lo, hi, threshold, self.thresholder if thresholder is None else thresholder, fill,
                                                 return_points)
        return {"view_search_depths": depth, "view_search_logits": pred, "view_search_flags": flags, "view_search_points": points}

    def remember(self, cam_T_world_b44: torch.Tensor, K_s0_b44: torch.Tensor, prior_inputs: Optional[Dict[str, torch.Tensor]] = None,
                 capacity: int = 4) -> int:
        """Keep the LAST forward for the multi-key queries: its scale-0 decoder features are copied - on the current stream, before the
        plan can be replayed - into a ``PredictionRing`` of ``capacity`` (<= 16) predictions together with the camera of that forward
        (``cam_T_world_b44``, ``K_s0_b44``) and, with ``prior_inputs`` as ``query_points``, the prior that belongs to it.  The oldest
        prediction leaves once the ring is full; another ``capacity`` or batch size starts a new ring.  Returns the slot."""
        final = _last_final(self, cam_T_world_b44.shape[0], (0,))
        if self._ring is None or self._ring.capacity != int(capacity):
            self._ring = PredictionRing(capacity)
        prior = None
        if prior_inputs is not None and prior_inputs.get("prior_prediction") is not None:
            prior = (prior_inputs["prior_prediction"], prior_inputs["prior_cam_T_world"], prior_inputs.get("K_s0_b44", K_s0_b44))
        return self._ring.push(final[0], cam_T_world_b44, K_s0_b44, prior)

    def forget(self) -> None:
        """Empty the ring of remembered predictions (its storage is kept)."""
        if self._ring is not None:
            self._ring.clear()

    def _remembered(self, B: int, order):
        if self.binary_mlp is None:
            raise _lib.IdhError("occlusion queries need a HotPath with a binary_mlp")
        ring = self._ring
        if ring is None or len(ring) == 0:
            raise _lib.IdhError("nothing is remembered on this HotPath yet: call remember() after a forward")
        if ring.B != B:
            raise _lib.IdhError(f"the remembered predictions have batch size {ring.B}, the query has {B}")
        live = ring.slots_newest_first()
        slots = live if order is None else [int(s) for s in order]
        if any(s not in live for s in slots):
            raise _lib.IdhError(f"order {slots} names a slot that holds no prediction (remembered: {live})")
        prior = ring.prior_rings() if getattr(self.binary_mlp, "use_prior", False) else None
        return ring, slots, prior

    def query_view_keys(self, rendered_depth: torch.Tensor, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor,
                        order: Optional[Sequence[int]] = None, fill: float = 0.0, return_points: bool = False) -> Dict[str, Optional[torch.Tensor]]:
        """``query_view`` against the predictions kept by ``remember``: every pixel is asked in the first remembered prediction - in
        ``order``, a list of ring slots; None = newest first - whose camera sees it, in one ``mlp.view_keys_logits`` launch with one MLP
        pass per pixel.  The answers are those of ``query_view`` on that prediction, bit for bit; the prior is the one remembered with it.
        Returns ``query_view``'s dictionary - "view_depth" is the depth in the selected prediction's camera - plus "view_key" (B,P,h,w)
        uint8: the position in the order of the prediction that answered, 255 where none did ("view_valid" False, "view_pred" ``fill``).
        ``IdhError`` when nothing is remembered or when B differs."""
        from .mlp import view_keys_logits

        ring, slots, prior = self._remembered(rendered_depth.shape[0], order)
        pred, key, depth, points = view_keys_logits(self.binary_mlp, ring.feat, 0, ring.feat.shape[-1], slots, rendered_depth, invK_b44,
                                                    world_T_cam_b44, ring.cam_T_world, ring.K, prior, fill, return_points)
        return {"view_pred": pred, "view_valid": key != 255, "view_depth": depth, "view_points": points, "view_key": key}

    def query_view_depths_keys(self, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor, size: Optional[Sequence[int]] = None,
                               rays: Optional[torch.Tensor] = None, order: Optional[Sequence[int]] = None, thresholder=None, iters: int = 12,
                               lo: float = 0.5, hi: float = 8.0, threshold: float = 0.5, fill: float = 0.0,
                               return_points: bool = False) -> Dict[str, Optional[torch.Tensor]]:
        """``query_view_depths`` against the predictions kept by ``remember``: the same search, every probe asked in the first remembered
        prediction (``order`` as ``query_view_keys``) whose camera sees it, in one ``mlp.view_keys_depths`` launch.  Returns
        ``query_view_depths``' dictionary - flag bit 2: no prediction saw some probe - plus "view_search_key": the position in the order
        of the prediction the LAST step asked, 255 = none.  ``IdhError`` when nothing is remembered or when B differs."""
        from .mlp import view_keys_depths

        if (size is None) == (rays is None):
            raise _lib.IdhError("query_view_depths_keys takes exactly one of size=(h, w) and rays=(B,N,2)")
        ring, slots, prior = self._remembered(invK_b44.shape[0], order)
        depth, pred, flags, points, key = view_keys_depths(self.binary_mlp, ring.feat, 0, ring.feat.shape[-1], slots, invK_b44, world_T_cam_b44,
                                                           ring.cam_T_world, ring.K, size, rays, prior, iters, lo, hi, threshold,
                                                           self.thresholder if thresholder is None else thresholder, fill, return_points)
        return {"view_search_depths": depth, "view_search_logits": pred, "view_search_flags": flags, "view_search_points": points,
                "view_search_key": key}

    def query_view_first_hit(self, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor, cam_T_world_b44: torch.Tensor, K_s0_b44: torch.Tensor,
                             size: Optional[Sequence[int]] = None, rays: Optional[torch.Tensor] = None,
                             prior_inputs: Optional[Dict[str, torch.Tensor]] = None, thresholder=None, samples=16, lo: float = 0.5,
                             hi: float = 8.0, spacing: str = "linear", refine: int = 8, threshold: float = 0.5, fill: float = 0.0,
                             return_points: bool = False) -> Dict[str, Optional[torch.Tensor]]:
        """FIRST depth along the rays of ANOTHER camera at which the probe is behind the surface, against the LAST forward (valid as for
        ``query_rays``): where ``query_view_depths`` bisects [lo, hi] and so assumes one crossing, every ray here probes the shared depths
        ``samples`` (a float32 vector, or n with ``lo`` / ``hi`` / ``spacing``; ``mlp.march_samples``) in turn until its first hit and then
        bisects ``refine`` steps inside the bracket, in one ``mlp.view_march_depths`` launch.  The other arguments as ``query_view_depths``.
        Returns {"view_march_depths" (B,1,h,w) | (B,N), "view_march_logits": logits of each ray's last probe, "view_march_flags" uint8
        (3 = bracketed; 1 = behind at the first sample; 2 = no hit, the depth is the last sample; bit 2: some evaluated probe was invalid),
        "view_march_hit_step" uint8: the first sample that was behind, 255 = none, "view_march_points" (...,3) world points with
        ``return_points``, else None}."""
        from .mlp import view_march_depths

        if (size is None) == (rays is None):
            raise _lib.IdhError("query_view_first_hit takes exactly one of size=(h, w) and rays=(B,N,2)")
        final = _last_final(self, invK_b44.shape[0], (0,))
        _lib.require_cuda_f32(invK_b44, world_T_cam_b44, cam_T_world_b44, K_s0_b44, rays)
        prior = None
        if prior_inputs is not None and prior_inputs.get("prior_prediction") is not None:
            prior = (prior_inputs["prior_prediction"], prior_inputs["prior_cam_T_world"], prior_inputs.get("K_s0_b44", K_s0_b44))
        depth, pred, flags, step, points = view_march_depths(self.binary_mlp, final[0], invK_b44, world_T_cam_b44, cam_T_world_b44, K_s0_b44, size,
                                                             rays, prior, samples, lo, hi, spacing, refine, threshold,
                                                             self.thresholder if thresholder is None else thresholder, fill, return_points)
        return {"view_march_depths": depth, "view_march_logits": pred, "view_march_flags": flags, "view_march_hit_step": step,
                "view_march_points": points}

    def query_view_first_hit_keys(self, invK_b44: torch.Tensor, world_T_cam_b44: torch.Tensor, size: Optional[Sequence[int]] = None,
                                  rays: Optional[torch.Tensor] = None, order: Optional[Sequence[int]] = None, thresholder=None, samples=16,
                                  lo: float = 0.5, hi: float = 8.0, spacing: str = "linear", refine: int = 8, threshold: float = 0.5,
                                  fill: float = 0.0, return_points: bool = False) -> Dict[str, Optional[torch.Tensor]]:
        """``query_view_first_hit`` against the predictions kept by ``remember``: the same march, every probe asked in the first remembered
        prediction (``order`` as ``query_view_keys``) whose camera sees it, in one ``mlp.view_keys_march_depths`` launch.  Returns
        ``query_view_first_hit``'s dictionary - flag bit 2: no prediction saw some evaluated probe - plus "view_march_key": the position in
        the order of the prediction the ray's LAST probe asked, 255 = none.  ``IdhError`` when nothing is remembered or when B differs."""
        from .mlp import view_keys_march_depths

        if (size is None) == (rays is None):
            raise _lib.IdhError("query_view_first_hit_keys takes exactly one of size=(h, w) and rays=(B,N,2)")
        ring, slots, prior = self._remembered(invK_b44.shape[0], order)
        depth, pred, flags, step, points, key = view_keys_march_depths(self.binary_mlp, ring.feat, 0, ring.feat.shape[-1], slots, invK_b44,
                                                                       world_T_cam_b44, ring.cam_T_world, ring.K, size, rays, prior, samples, lo, hi,
                                                                       spacing, refine, threshold,
                                                                       self.thresholder if thresholder is None else thresholder, fill, return_points)
        return {"view_march_depths": depth, "view_march_logits": pred, "view_march_flags": flags, "view_march_hit_step": step,
                "view_march_points": points, "view_march_key": key}

    def _plan(self, B, K, C, H, W, enc_shapes: Sequence[Sequence[int]], device, head: Optional[str] = None, head_ch: int = 0,
              images: Optional[torch.Tensor] = None, scales: int = nhwc.ALL_SCALES):
        """``scales``: bit i = the plan builds the decoder's output_i result (part of the plan key: the full plan is built on first demand).
        ``head``: None = matching features come in finished (NCHW); "nchw" / "nhwc" = the plan starts at the
        matching backbone's layer1 map (B*(K+1), head_ch, H, W) in that physical layout and runs the encoder head;
        "images" = the plan starts at the raw (B, K+1, 3, h, w) ``images`` and runs the native stem (nhwc.build_matching_stem) first."""
        geom = None
        if head == "images":
            _, shape, strides = nhwc.image_strides(images)
            geom = (tuple(shape), strides)
        key = (B, K, C, H, W, tuple(tuple(s) for s in enc_shapes), str(device), self.conv_math, head, head_ch, geom, scales,
               nhwc._param_key(self.cost_volume_net), nhwc._param_key(self.depth_decoder),
               nhwc.ParamKey(nhwc._param_key(self.matching_model.net[5]) + nhwc._param_key(self.matching_model.net[8])) if head else None,
               nhwc.stem_param_key(self.matching_model.net[:5]) if head == "images" else None)
        ent = self._plans.get(key)
        if ent is not None:
            return ent
        D = self.cost_volume.num_depth_bins
        p = nhwc.Plan(device, math=self.conv_math)
        st = {"lowest": None, "planes": torch.empty(D, device=device)}
        ent = {"plan": p, "state": st, "heads": {}, "i_l1": None}
        if head is None:
            st["cur_n"] = torch.empty(B, H, W, C, device=device)
            st["src_n"] = torch.empty(B, K, H, W, C, device=device)
            ent["feats"] = (st["cur_n"].data_ptr(), st["src_n"].data_ptr(), (B, K, C, H, W), 0, 0)
        else:
            # matching-encoder head over all B*(K+1) images at once (the reference loops image by image,
            # bd_model.py:149-160; InstanceNorm statistics are per image either way).  Image order = frame b's
            # current view then its K source views, so the result is ONE (B, K+1, H, W, C) buffer that the volume
            # kernel addresses with batch strides.
            M = B * (K + 1)
            n0 = len(p.ops)
            if head == "images":  # stem + layer1 (one fused pass + four Winograd convs), then the head, all NHWC
                x, ent["i_l1"] = nhwc.build_matching_stem(p, self.matching_model, images)
                y = nhwc.build_matching_head(p, self.matching_model, x)
            elif head == "nchw" and nhwc.FUSE_HEAD_IMPORT and nhwc.Plan.pointwise_nchw_eligible(self.matching_model.net[5]):
                # the first 1x1 conv reads the backbone's NCHW map in place: no layout-import pass
                y, ent["i_l1"] = nhwc.build_matching_head(p, self.matching_model, None, nchw_shape=(M, head_ch, H, W))
            elif head == "nchw":
                x, ent["i_l1"] = p.input_nchw((M, head_ch, H, W))
                y =nhwc.build_matching_head(p, self.matching_model, x)
            else:  # channels-last producer: the first conv reads the caller's tensor in place (pointer patched per call)
                x = nhwc.View(torch.empty(1, device=device).expand(M, H, W, head_ch), 0, head_ch)
                y = nhwc.build_matching_head(p, self.matching_model, x)
                ent["i_l1"] = n0  # the 1x1 conv added first by build_matching_head
            if y.C != C:
                raise _lib.IdhError(f"matching head produces {y.C} channels, cost volume expects {C}")
            hw = H * W * C
            ent["feats"] = (y.ptr, y.ptr + 4 * hw, (B, K, C, H, W), (K + 1) * hw, (K + 1) * hw)
            ent["match_view"] = y
        n_pre = len(p.ops)
        cv_in = p.buffer(B, H, W, D)
        v0, i_v0 = p.input_nchw(enc_shapes[0])
        outs, i_img = nhwc.build_cv_encoder(p, self.cost_volume_net, cv_in, enc_shapes[1:])
        i_enc = [i_v0] + i_img
        final = nhwc.build_any_decoder(p, self.depth_decoder, [v0] + outs, scales)
        ent.update(cv_in=cv_in, i_enc=i_enc, final=final)
        if getattr(self.depth_decoder, "depth_head", False):
            for i, v in final.items():
                ent["heads"][i] = p.head(v, self.depth_decoder.convs[f"output_{i}"][1], torch.empty(1, device=device))
        elif hasattr(self.depth_decoder, "out1"):  # SkipDecoderRegression
            for i, (hv, last) in nhwc.build_regression_heads(p, self.depth_decoder, final).items():
                ent["heads"][i] = p.head(hv, last, torch.empty(1, device=device))
        # the volume kernel runs between the matching head and the CVEncoder: two replay segments of one plan
        ent["n_head_ops"] = p.schedule_segments(n_pre)
        return self._plans.put(key, ent)

    # ------------------------------------------------------------------------------------
    def forward(self, matching_cur_feats: Optional[torch.Tensor], matching_src_feats: Optional[torch.Tensor], cur_feats: List[torch.Tensor],
                src_cam_T_cur_cam: torch.Tensor, cur_cam_T_src_cam: torch.Tensor, src_K: torch.Tensor, cur_invK: torch.Tensor,
                rendered_depth: Optional[torch.Tensor] = None, prior: Optional[torch.Tensor] = None,
                return_mask: bool = False, return_features: bool = False,
                prior_inputs: Optional[Dict[str, torch.Tensor]] = None, infer_depth: bool = False,
                matching_layer1: Optional[torch.Tensor] = None, return_matching_feats: bool = False,
                frame_chain: Optional[Dict[str, torch.Tensor]] = None, matching_images: Optional[torch.Tensor] = None,
                matching_nhwc: Optional[Sequence[torch.Tensor]] = None, query_rays: Optional[torch.Tensor] = None,
                query_depths: Optional[torch.Tensor] = None, query_prior=None, query_grid: Optional[Sequence[int]] = None,
                query_scales: Sequence[int] = (0,)) -> Dict[str, torch.Tensor]:
        """``matching_layer1`` (B, K+1, 64, H, W): output of the matching backbone (conv1..layer1 of the ResNet18,
        third-party, run by the caller) for frame b's current image followed by its K source images — the order
        reference bd_model.py:149-160 builds; contiguous or channels-last per image
        (``x.view(-1, 64, H, W)`` in ``torch.channels_last``).  With it the encoder head (networks.py:279-283) runs
        inside this call and ``matching_cur_feats`` / ``matching_src_feats`` must be None.
        ``prior``: an already-warped prior channel (B,P,H/2,W/2), or ``prior_inputs`` = the
        reference's temporal inputs {"prior_prediction", "prior_cam_T_world", "world_T_cam_b44",
        "K_s0_b44", "invK_s0_b44"} (bd_model.py:420-431) to warp it here; with neither, a
        prior-enabled MLP sees the constant -1 (bd_model.py:433-434).
        ``frame_chain``: the B batch entries are CONSECUTIVE FRAMES OF ONE SEQUENCE (the temporal loop of
        inference/inference.py:139-157 over a recorded scan).  Everything up to the decoder does not depend on the previous
        frame, so it runs once for all B frames; only the occlusion MLP is evaluated frame by frame, frame b taking
        sigmoid(pred_0) of frame b-1 - warped by sample_prior with frame b-1's cam_T_world - as its prior, exactly as B
        separate calls would.  Keys: "world_T_cam_b44", "cam_T_world_b44" (B,4,4: the frames' poses), "K_s0_b44",
        "invK_s0_b44" (B,4,4), and the chain's start "prior_prediction" (1,1,H/2,W/2) + "prior_cam_T_world" (1,4,4) (or None
        for the first frame of a sequence).  Returns the usual dictionary with pred_0 of all B frames (the last one's
        sigmoid and pose are the next call's chain start).
        ``matching_images`` (B, K+1, 3, h, w): instead of ``matching_layer1``, the raw images in the same order; the matching encoder's
        ResNet18 stem (conv1 .. layer1, backbone.py) then runs natively inside this call as well, the whole encoder in the same plan.
        Needs a ``matching_model`` whose ``net[:5]`` passes ``backbone.stem_is_native_eligible`` (eval mode).
        ``matching_nhwc`` = (cur (B,H,W,C), src (B,K,H,W,C)): FINISHED matching features that are already channels-last and contiguous
        (``FeatureBank.gather``'s output, ``ResnetMatchingEncoder(..., channels_last=True)``); the volume kernel reads them in place, with no
        layout import.  Excludes the four other forms.
        ``query_rays`` (B,N,2) + ``query_depths`` (B,N,S): sparse occlusion queries against this forward's decoder output, with or without
        ``rendered_depth`` - see ``query_rays()``; adds ``out["ray_pred_{s}"]`` (B,1,ceil(N/(s+1)),S) for s in ``query_scales``.  Scales 1-3
        need the full decoder plan (the plan key's ``scales``)."""
        _lib.require_cuda_f32(matching_cur_feats, matching_src_feats, matching_layer1, matching_images, src_cam_T_cur_cam, src_K, cur_invK, rendered_depth, prior, *cur_feats)
        if (query_rays is None) != (query_depths is None):
            raise _lib.IdhError("query_rays and query_depths come together")
        query_scales = self._check_query_scales(query_scales) if query_rays is not None else ()
        if matching_nhwc is not None:
            if matching_cur_feats is not None or matching_src_feats is not None or matching_layer1 is not None or matching_images is not None:
                raise _lib.IdhError("pass one of finished matching features (NCHW or matching_nhwc), matching_layer1 or matching_images")
            cur_n, src_n = matching_nhwc
            _lib.require_cuda_f32(cur_n, src_n)
            if src_n.dim() != 5 or tuple(cur_n.shape) != (src_n.shape[0], *src_n.shape[2:]) or not (cur_n.is_contiguous() and src_n.is_contiguous()):
                raise _lib.IdhError(f"matching_nhwc must be contiguous (B,H,W,C) and (B,K,H,W,C), got {tuple(cur_n.shape)} and {tuple(src_n.shape)}")
        head = None
        head_ch = 0
        images = None
        if matching_images is not None:
            if matching_cur_feats is not None or matching_src_feats is not None or matching_layer1 is not None:
                raise _lib.IdhError("pass one of finished matching features, matching_layer1 or matching_images")
            if self.matching_model is None:
                raise _lib.IdhError("matching_images needs HotPath(matching_model=...)")
            if matching_images.dim() != 5 or matching_images.shape[2] != 3:
                raise _lib.IdhError(f"matching_images must be (B, K+1, 3, H, W), got {tuple(matching_images.shape)}")
            nhwc.require_native_stem(self.matching_model)
            images, _, _ = nhwc.image_strides(matching_images)
            B, K1, _, h_img, w_img = images.shape
            K, C, head, head_ch = K1 - 1, self.matching_model.net[8].out_channels, "images", 64
            H, W = ((h_img + 1) // 2) // 2, ((w_img + 1) // 2) // 2
            l1 = images
        elif matching_layer1 is not None:
            if matching_cur_feats is not None or matching_src_feats is not None:
                raise _lib.IdhError("pass either finished matching features or matching_layer1, not both")
            if self.matching_model is None:
                raise _lib.IdhError("matching_layer1 needs HotPath(matching_model=...)")
            if matching_layer1.dim() != 5:
                raise _lib.IdhError(f"matching_layer1 must be (B, K+1, C, H, W), got {tuple(matching_layer1.shape)}")
            B, K1, head_ch, H, W = matching_layer1.shape
            K, C = K1 - 1, self.matching_model.net[8].out_channels
            l1 = matching_layer1.reshape(B * K1, head_ch, H, W)
            if l1.is_contiguous():
                head = "nchw"
            elif l1.is_contiguous(memory_format=torch.channels_last):
                head = "nhwc"
            else:
                l1, head = l1.contiguous(), "nchw"
        elif matching_nhwc is not None:
            B, K, H, W, C = src_n.shape
        else:
            B, K, C, H, W = matching_src_feats.shape
        dev = src_K.device
        cur_feats = [f if f.is_contiguous() else f.contiguous() for f in cur_feats]
        ent = self._plan(B, K, C, H, W, [f.shape for f in cur_feats], dev, head, head_ch, images, self._scales(return_features, query_scales))
        p, st = ent["plan"], ent["state"]
        L = _lib.lib()
        sp = _lib.stream_ptr()
        D = self.cost_volume.num_depth_bins
        out: Dict[str, torch.Tensor] = {}

        # 0. matching features: the encoder head (first segment of the plan) or a layout import of finished features
        zero_volume = isinstance(self.cost_volume, ZeroCostVolumeManager)
        if head is not None:
            p.set_in(ent["i_l1"], l1)
            p.run(0, ent["n_head_ops"])
        elif matching_nhwc is not None:
            pass  # read in place below
        elif not zero_volume:
            mc = matching_cur_feats if matching_cur_feats.is_contiguous() else matching_cur_feats.contiguous()
            ms = matching_src_feats if matching_src_feats.is_contiguous() else matching_src_feats.contiguous()
            _lib.check(L.idh_nchw_to_nhwc_f32(mc.data_ptr(), st["cur_n"].data_ptr(), B, C, H * W, sp), "idh_nchw_to_nhwc_f32")
            _lib.check(L.idh_nchw_to_nhwc_f32(ms.data_ptr(), st["src_n"].data_ptr(), B * K, C, H * W, sp), "idh_nchw_to_nhwc_f32")
        feats = ent["feats"] if matching_nhwc is None else (cur_n.data_ptr(), src_n.data_ptr(), (B, K, C, H, W), 0, 0)
        cur_ptr, src_ptr, dims, cbs, sbs = feats

        # 1. cost volume, written NHWC straight into the CVEncoder's input buffer
        lowest = torch.empty(B, H, W, device=dev)
        mask = None
        if zero_volume:
            ent["cv_in"].buf.zero_()
            planes = self.cost_volume.generate_depth_planes(B, torch.tensor(self.min_depth, device=dev).view(1, 1, 1, 1),
                                                            torch.tensor(self.max_depth, device=dev).view(1, 1, 1, 1))
            lowest = planes[:, 0]
        elif type(self.cost_volume) is CostVolumeManager:
            mats = [t if t.is_contiguous() else t.contiguous() for t in (src_K, src_cam_T_cur_cam, cur_invK)]  # alive until enqueued
            opts, _keep = volume_opts(B, K, C, H, W, D, None, cbs, sbs, kernel=self.cost_volume.__dict__.get("kernel", 0), dot_scratch_device=dev)
            _lib.check(L.idh_cost_volume_dot_ex_fwd(cur_ptr, src_ptr, mats[0].data_ptr(), mats[1].data_ptr(), mats[2].data_ptr(),
                                                    self.min_depth, self.max_depth, B, K, C, H, W, D, ent["cv_in"].ptr, ent["cv_in"].cs,
                                                    lowest.data_ptr(), st["planes"].data_ptr(), opts, sp), "idh_cost_volume_dot_ex_fwd")
        else:
            lowest, mask = self.cost_volume.fused_into(ent["cv_in"], st, feats, src_cam_T_cur_cam, cur_cam_T_src_cam, src_K, cur_invK,
                                                       self.min_depth, self.max_depth, return_mask)

        # 2. CVEncoder + UNet++ decoder: one idh_run_ops call
        for idx, f in zip(ent["i_enc"], cur_feats):
            p.set_in(idx, f)
        final = ent["final"]
        if ent["heads"]:
            for i, idx in ent["heads"].items():
                v = final[i]
                t = torch.empty(B, 1, v.H, v.W, device=dev)
                e = torch.empty(B, 1, v.H, v.W, device=dev)
                p.set_out(idx, t, exp_out=e)  # the head kernel writes log-depth and exp(log-depth) (depth_model.py:425-433)
                out[f"log_depth_pred_s{i}_b1hw"] = t
                out[f"depth_pred_s{i}_b1hw"] = e
        p.run(ent["n_head_ops"])
        self._last = {"ent": ent, "final": final, "B": B}  # (the entry keeps its buffers alive if the cache drops it)

        # 3. occlusion MLP over every query plane (BDModel only)
        if self.binary_mlp is not None and rendered_depth is not None and frame_chain is not None:
            from .mlp import sample_prior

            if infer_depth or prior is not None or prior_inputs is not None:
                raise _lib.IdhError("frame_chain excludes prior / prior_inputs / infer_depth")
            if not getattr(self.binary_mlp, "use_prior", False):
                raise _lib.IdhError("frame_chain needs an occlusion MLP built with use_prior=True")
            for k in ("world_T_cam_b44", "cam_T_world_b44", "K_s0_b44", "invK_s0_b44"):
                if k not in frame_chain or tuple(frame_chain[k].shape) != (B, 4, 4):
                    raise _lib.IdhError(f"frame_chain[{k!r}] must be ({B}, 4, 4): one pose / intrinsics matrix per frame of the batch")
            if (frame_chain.get("prior_prediction") is None) != (frame_chain.get("prior_cam_T_world") is None):
                raise _lib.IdhError("frame_chain: prior_prediction and prior_cam_T_world come together (both None at the first frame of a sequence)")
            _lib.require_cuda_f32(*[t for t in frame_chain.values() if t is not None])
            f0 = final[0]
            prev_pred, prev_cTw = frame_chain.get("prior_prediction"), frame_chain.get("prior_cam_T_world")
            pred = torch.empty(B, rendered_depth.shape[1], f0.H, f0.W, device=dev)
            priors = []
            for b in range(B):
                pb = None
                if prev_pred is not None:
                    pb = sample_prior(rendered_depth[b:b + 1], prev_pred, frame_chain["world_T_cam_b44"][b:b + 1], prev_cTw,
                                      frame_chain["K_s0_b44"][b:b + 1], frame_chain["invK_s0_b44"][b:b + 1])
                priors.append(pb)
                occlusion_logits(self.binary_mlp, f0.buf[b:b + 1], f0.c0, f0.C, rendered_depth[b:b + 1], pb, out=pred[b:b + 1])
                prev_pred, prev_cTw = torch.sigmoid(pred[b:b + 1]), frame_chain["cam_T_world_b44"][b:b + 1]  # sigmoid_custom(x, 1.0), inference.py:154
            out["pred_0"] = pred
            if all(t is not None for t in priors):
                out["prior_mask"] = torch.cat(priors, 0)
        elif self.binary_mlp is not None and rendered_depth is not None:
            if prior is None and prior_inputs is not None and prior_inputs.get("prior_prediction") is not None:
                from .mlp import sample_prior

                prior = sample_prior(rendered_depth, prior_inputs["prior_prediction"], prior_inputs["world_T_cam_b44"],
                                     prior_inputs["prior_cam_T_world"], prior_inputs["K_s0_b44"], prior_inputs["invK_s0_b44"])
                out["prior_mask"] = prior
            f0 = final[0]
            if infer_depth:  # bd_model.py:273-292: 12-step per-pixel binary search, one launch
                from .mlp import infer_depth as _search

                out["search_depths"], out["pred_0"] = _search(self.binary_mlp, f0.buf, f0.c0, f0.C, prior[:, :1] if prior is not None else None,
                                                              thresholder=self.thresholder)
            else:
                out["pred_0"] = occlusion_logits(self.binary_mlp, f0.buf, f0.c0, f0.C, rendered_depth, prior)
        if query_rays is not None:
            out.update(self.query_rays(query_rays, query_depths, query_prior, query_grid, query_scales))
        if return_features:
            for i, v in final.items():
                out[f"feature_s{i}_b1hw"] = _export(v)
        if return_matching_feats and head is not None:
            y = ent["match_view"]
            feats = _export(y).view(B, K + 1, C, H, W)
            out["matching_cur_feats"], out["matching_src_feats"] = feats[:, 0], feats[:, 1:]
        out["lowest_cost_bhw"] = lowest
        out["overall_mask_bhw"] = mask
        return out


def _last_final(hot: HotPath, B: int, scales: Sequence[int]):
    if hot.binary_mlp is None:
        raise _lib.IdhError("occlusion queries need a HotPath with a binary_mlp")
    last = hot._last
    if last is None:
        raise _lib.IdhError("no forward has run on this HotPath yet: queries read the decoder output of the last forward")
    if last["B"] != B:
        raise _lib.IdhError(f"the last forward had batch size {last['B']}, the query has {B}")
    missing = [s for s in scales if s not in last["final"]]
    if missing:
        raise _lib.IdhError(f"the last forward built no decoder output at scales {missing}: pass query_scales (or return_features=True) to that forward")
    return last["final"]


def _export(v: nhwc.View) -> torch.Tensor:
    t = torch.empty(v.N, v.C, v.H, v.W, device=v.buf.device)
    p = nhwc.Plan(v.buf.device)
    p.export_nchw(v, t)
    p.run()
    return t
