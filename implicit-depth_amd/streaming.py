"""A live sequence: ``StreamingSession`` joins frame ingest, the keyframe buffer, the feature bank and the fused forward.

The reference builds its test tuples off line (data_scripts/generate_test_tuples.py:161-212: ``KeyframeBuffer`` over a scan's poses) and
its forward runs the matching encoder on the current image AND the K source images of every tuple (bd_model.py:149-160).  In a stream
the K source views are keyframes whose features were computed when they were the current frame.  Per frame the session

1. asks ``keyframes.KeyframeBuffer`` (the host pose decides: return codes 0-5); a frame the buffer does not store costs nothing more;
2. runs the matching encoder (native stem, layer1 and head) on the ONE current image, channels-last;
3. commits its features, poses and ``K_s1`` to the ``FeatureBank`` slot the buffer handed out;
4. on a new keyframe selects K measurement slots - the reference's choice in the reference's order - and gathers them in one launch;
5. runs ``HotPath`` from the finished channels-last features (``matching_nhwc``): volume, CVEncoder, decoder, occlusion MLP / depth heads.

With ``use_prior`` the previous prediction's ``sigmoid(pred_0)`` and ``cam_T_world`` are carried to the next prediction
(inference/inference.py:139-157).  The image encoder stays the model's own torch module, as in ``dropin.fused_forward``.

Mode ``"keyframe"`` predicts on return code 1 only, as the DVMVS buffer intends (``default_dvmvs_tuples``).  The reference's dense rule
(``dense_dvmvs_tuples``, generate_test_tuples.py:264-336) is NOT provided: for every frame it walks back over ALL earlier frames with a
fresh ``OfflineKeyframeBuffer`` until 30 of them are accepted, so any earlier frame - keyframe or not, arbitrarily far back when the camera
moves slowly - can be a source view; a ring that keeps the features of the last N keyframes cannot serve that choice."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib, keyframes
from .feature_bank import FeatureBank
from .pipeline import MAX_RING_CAPACITY, HotPath

MODES = ("keyframe",)


def nearest_keys_first(live_world_T_cam, key_poses_newest_first) -> list:
    """The order in which a live view asks the remembered keyframes: indices into ``key_poses_newest_first`` - (4,4) camera-to-world host
    arrays, newest first - sorted by ``keyframes.pose_distance`` from the live pose, nearest first; equal distances go to the newer key."""
    live = np.asarray(live_world_T_cam, dtype=np.float64)
    dist = [float(keyframes.pose_distance(live, np.asarray(p, dtype=np.float64))[0]) for p in key_poses_newest_first]
    return sorted(range(len(dist)), key=lambda i: (dist[i], i))


def patch_rays(rays: torch.Tensor, step: float = 1.0) -> torch.Tensor:
    """(B,9N,2): every ray (x, y) of ``rays`` (B,N,2) with its eight neighbours ``step`` pixels apart, patch-major; inside a patch row-major
    (y - step first, x - step first), so index 4 is the ray itself - exactly: its offset is 0."""
    o = torch.tensor([-1.0, 0.0, 1.0], device=rays.device, dtype=rays.dtype) * float(step)
    off = torch.stack([o.repeat(3), o.repeat_interleave(3)], -1)  # (9,2): x runs fastest
    return (rays[:, :, None, :] + off).reshape(rays.shape[0], -1, 2)


class StreamingSession:
    """``model``: a reference ``BDModel`` / ``DepthModel`` (converted in place by ``dropin.hot_path_of``; its ``encoder`` is the image
    encoder) or a ``HotPath`` with a ``matching_model`` (then pass ``image_encoder``).  The matching encoder's stem must be eligible for
    the native kernels (``backbone.stem_is_native_eligible``).  ``num_source_views``: K; read off an MLP feature volume, required for the
    dot-product volume.  ``buffer_size``: keyframes kept (the ring's slots, at most 64 and more than K); ``config``: the DVMVS thresholds.
    ``query_keyframes``: how many predictions ``occlusion_for_view`` / ``depth_for_view`` / ``raycast_view`` ask.  1 (the default): the
    last one, as ever.  N in [2, 16]: every prediction is remembered (``HotPath.remember``, with its own ``sigmoid(pred_0[:, :1])`` and
    camera as its prior under ``use_prior``) and a live pixel is asked in the first of the last N whose camera sees it, nearest pose
    first (``nearest_keys_first``); the dictionaries gain "view_key" / "view_search_key".  ``reset()`` empties that ring; like the last
    prediction it survives a tracking-lost code.  The same number bounds the ring of depth maps (``remember_depth``: a ``DepthModel``'s
    predictions, pushed by ``step``; lidar frames or an inferred depth, pushed by the caller) that ``warped_depth_for_view`` draws into
    a live camera and the depth route of ``composite_asset`` composites against.  ``start_fusion`` adds a memory that is not bounded by
    that ring: every remembered map is also averaged into a TSDF volume (``fusion.TSDFVolume``) that ``fused_depth_for_view`` ray-casts."""

    def __init__(self, model: nn.Module, num_source_views: Optional[int] = None, buffer_size: Optional[int] = None, mode: str = "keyframe",
                 config=keyframes.DVMVS_Config, image_encoder: Optional[nn.Module] = None, math: Optional[str] = None,
                 query_keyframes: int = 1):
        if not 1 <= int(query_keyframes) <= MAX_RING_CAPACITY:
            raise _lib.IdhError(f"query_keyframes must be in [1, {MAX_RING_CAPACITY}], got {query_keyframes}")
        if mode not in MODES:
            raise _lib.IdhError(f"mode must be one of {MODES}, got {mode!r} (the reference's dense tuples cannot be served from a keyframe "
                                "ring: see the module docstring)")
        self._model = None
        if isinstance(model, HotPath):
            self.hot, self.image_encoder = model, image_encoder
            use_prior = bool(getattr(model.binary_mlp, "use_prior", False))
        else:
            from .dropin import hot_path_of

            if getattr(getattr(model, "run_opts", None), "matching_scale", 1) != 1:
                raise _lib.IdhError("the streaming session covers matching_scale = 1, as dropin.fused_forward")
            self._model = model
            self.hot = hot_path_of(model, math=math, native_matching_stem=True)
            self.image_encoder = image_encoder if image_encoder is not None else model.encoder
            use_prior = bool(getattr(getattr(model, "run_opts", None), "use_prior", False)) and self.hot.binary_mlp is not None
        if self.image_encoder is None:
            raise _lib.IdhError("StreamingSession(HotPath) needs image_encoder=...")
        if self.hot.matching_model is None:
            raise _lib.IdhError("StreamingSession needs a ResnetMatchingEncoder (HotPath(matching_model=...))")
        from .nhwc import require_native_stem

        require_native_stem(self.hot.matching_model)
        self.use_prior = use_prior
        K = getattr(self.hot.cost_volume, "num_source_views", None) or num_source_views
        if K is None:
            raise _lib.IdhError("num_source_views is required for a dot-product cost volume")
        if num_source_views is not None and int(num_source_views) != int(K):
            raise _lib.IdhError(f"the feature volume was built for {K} source views, got num_source_views={num_source_views}")
        self.K = int(K)
        size = config.test_keyframe_buffer_size if buffer_size is None else int(buffer_size)
        if not self.K < size <= _lib.BANK_MAX_SLOTS:
            raise _lib.IdhError(f"buffer_size must be in ({self.K}, {_lib.BANK_MAX_SLOTS}]: K source views plus the current keyframe, got {size}")
        self.mode = mode
        self.buffer = keyframes.KeyframeBuffer.from_config(config, buffer_size=size)
        self.bank: Optional[FeatureBank] = None
        self.frame_index = 0
        self.last_code: Optional[int] = None
        self.last_slots: Optional[Tuple[int, ...]] = None    # ring slots of the last prediction's source views, in order
        self.last_indices: Optional[Tuple[int, ...]] = None  # their frame numbers
        self.last_matching: Optional[Tuple[torch.Tensor, torch.Tensor]] = None  # (cur (1,H,W,C), src (1,K,H,W,C)) of the last prediction
        self._prior: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self._key: Optional[Dict[str, torch.Tensor]] = None  # the last prediction's poses and intrinsics: what query_points / raycast / occlusion_for_view use
        # query_keyframes = N > 1: every prediction is remembered on the HotPath's ring (HotPath.remember) and occlusion_for_view /
        # depth_for_view / raycast_view ask the last N of them, nearest pose first.  Like _key the ring survives a tracking-lost code -
        # and so do the priors remembered with its predictions, while the single-key queries drop theirs there; reset() empties it.
        self.query_keyframes = int(query_keyframes)
        self._ring_poses: Dict[int, np.ndarray] = {}  # ring slot -> that prediction's world_T_cam on the host
        # the last query_keyframes depth maps (remember_depth), newest first: (depth (1,1,h,w), world_T_cam float64 (4,4), invK (1,4,4)).
        # What warped_depth_for_view draws; a DepthModel's predictions are pushed by step(), lidar or an inferred depth by the caller.
        self._depth_ring: list = []
        self._fusion: Optional[dict] = None  # start_fusion's arguments; the volume is made when the first map arrives
        self._volume = None                  # fusion.TSDFVolume
        self._fused_maps = 0                 # maps integrated since start_fusion / reset
        # start_fusion(consistency=): per ring map, newest first, its (K (1,4,4), cam_T_world (1,4,4)) on the device - what the check projects with
        self._ring_cams: list = []
        self.last_depth_counts: Optional[torch.Tensor] = None  # (1,3,h,w) uint8 of the last check: sources that see / agree with / conflict with a pixel
        # start_fusion(follow=): how often the volume was moved after the camera since start_fusion / reset, and the last (sx, sy, sz)
        self.fusion_scrolls = 0
        self.last_scroll: Optional[Tuple[int, int, int]] = None
        # start_fusion(track=): what the last alignment of a remembered map came to (None: none yet, or the first map of a sequence)
        self.last_alignment: Optional[dict] = None

    def reset(self) -> None:
        """Start a new sequence: empty buffer, no prior.  The bank's storage is kept."""
        self.buffer = keyframes.KeyframeBuffer(self.buffer.buffer_size, self.buffer.keyframe_pose_distance, self.buffer.optimal_t_score,
                                               self.buffer.optimal_R_score)
        self.frame_index, self.last_code, self.last_slots, self.last_indices, self.last_matching, self._prior = 0, None, None, None, None, None
        self._key = None
        self._depth_ring = []
        self._ring_cams, self.last_depth_counts = [], None
        self._fused_maps = 0
        self.fusion_scrolls, self.last_scroll = 0, None
        self.last_alignment = None
        if self._volume is not None:
            self._volume.reset()  # (with origin=None the next first map centres the grid again)
        if self.query_keyframes > 1:
            self.hot.forget()
            self._ring_poses = {}

    def step(self, cur_data: Dict[str, torch.Tensor], world_T_cam=None, dist_to_last_valid=None, return_mask: bool = False,
             infer_depth: bool = False, query_points: Optional[torch.Tensor] = None, frame_u8: Optional[torch.Tensor] = None,
             frame_K: Optional[torch.Tensor] = None) -> Tuple[Optional[Dict[str, torch.Tensor]], int]:
        """``cur_data``: what ``FrameIngest`` returns for ONE frame (``image_b3hw``, ``world_T_cam_b44``, ``cam_T_world_b44``, ``K_s0/s1_b44``,
        ``invK_s0/s1_b44``; for a BDModel also ``rendered_depth``).  ``world_T_cam``: the same pose as a (4,4) host array, in the dtype the
        selection is to be computed in - the keyframe decision is taken on the host; without it the pose is read back from the device, which synchronises.
        Returns ``(outputs, code)``: the output dictionary of ``fused_forward`` when a prediction is due, else None - first frame, not enough
        motion, no pose, tracking lost, or fewer than K keyframes stored so far; ``code`` is the buffer's return code either way.
        ``query_points`` (1,N,3) world points: when a prediction is due, its outputs gain ``point_pred`` / ``point_valid`` / ``point_depth`` /
        ``point_rays`` (``HotPath.query_points`` against this prediction); on the other frames ask ``session.query_points``.
        ``frame_u8`` / ``frame_K``: the camera frame of this step, handed to the ``remember_depth`` a ``DepthModel``'s prediction goes to
        (``start_fusion(color=True)``)."""
        image = cur_data["image_b3hw"]
        if image.dim() != 4 or image.shape[0] != 1:
            raise _lib.IdhError(f"step() takes one frame: image_b3hw must be (1,3,h,w), got {tuple(image.shape)}")
        if world_T_cam is None:
            world_T_cam = cur_data["world_T_cam_b44"][0].detach().cpu().numpy()
        pose = np.asarray(world_T_cam.detach().cpu().numpy() if isinstance(world_T_cam, torch.Tensor) else world_T_cam)  # dtype kept: the reference's arithmetic is its caller's
        if pose.shape != (4, 4):
            raise _lib.IdhError(f"world_T_cam {pose.shape} must be (4,4)")
        index = self.frame_index
        self.frame_index += 1
        code = self.last_code = self.buffer.try_new_keyframe(pose, dist_to_last_valid, index=index)
        if code == keyframes.CODE_TRACKING_LOST:
            self._prior = None  # the previous prediction belongs to a track that ended
        slot = self.buffer.stored_slot
        if slot is None:
            return None, code
        from .nhwc import matching_encoder_forward

        with torch.inference_mode():
            cur_n = matching_encoder_forward(self.hot.matching_model, image, channels_last=True)  # (1,H,W,C)
            _, H, W, C = cur_n.shape
            if self.bank is None or (self.bank.H, self.bank.W, self.bank.C) != (H, W, C) or self.bank.device != cur_n.device:
                self.bank = FeatureBank(self.buffer.buffer_size, H, W, C, device=cur_n.device)
            self.bank.commit(slot, cur_n, cur_data["world_T_cam_b44"], cur_data["cam_T_world_b44"], cur_data["K_s1_b44"])
            if code != keyframes.CODE_KEYFRAME or len(self.buffer) - 1 < self.K:
                return None, code
            frames = self.buffer.get_best_measurement_frames(self.K)
            self.last_slots, self.last_indices = tuple(s for _, s, _ in frames), tuple(i for _, _, i in frames)
            g = self.bank.gather([self.last_slots], cur_data["world_T_cam_b44"], cur_data["cam_T_world_b44"])
            self.last_matching = (cur_n, g["src_nhwc"])
            kw = {}
            if self.hot.binary_mlp is not None:
                kw["rendered_depth"], kw["infer_depth"] = cur_data["rendered_depth"], infer_depth
                if self.use_prior and self._prior is not None:
                    kw["prior_inputs"] = {"prior_prediction": self._prior[0], "prior_cam_T_world": self._prior[1],
                                          "world_T_cam_b44": cur_data["world_T_cam_b44"], "K_s0_b44": cur_data["K_s0_b44"],
                                          "invK_s0_b44": cur_data["invK_s0_b44"]}
            if self._model is not None:
                self.hot.thresholder = getattr(self._model, "thresholder", None)
            cur_feats = list(self.image_encoder(image))
            out = self.hot(None, None, cur_feats, g["src_E"], g["src_poses"], g["src_K"], cur_data["invK_s1_b44"], return_mask=return_mask,
                           matching_nhwc=self.last_matching, **kw)
            if self.use_prior and "pred_0" in out:
                self._prior = (torch.sigmoid(out["pred_0"]), cur_data["cam_T_world_b44"])  # sigmoid_custom(x, 1.0), inference.py:154
            if self.hot.binary_mlp is not None:
                self._key = {"cam_T_world_b44": cur_data["cam_T_world_b44"], "K_s0_b44": cur_data["K_s0_b44"],
                             "world_T_cam_b44": cur_data["world_T_cam_b44"], "invK_s0_b44": cur_data["invK_s0_b44"]}
                if self.query_keyframes > 1:
                    pi = None
                    if self.use_prior and "pred_0" in out:
                        pi = {"prior_prediction": torch.sigmoid(out["pred_0"][:, :1]), "prior_cam_T_world": cur_data["cam_T_world_b44"]}
                    slot = self.hot.remember(cur_data["cam_T_world_b44"], cur_data["K_s0_b44"], prior_inputs=pi, capacity=self.query_keyframes)
                    self._ring_poses[slot] = np.array(pose, dtype=np.float64)
                if query_points is not None:
                    out.update(self.query_points(query_points))
            elif "depth_pred_s0_b1hw" in out:  # a DepthModel: its prediction is what the frames between keyframes can be answered from
                self.remember_depth(out["depth_pred_s0_b1hw"], pose, cur_data["invK_s0_b44"], frame_u8=frame_u8, frame_K=frame_K)
        if "prior_mask" in out:
            cur_data["prior_mask"] = out.pop("prior_mask")  # as fused_forward: run_mlp_val stores it on the inputs (bd_model.py:431)
        return out, code

    def query_points(self, points_bn3: torch.Tensor, world_T_cam=None) -> Dict[str, torch.Tensor]:
        """Occlusion of points (1,N,3) against the LAST prediction's decoder features and pose - also on the frames where ``step`` returned
        None: no network runs, the features and the camera are the keyframe's.  The points are world points, or - with ``world_T_cam``, a
        (4,4) array or tensor - points in that (live) camera's frame, taken to the world first.  With ``use_prior`` the carried prior - the
        sigmoid of that prediction's ``pred_0``, which the next prediction will see - is sampled at the points' projections into the
        keyframe's camera.  Returns ``HotPath.query_points``' dictionary."""
        if self._key is None:
            raise _lib.IdhError("no prediction has been made in this sequence yet (step() returned None so far)")
        _lib.require_cuda_f32(points_bn3)
        k = self._key
        if world_T_cam is not None:
            T = torch.as_tensor(world_T_cam.detach().cpu().numpy() if isinstance(world_T_cam, torch.Tensor) else np.asarray(world_T_cam))
            T = T.to(device=points_bn3.device, dtype=torch.float32)
            if tuple(T.shape) != (4, 4):
                raise _lib.IdhError(f"world_T_cam {tuple(T.shape)} must be (4,4)")
            points_bn3 = points_bn3 @ T[:3, :3].t() + T[:3, 3]
        pi = None
        if self.use_prior and self._prior is not None:
            pi = {"prior_prediction": self._prior[0][:, :1], "prior_cam_T_world": self._prior[1]}
        with torch.inference_mode():
            return self.hot.query_points(points_bn3, k["cam_T_world_b44"], k["K_s0_b44"], prior_inputs=pi)

    def occlusion_for_view(self, rendered_depth: torch.Tensor, world_T_cam, invK: torch.Tensor, fill: float = 0.0) -> Dict[str, Optional[torch.Tensor]]:
        """Occlusion logits of an asset in the LIVE camera, also on the frames where ``step`` returned None: ``rendered_depth`` (1,P,h,w) is
        the asset's depth rendered in the camera at ``world_T_cam`` - a (4,4) array or tensor - with inverse intrinsics ``invK`` ((4,4) or
        (1,4,4), at h x w; any resolution).  Every pixel is asked against the LAST prediction's decoder features through the keyframe's
        ``cam_T_world`` and ``K_s0`` (``HotPath.query_view``, one launch); with ``use_prior`` the carried prior is sampled as in
        ``query_points``.  Returns ``HotPath.query_view``'s dictionary: "view_pred" (1,P,h,w) is in the live view, ``fill`` where
        "view_valid" is False, and feeds ``compositing.composite_mask(image_u8, view_pred)`` as a prediction's ``pred_0`` does."""
        if self._key is None:
            raise _lib.IdhError("no prediction has been made in this sequence yet (step() returned None so far)")
        _lib.require_cuda_f32(rendered_depth, invK)
        k = self._key
        T = torch.as_tensor(world_T_cam.detach().cpu().numpy() if isinstance(world_T_cam, torch.Tensor) else np.asarray(world_T_cam))
        if tuple(T.shape) != (4, 4):
            raise _lib.IdhError(f"world_T_cam {tuple(T.shape)} must be (4,4)")
        T_host = T
        T = T.to(device=rendered_depth.device, dtype=torch.float32)[None]
        if invK.dim() == 2:
            invK = invK[None]
        if self.query_keyframes > 1:
            with torch.inference_mode():
                return self.hot.query_view_keys(rendered_depth, invK, T, order=self._key_order(T_host), fill=fill)
        pi = None
        if self.use_prior and self._prior is not None:
            pi = {"prior_prediction": self._prior[0][:, :1], "prior_cam_T_world": self._prior[1]}
        with torch.inference_mode():
            return self.hot.query_view(rendered_depth, invK, T, k["cam_T_world_b44"], k["K_s0_b44"], prior_inputs=pi, fill=fill)

    def composite_asset(self, image_u8: torch.Tensor, asset, world_T_cam, K: torch.Tensor, *, query_size: Sequence[int] = None,
                        fill: float = -20.0, fade=None, bgr: bool = False, return_parts: bool = False, depth_source: Optional[str] = None):
        """The whole live frame, also on the frames where ``step`` returned None: the camera image ``image_u8`` (1,H,W,3) uint8 with
        ``asset`` - a ``raster.AssetRenderer`` - drawn into it at the live pose ``world_T_cam`` ((4,4) array or tensor), hidden where
        the scene is in front of it.  ``K`` ((4,4) or (1,4,4)) is the live camera's intrinsics at the image's H x W.  The asset is rendered
        once at ``query_size`` (default ``compositing.MODEL_SIZE``) for its depth - with the first two rows of ``K`` scaled by w / W and
        h / H, which is exact under the half-integer pixel centres the rasteriser and the view query share - and once at H x W for its
        RGBA; then ``occlusion_for_view(depth, world_T_cam, inv(K_query), fill)`` and
        ``compositing.composite_mask(image_u8, view_pred, virtual_rgba=rgba, fade=fade, bgr=bgr)``.  ``fill`` is the logit of the pixels
        the keyframe cannot answer (-20: the asset stays visible there).  Returns the (1,H,W,3) uint8 frame; with ``return_parts`` a
        dictionary with "frame", "asset_depth" (1,1,h,w; -1 where the asset is not), "asset_rgba" (1,H,W,4) and the view query's entries.

        A session without an occlusion MLP (a ``DepthModel``) takes the depth route (inference/composite.py:104-134): the asset's depth
        and RGBA in one render at H x W, ``warped_depth_for_view`` at ``query_size`` with ``WARP_FAR`` where no remembered map saw
        anything (the asset stays visible there), then ``compositing.composite_depth(image_u8, warped, virtual_depth=asset depth,
        virtual_rgba=rgba, fade=fade, bgr=bgr)``.  ``fill`` is not used; "asset_depth" is then (1,1,H,W) and the parts hold
        ``warped_depth_for_view``'s entries.

        ``depth_source="fused"`` (any session after ``start_fusion``, a ``BDModel``'s fed with inferred depths included) takes the depth
        route against the fused volume: ``fused_depth_for_view`` at ``query_size`` with ``WARP_FAR`` where no surface is hit; the parts
        hold its entries.  ``None`` is the behaviour described above."""
        from . import compositing

        if depth_source not in (None, "fused"):
            raise _lib.IdhError(f"composite_asset: depth_source must be None or 'fused', got {depth_source!r}")
        fused = depth_source == "fused"
        depth_route = fused or self.hot.binary_mlp is None  # a DepthModel: no occlusion MLP to ask, its remembered depth maps are warped instead
        if fused and self._fusion is None:
            raise _lib.IdhError("composite_asset(depth_source='fused') needs start_fusion()")
        if (self._fused_maps == 0) if fused else (not self._depth_ring) if depth_route else (self._key is None):
            raise _lib.IdhError("no prediction has been made in this sequence yet (step() returned None so far)")
        if not isinstance(image_u8, torch.Tensor) or image_u8.dim() != 4 or image_u8.shape[0] != 1 or image_u8.shape[-1] != 3:
            raise _lib.IdhError("composite_asset: image_u8 must be one (1,H,W,3) uint8 frame on the GPU")
        if getattr(asset, "colors", None) is None:
            raise _lib.IdhError("composite_asset: the asset has no vertex colours (AssetRenderer(colors=...))")
        H, W = int(image_u8.shape[1]), int(image_u8.shape[2])
        h, w = (int(s) for s in (compositing.MODEL_SIZE if query_size is None else query_size))
        K = torch.as_tensor(K).to(device=image_u8.device, dtype=torch.float32).reshape(-1, 4, 4)[:1]
        K_query = K.clone()
        K_query[:, 0] *= w / W
        K_query[:, 1] *= h / H
        if depth_route:
            full = asset.render(world_T_cam, K, (H, W))  # composite_depth compares at the image's resolution
            if fused:
                v = self.fused_depth_for_view(world_T_cam, torch.linalg.inv(K_query), (h, w), empty_depth=self.WARP_FAR)
            else:
                v = self.warped_depth_for_view(world_T_cam, K_query, (h, w), empty_depth=self.WARP_FAR)
            frame = compositing.composite_depth(image_u8, v["view_fused_depth" if fused else "view_warp_depth"], virtual_depth=full["depth"][:, 0], virtual_rgba=full["rgba"],
                                                fade=fade, bgr=bgr)
            if return_parts:
                return {**v, "frame": frame, "asset_depth": full["depth"], "asset_rgba": full["rgba"]}
            return frame
        depth = asset.render(world_T_cam, K_query, (h, w))["depth"]  # -1 where the asset is not: no positive depth, so `fill` there
        rgba = asset.render(world_T_cam, K, (H, W))["rgba"]
        v = self.occlusion_for_view(depth, world_T_cam, torch.linalg.inv(K_query), fill=fill)
        frame = compositing.composite_mask(image_u8, v["view_pred"], virtual_rgba=rgba, fade=fade, bgr=bgr)
        if return_parts:
            return {**v, "frame": frame, "asset_depth": depth, "asset_rgba": rgba}
        return frame

    WARP_FAR = 1.0e4  # metres: the depth composite_asset's depth route gives the pixels no remembered map covers

    def remember_depth(self, depth_11hw: torch.Tensor, world_T_cam, invK: torch.Tensor, frame_u8: Optional[torch.Tensor] = None,
                       frame_K: Optional[torch.Tensor] = None) -> None:
        """Push a depth map (1,1,h,w) onto the ring of the last ``query_keyframes`` maps ``warped_depth_for_view`` draws: the camera that
        saw it at ``world_T_cam`` ((4,4) array or tensor) with inverse intrinsics ``invK`` ((4,4) or (1,4,4), at h x w).  ``step`` calls
        this with a ``DepthModel``'s ``depth_pred_s0_b1hw``; a caller pushes a lidar frame or a ``BDModel``'s inferred depth.  Taps that
        are not finite and positive are holes.  The map is copied; all maps of the ring have one size.  ``reset()`` empties the ring.
        ``frame_u8`` (1,Hf,Wf,3) uint8: the camera frame that belongs to the map, fused into the colours of the volume of
        ``start_fusion(color=True)`` (it is not kept); ``frame_K`` its intrinsics ((4,4) or (1,4,4)) at Hf x Wf, None: the inverse of
        ``invK`` with rows 0 and 1 scaled by Wf / w and Hf / h (``intrinsics_pyramid``'s rule).
        After ``start_fusion(track=...)``, and once a map has been fused, the map is first aligned against the volume starting from
        ``world_T_cam`` (``fusion.align_depth``) and, if the fit is accepted, the refined pose is the one the consistency
        check, the ring, the volume's follow-shift and the integration use; ``last_alignment`` says what happened.  This reads 16 floats
        and the fit's records back from the device (the session keeps poses in float64 on the host): one synchronisation per map."""
        from .raster import _pose_f64

        _lib.require_cuda_f32(depth_11hw, invK)
        if depth_11hw.dim() != 4 or tuple(depth_11hw.shape[:2]) != (1, 1) or depth_11hw.shape[2] < 2 or depth_11hw.shape[3] < 2:
            raise _lib.IdhError(f"remember_depth: depth {tuple(depth_11hw.shape)} must be (1,1,h,w) with h, w >= 2")
        if self._depth_ring and self._depth_ring[0][0].shape != depth_11hw.shape:
            raise _lib.IdhError(f"remember_depth: the ring holds maps of {tuple(self._depth_ring[0][0].shape)}, got {tuple(depth_11hw.shape)}")
        invK = invK.reshape(-1, 4, 4)
        if invK.shape[0] != 1:
            raise _lib.IdhError("remember_depth: invK must be (4,4) or (1,4,4)")
        pose = _pose_f64("world_T_cam", world_T_cam)
        if frame_u8 is None and frame_K is not None:
            raise _lib.IdhError("remember_depth: frame_K without frame_u8")
        if frame_u8 is not None:
            if self._fusion is None or not self._fusion["color"]:
                raise _lib.IdhError("remember_depth: a frame needs start_fusion(color=True)")
            if frame_u8.dtype != torch.uint8 or not frame_u8.is_cuda or frame_u8.dim() != 4 or frame_u8.shape[0] != 1 or frame_u8.shape[3] != 3:
                raise _lib.IdhError(f"remember_depth: frame_u8 {tuple(frame_u8.shape)} {frame_u8.dtype} must be uint8 (1,Hf,Wf,3) on the GPU")
            if frame_K is not None:
                _lib.require_cuda_f32(frame_K)
                frame_K = frame_K.reshape(-1, 4, 4)
                if frame_K.shape[0] != 1:
                    raise _lib.IdhError("remember_depth: frame_K must be (4,4) or (1,4,4)")
        if self._fusion is not None and self._fusion["track"] is not None and self._fused_maps > 0:
            pose = self._track(depth_11hw.detach(), pose, invK.detach())  # before the check, the ring, the follow-shift and the integrate
        checked = None
        if self._fusion is not None and self._fusion["consistency"] is not None:
            checked = self._check_depth(depth_11hw.detach(), pose, invK.detach())  # against the maps already in the ring
        self._depth_ring.insert(0, (depth_11hw.detach().clone(), pose, invK.detach().clone()))  # the raw map: the warp path is unchanged
        del self._depth_ring[self.query_keyframes:]
        if self._fusion is not None:
            if checked is None:
                self._fuse(self._depth_ring[0][0], pose, invK, frame_u8, frame_K)
            elif self._fusion["weighted"]:
                self._fuse(self._depth_ring[0][0], pose, invK, frame_u8, frame_K, weight=checked["weight"])
            else:
                self._fuse(checked["filtered_depth"], pose, invK, frame_u8, frame_K)

    def _fit_pose(self, depth_11hw: torch.Tensor, pose: np.ndarray, invK_144: torch.Tensor, kw: dict) -> Tuple[np.ndarray, dict]:
        """``fusion.align_depth`` of a map against the session's volume from ``pose``: the fitted pose in float64 on the host (the float32
        result widened) and ``fusion.alignment_summary`` of its records.  One device-to-host read of each."""
        from .fusion import align_depth, alignment_summary

        start = torch.from_numpy(pose.astype(np.float32)).to(depth_11hw.device)
        out = align_depth(self._volume, depth_11hw, invK_144, start, **kw)
        return out["world_T_cam"][0].cpu().numpy().astype(np.float64), alignment_summary(out["records"])

    def _track(self, depth_11hw: torch.Tensor, pose: np.ndarray, invK_144: torch.Tensor) -> np.ndarray:
        """The pose ``remember_depth`` goes on with: the fit's if it ended on a step (status 0, also when later iterations were skipped),
        counted at least ``min_count`` pixels and moved the camera by no more than ``max_correction``; else the caller's, bit for bit."""
        from .raster import _pose_f64

        kw = dict(self._fusion["track"])
        max_t, max_r = kw.pop("max_correction")
        fitted, summary = self._fit_pose(depth_11hw, pose, invK_144, kw)
        dt = float(np.linalg.norm(fitted[:3, 3] - pose[:3, 3]))
        M = fitted[:3, :3] @ pose[:3, :3].T
        dr = float(np.arctan2(0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]), (np.trace(M) - 1.0) / 2.0))
        ok = summary["status"] == 0 and summary["count"] >= kw.get("min_count", 64) and dt <= max_t and dr <= max_r and bool(np.isfinite(fitted).all())
        used = _pose_f64("world_T_cam", fitted) if ok else pose
        self.last_alignment = dict(summary=summary, given=pose.copy(), used=used.copy(), accepted=ok, translation=dt, rotation=dr)
        return used

    def align_pose(self, depth_11hw: torch.Tensor, world_T_cam, invK: torch.Tensor, **kw) -> Tuple[np.ndarray, dict]:
        """The fit of ``remember_depth``'s tracking for a map that is NOT remembered - the live camera between keyframes: ``(pose,
        summary)``, the fitted world_T_cam as a float64 (4,4) host array and ``fusion.alignment_summary`` of the fit, for the caller to
        judge.  ``kw``: the keywords of ``fusion.align_depth`` (default: those of ``start_fusion(track=)``, if given).  The ring, the
        volume and ``last_alignment`` are left as they are.  Needs ``start_fusion`` and a fused map; synchronises (two host reads)."""
        from .raster import _pose_f64

        if self._fusion is None or self._volume is None or self._fused_maps == 0:
            raise _lib.IdhError("align_pose needs start_fusion() and at least one fused map")
        _lib.require_cuda_f32(depth_11hw, invK)
        if depth_11hw.requires_grad or invK.requires_grad:
            raise _lib.IdhError("align_pose: inputs that require grad (the alignment is not differentiable)")
        invK = invK.reshape(-1, 4, 4)
        if invK.shape[0] != 1:
            raise _lib.IdhError("align_pose: invK must be (4,4) or (1,4,4)")
        base = dict(self._fusion["track"] or {})
        base.pop("max_correction", None)
        base.update(kw)
        return self._fit_pose(depth_11hw, _pose_f64("world_T_cam", world_T_cam), invK, base)

    def _check_depth(self, depth_11hw: torch.Tensor, pose: np.ndarray, invK_144: torch.Tensor) -> Optional[dict]:
        """``geometry.depth_consistency`` of a new map against the ring's maps (B = 1, K = their number, one launch), before the map is
        pushed; None for the first map of a sequence, which has nothing to be checked against.  Also keeps the new map's camera for the
        checks to come."""
        from .geometry import depth_consistency

        c, dev = self._fusion["consistency"], depth_11hw.device
        cams = self._ring_cams
        checked = None
        if self._depth_ring:
            K = len(self._depth_ring)
            checked = depth_consistency(depth_11hw, invK_144, torch.from_numpy(pose.astype(np.float32))[None].to(dev),
                                        torch.cat([d for d, _, _ in self._depth_ring])[None], torch.cat([k for k, _ in cams])[None],
                                        torch.cat([t for _, t in cams])[None], ratio=c["ratio"], log_tol=c["log_tol"],
                                        min_consistent=min(c["min_consistent"], K), max_conflict=c["max_conflict"])
            self.last_depth_counts = checked["counts"]
        cams.insert(0, (torch.linalg.inv(invK_144), torch.from_numpy(np.linalg.inv(pose).astype(np.float32))[None].to(dev)))
        del cams[self.query_keyframes:]
        return checked

    def start_fusion(self, voxel_size: float = 0.04, dims: Sequence[int] = (96, 256, 256), origin=None, trunc_voxels: float = 3.0,
                     max_weight: float = 64.0, color: bool = False, consistency: Optional[dict] = None, weighted: bool = False,
                     follow: Optional[float] = None, on_scroll=None, track: Optional[dict] = None) -> None:
        """From now on ``remember_depth`` - which ``step`` calls with a ``DepthModel``'s predictions - also averages the map it pushes
        into a TSDF volume of ``dims`` = (Nz, Ny, Nx) voxels of ``voxel_size`` metres (``fusion.TSDFVolume``), which
        ``fused_depth_for_view`` ray-casts: maps are combined, holes one map left are filled by another, and a map that has left the ring
        is still in the volume.  ``origin``: the world (x, y, z) of voxel (0,0,0)'s centre; None centres the grid on the camera position
        of the first map integrated.  ``reset()`` empties the volume and keeps its storage.  Calling it again starts a new volume.
        ``color=True`` gives the volume colours (16 more bytes per voxel): ``remember_depth`` and ``step`` then take the
        camera frame of a map, ``fused_depth_for_view(return_color=True)`` and ``fused_mesh(return_colors=True)`` return them.
        ``consistency``: a dict with any of ``log_tol`` (0.05), ``min_consistent`` (1), ``max_conflict`` (0) and ``ratio``
        (1.05), the parameters of ``geometry.depth_consistency``.  ``remember_depth`` then checks every new map against the maps already
        in the ring, in one launch, and fuses only the pixels enough of them agree with and too few contradict - flying pixels at depth
        discontinuities stay out of the volume; ``min_consistent`` is capped at the number of ring maps, and the first map of a sequence
        is fused as it is.  ``weighted=True`` fuses the raw map with the check's weight (0 for a rejected pixel, else 1 + the number of
        agreeing maps) instead of the filtered map with weight 1.  The ring keeps the raw map; ``last_depth_counts`` holds the counts of
        the last check.  Start fusion before the first map of a sequence: the check knows the cameras of the maps remembered since.
        ``follow``: None keeps the grid where the first map put it - what leaves it is not fused.  A slack in metres
        (> 0) lets the volume follow the camera: before a map is integrated, ``fusion.follow_shift`` is asked with the map's camera
        position, and once that is further than ``follow`` from the grid's centre on an axis the grid is moved back under it by whole
        8-voxel blocks (``TSDFVolume.shift``: what stays keeps its bits, what leaves is dropped, the volume holds twice its memory from
        the first move on).  ``on_scroll(volume, shift_xyz)`` is called just before such a move, with the volume still unshifted: the
        place to ``crop`` or mesh the ``fusion.leaving_boxes``.  ``fusion_scrolls`` counts the moves, ``last_scroll`` is the last one.
        ``track``: None trusts every pose as given.  A dict with any of the keywords of ``fusion.align_depth`` (``iters``,
        ``stride``, ``huber``, ``damping``, ``min_step``, ``min_count``, ``schedule``, ``min_pivot_ratio``) and ``max_correction`` =
        (metres, radians), default (0.1, 0.1): from the second map of a sequence on, ``remember_depth`` fits the new map's camera to the
        volume, starting from the caller's pose, before anything else is done with the map, and uses the fitted pose for the consistency
        check, the ring, the follow-shift and the integration - if the fit ended on a step, counted ``min_count`` pixels and stayed
        within ``max_correction``; otherwise the caller's pose is used as it is.  ``last_alignment`` holds "summary", "given", "used",
        "accepted" and the correction's "translation" / "rotation".  The fit converges from about a truncation distance away, not
        further.  The keyframe bank of ``step`` keeps the caller's pose: only the depth memory is corrected."""
        dims = tuple(int(d) for d in dims)
        if follow is not None and not float(follow) > 0:
            raise _lib.IdhError(f"start_fusion: follow = {follow} must be a positive slack in metres (None: a fixed grid)")
        if on_scroll is not None and (follow is None or not callable(on_scroll)):
            raise _lib.IdhError("start_fusion: on_scroll must be callable and needs follow")
        if weighted and consistency is None:
            raise _lib.IdhError("start_fusion: weighted=True needs consistency (the weights are the check's)")
        if consistency is not None:
            unknown = set(consistency) - {"log_tol", "min_consistent", "max_conflict", "ratio"}
            if unknown:
                raise _lib.IdhError(f"start_fusion: consistency has unknown keys {sorted(unknown)}")
            if self._depth_ring:
                raise _lib.IdhError("start_fusion(consistency=) must come before the first remembered map of a sequence (reset() first)")
            consistency = dict(log_tol=float(consistency.get("log_tol", 0.05)), min_consistent=int(consistency.get("min_consistent", 1)),
                               max_conflict=int(consistency.get("max_conflict", 0)), ratio=float(consistency.get("ratio", 1.05)))
        if track is not None:
            unknown = set(track) - {"iters", "stride", "huber", "damping", "min_step", "min_count", "schedule", "min_pivot_ratio", "max_correction"}
            if unknown:
                raise _lib.IdhError(f"start_fusion: track has unknown keys {sorted(unknown)}")
            track = dict(track)
            mc = tuple(float(x) for x in track.get("max_correction", (0.1, 0.1)))
            if len(mc) != 2 or not (mc[0] >= 0 and mc[1] >= 0):
                raise _lib.IdhError(f"start_fusion: track max_correction {mc} must be (metres, radians), both >= 0")
            track["max_correction"] = mc
        if len(dims) != 3 or min(dims) < 2 or not float(voxel_size) > 0:
            raise _lib.IdhError(f"start_fusion: dims {dims} must be three sizes >= 2 and voxel_size {voxel_size} positive")
        self._fusion = dict(voxel_size=float(voxel_size), dims=dims, origin=None if origin is None else tuple(float(o) for o in origin),
                            trunc_voxels=float(trunc_voxels), max_weight=float(max_weight), color=bool(color), consistency=consistency,
                            weighted=bool(weighted), follow=None if follow is None else float(follow), on_scroll=on_scroll, track=track)
        self._volume, self._fused_maps = None, 0
        self.fusion_scrolls, self.last_scroll = 0, None
        self._ring_cams, self.last_depth_counts = [], None
        self.last_alignment = None

    def _fuse(self, depth_11hw: torch.Tensor, pose: np.ndarray, invK_144: torch.Tensor, frame_u8: Optional[torch.Tensor] = None,
              frame_K_144: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None) -> None:
        from .fusion import TSDFVolume

        f = self._fusion
        if self._fused_maps == 0:
            origin = f["origin"]
            if origin is None:  # the camera sits at the centre of the grid
                nz, ny, nx = f["dims"]
                origin = tuple(pose[:3, 3] - f["voxel_size"] * 0.5 * (np.array([nx, ny, nz], dtype=np.float64) - 1.0))
            if self._volume is None:
                self._volume = TSDFVolume(f["dims"], f["voxel_size"], origin, f["trunc_voxels"], f["max_weight"], device=depth_11hw.device, color=f["color"])
            self._volume.origin = tuple(float(o) for o in origin)
        if f["follow"] is not None:  # the grid goes after the camera before the map is integrated
            from .fusion import follow_shift

            s = follow_shift(pose[:3, 3], self._volume.origin, f["dims"], f["voxel_size"], f["follow"])
            if any(s):
                if f["on_scroll"] is not None:
                    f["on_scroll"](self._volume, s)  # still unshifted: the caller keeps what is about to leave
                self._volume.shift(s)
                self.fusion_scrolls, self.last_scroll = self.fusion_scrolls + 1, s
        cam_T_world =torch.from_numpy(np.linalg.inv(pose).astype(np.float32))[None]  # inverted in float64 on the host
        K = torch.linalg.inv(invK_144)
        if frame_u8 is not None and frame_K_144 is None:
            frame_K_144 = K.clone()
            frame_K_144[:, 0] *= frame_u8.shape[2] / depth_11hw.shape[3]
            frame_K_144[:, 1] *= frame_u8.shape[1] / depth_11hw.shape[2]
        if weight is None:
            self._volume.integrate(depth_11hw, K, cam_T_world, frame_u8, frame_K_144)
        else:
            self._volume.integrate(depth_11hw, K, cam_T_world, frame_u8, frame_K_144, weight=weight)
        self._fused_maps += 1

    @property
    def fusion_volume(self):
        """The ``fusion.TSDFVolume`` of ``start_fusion`` (None before the first map)."""
        return self._volume

    def fused_depth_for_view(self, world_T_cam, invK: torch.Tensor, size: Sequence[int], near: float = 0.25, far: float = 8.0,
                             step_voxels: float = 1.0, empty_depth: float = -1.0, return_normals: bool = False,
                             return_color: bool = False) -> Dict[str, torch.Tensor]:
        """The fused surface in the LIVE camera, also on the frames where ``step`` returned None: the volume of ``start_fusion`` ray-cast
        into the ``size`` = (H, W) image of the camera at ``world_T_cam`` ((4,4) array or tensor; taken to float32 from float64 on the
        host) with inverse intrinsics ``invK`` ((4,4) or (1,4,4), at H x W) - ``TSDFVolume.raycast``, one launch.  Returns
        "view_fused_depth" (1,1,H,W): the camera's z of the first surface between ``near`` and ``far`` metres along each pixel's ray,
        ``empty_depth`` where "view_fused_valid" (1,1,H,W) bool is False; "view_fused_flags" (1,H,W) uint8 (``fusion.FLAG_*``: a ray
        without a hit crossed only unobserved space, partly observed space, or - flags 0 - observed free space); with
        ``return_normals`` "view_fused_normals" (1,3,H,W), unit normals in WORLD space that face the camera, zero where there is none;
        with ``return_color`` (``start_fusion(color=True)``) "view_fused_rgba" (1,H,W,4) uint8, the surface's fused colour with alpha
        255, four zero bytes where there is no hit or no colour."""
        from .raster import _pose_f64

        if self._fusion is None:
            raise _lib.IdhError("fused_depth_for_view needs start_fusion()")
        if return_color and not self._fusion["color"]:
            raise _lib.IdhError("fused_depth_for_view(return_color=True) needs start_fusion(color=True)")
        if self._fused_maps == 0:
            raise _lib.IdhError("no prediction has been made in this sequence yet and no depth map was remembered (remember_depth)")
        _lib.require_cuda_f32(invK)
        T = torch.from_numpy(_pose_f64("world_T_cam", world_T_cam).astype(np.float32))[None]
        out = self._volume.raycast(T, invK.reshape(-1, 4, 4)[:1], (int(size[0]), int(size[1])), near=near, far=far, step_voxels=step_voxels,
                                   empty_depth=empty_depth, return_normals=return_normals, world_normals=True, return_color=return_color)
        res = {"view_fused_depth": out["depth"], "view_fused_valid": ((out["flags"] & 1) != 0)[:, None], "view_fused_flags": out["flags"]}
        if return_normals:
            res["view_fused_normals"] = out["normals"]
        if return_color:
            res["view_fused_rgba"] = out["rgba"]
        return res

    def fused_mesh(self, min_weight: float = 0.0, return_colors: bool = False) -> Dict[str, torch.Tensor]:
        """The session's own reconstruction as a triangle mesh: ``fusion.extract_mesh`` of the volume of ``start_fusion`` - "verts"
        (V,3) float32 in the world, "faces" (F,3) int32, normals towards free space - as ``MeshDepthRasterizer.load_gt_mesh(verts=,
        faces=)``, ``evaluation.TemporalEvaluator``, ``raster.render_shaded`` and ``raster.save_ply`` take them.  ``min_weight`` keeps
        the cells whose eight voxels were observed more often than that.  ``return_colors`` (``start_fusion(color=True)``) adds
        "colors" (V,4) uint8, what ``render_shaded(colors=)`` and ``save_ply(colors=)`` take."""
        if self._fusion is None:
            raise _lib.IdhError("fused_mesh needs start_fusion()")
        if return_colors and not self._fusion["color"]:
            raise _lib.IdhError("fused_mesh(return_colors=True) needs start_fusion(color=True)")
        if self._fused_maps == 0:
            raise _lib.IdhError("no prediction has been made in this sequence yet and no depth map was remembered (remember_depth)")
        return self._volume.extract_mesh(min_weight=min_weight, return_colors=return_colors)

    def warped_depth_for_view(self, world_T_cam, K: torch.Tensor, size: Sequence[int], tear_ratio: float = 1.1, empty_depth: float = -1.0,
                              return_source: bool = False) -> Dict[str, torch.Tensor]:
        """The remembered depth maps in the LIVE camera, also on the frames where ``step`` returned None: every map of the ring drawn as a
        triangulated surface, torn where neighbouring taps differ by more than ``tear_ratio``, into the ``size`` = (H, W) image of the
        camera at ``world_T_cam`` ((4,4) array or tensor) with intrinsics ``K`` ((4,4) or (1,4,4), at H x W) - ``raster.warp_depth``, one
        call for all maps.  Returns "view_warp_depth" (1,1,H,W): the depth of the nearest remembered surface, ``empty_depth`` where
        "view_warp_valid" (1,1,H,W) bool is False (no map saw anything there); with ``return_source`` "view_warp_source" (1,H,W) int32
        (``raster.decode_source``; source 0 is the newest map).  No network runs and nothing is searched: one pass over the maps' pixels."""
        from . import raster

        if not self._depth_ring:
            raise _lib.IdhError("no prediction has been made in this sequence yet and no depth map was remembered (remember_depth)")
        depth = torch.cat([d for d, _, _ in self._depth_ring])
        invK = torch.cat([k for _, _, k in self._depth_ring])
        T = raster.relative_poses([world_T_cam], [p for _, p, _ in self._depth_ring]).to(depth.device)
        K = torch.as_tensor(K).to(device=depth.device, dtype=torch.float32).reshape(-1, 4, 4)[:1]
        out = raster.warp_depth(depth, invK, T, K, int(size[0]), int(size[1]), tear_ratio=tear_ratio, empty_depth=empty_depth, return_source=True)
        res = {"view_warp_depth": out["depth"], "view_warp_valid": (out["source"] >= 0)[:, None]}
        if return_source:
            res["view_warp_source"] = out["source"]
        return res

    def _key_order(self, T_host: torch.Tensor) -> list:
        """Ring slots of the remembered predictions, nearest pose to the live camera first (``nearest_keys_first``; host arithmetic)."""
        slots = self.hot._ring.slots_newest_first()
        order = nearest_keys_first(T_host.double().numpy(), [self._ring_poses[s] for s in slots])
        return [slots[i] for i in order]

    def _live_view(self, world_T_cam, invK: torch.Tensor, rays):
        """What the ray queries in the live camera share: the checks, the pose on the device, ``invK`` with a batch axis, and either the
        order of the remembered keys (``query_keyframes`` > 1) or the carried prior's inputs.  Returns (T (1,4,4), invK (1,4,4), order | None,
        prior_inputs | None)."""
        if self._key is None:
            raise _lib.IdhError("no prediction has been made in this sequence yet (step() returned None so far)")
        _lib.require_cuda_f32(invK, rays)
        T = torch.as_tensor(world_T_cam.detach().cpu().numpy() if isinstance(world_T_cam, torch.Tensor) else np.asarray(world_T_cam))
        if tuple(T.shape) != (4, 4):
            raise _lib.IdhError(f"world_T_cam {tuple(T.shape)} must be (4,4)")
        T_host = T
        T = T.to(device=invK.device, dtype=torch.float32)[None]
        if invK.dim() == 2:
            invK = invK[None]
        if self.query_keyframes > 1:
            return T, invK, self._key_order(T_host), None
        pi = None
        if self.use_prior and self._prior is not None:
            pi = {"prior_prediction": self._prior[0][:, :1], "prior_cam_T_world": self._prior[1]}
        return T, invK, None, pi

    def _view_search(self, world_T_cam, invK: torch.Tensor, size, rays, thresholder, fill: float):
        T, invK, order, pi = self._live_view(world_T_cam, invK, rays)
        k = self._key
        if order is not None:
            with torch.inference_mode():
                return self.hot.query_view_depths_keys(invK, T, size=size, rays=rays, order=order, thresholder=thresholder, fill=fill,
                                                       return_points=True)
        with torch.inference_mode():
            return self.hot.query_view_depths(invK, T, k["cam_T_world_b44"], k["K_s0_b44"], size=size, rays=rays, prior_inputs=pi,
                                              thresholder=thresholder, fill=fill, return_points=True)

    def depth_for_view(self, world_T_cam, invK: torch.Tensor, size: Sequence[int], thresholder=None, fill: float = 0.0) -> Dict[str, Optional[torch.Tensor]]:
        """A dense depth map of the LIVE camera, also on the frames where ``step`` returned None: for every pixel centre of the ``size`` =
        (h, w) image of the camera at ``world_T_cam`` - a (4,4) array or tensor - with inverse intrinsics ``invK`` ((4,4) or (1,4,4), at
        h x w; any resolution), the depth search along that pixel's ray against the LAST prediction's decoder features
        (``HotPath.query_view_depths``, one launch).  With ``use_prior`` the carried prior is sampled at every probe, as in
        ``occlusion_for_view``.  ``thresholder``: None = the model's.  Returns ``HotPath.query_view_depths``' dictionary with
        "view_search_points" (1,1,h,w,3) WORLD points; "view_search_flags" == 3 marks the pixels whose crossing lies inside the search
        range and whose probes all fell inside the keyframe's view.  The depth is where the live ray enters the region hidden from the
        KEYFRAME camera: the surface as far as both cameras see the same side of it."""
        return self._view_search(world_T_cam, invK, tuple(size), None, thresholder, fill)

    def raycast_view(self, rays: torch.Tensor, world_T_cam, invK: torch.Tensor, thresholder=None, fill: float = 0.0) -> Dict[str, Optional[torch.Tensor]]:
        """The hit test from the LIVE screen, also on the frames where ``step`` returned None: ``rays`` (1,N,2) are (x, y) in pixel-centre
        units of the camera at ``world_T_cam`` / ``invK`` (a tap at pixel (i, j) is (j + 0.5, i + 0.5)).  ``depth_for_view`` at those rays:
        "view_search_depths" (1,N) is the z-depth in the live camera, "view_search_points" (1,N,3) the WORLD hit points.  Unlike
        ``raycast``, the carried prior (``use_prior``) is sampled per probe: the probes move across the keyframe's image."""
        return self._view_search(world_T_cam, invK, None, rays, thresholder, fill)

    def _view_march(self, world_T_cam, invK: torch.Tensor, size, rays, thresholder, fill: float, march: dict):
        T, invK, order, pi = self._live_view(world_T_cam, invK, rays)
        k = self._key
        if order is not None:
            with torch.inference_mode():
                return self.hot.query_view_first_hit_keys(invK, T, size=size, rays=rays, order=order, thresholder=thresholder, fill=fill,
                                                          return_points=True, **march)
        with torch.inference_mode():
            return self.hot.query_view_first_hit(invK, T, k["cam_T_world_b44"], k["K_s0_b44"], size=size, rays=rays, prior_inputs=pi,
                                                 thresholder=thresholder, fill=fill, return_points=True, **march)

    def first_hit_for_view(self, world_T_cam, invK: torch.Tensor, size: Sequence[int], thresholder=None, fill: float = 0.0, samples=16,
                           lo: float = 0.5, hi: float = 8.0, spacing: str = "linear", refine: int = 8) -> Dict[str, Optional[torch.Tensor]]:
        """``depth_for_view`` without its one-crossing assumption, also on the frames where ``step`` returned None: every pixel's ray of the
        LIVE camera probes the shared depths ``samples`` (a float32 vector, or n with ``lo`` / ``hi`` / ``spacing``) in turn until the
        first probe that is behind the surface and bisects ``refine`` steps inside that bracket (``HotPath.query_view_first_hit``, one
        launch; with ``query_keyframes`` > 1 ``query_view_first_hit_keys`` against the remembered predictions, nearest pose first).  Where a
        live ray enters the region hidden from the keyframe, leaves it and enters it again, ``depth_for_view`` may return either crossing;
        this returns the first one, at the resolution of the samples.  Returns ``HotPath.query_view_first_hit``'s dictionary with
        "view_march_points" (1,1,h,w,3) WORLD points; "view_march_flags" == 3 marks the bracketed pixels whose probes all fell inside the
        keyframe's view, "view_march_hit_step" == 255 those without a hit."""
        return self._view_march(world_T_cam, invK, tuple(size), None, thresholder, fill,
                                dict(samples=samples, lo=lo, hi=hi, spacing=spacing, refine=refine))

    def raycast_first_hit(self, rays: torch.Tensor, world_T_cam, invK: torch.Tensor, thresholder=None, fill: float = 0.0, samples=16,
                          lo: float = 0.5, hi: float = 8.0, spacing: str = "linear", refine: int = 8) -> Dict[str, Optional[torch.Tensor]]:
        """The hit test from the LIVE screen that returns the FIRST surface along the ray: ``first_hit_for_view`` at ``rays`` (1,N,2), (x, y)
        in pixel-centre units of the camera at ``world_T_cam`` / ``invK`` as in ``raycast_view``.  "view_march_depths" (1,N) is the z-depth in
        the live camera, "view_march_points" (1,N,3) the WORLD hit points."""
        return self._view_march(world_T_cam, invK, None, rays, thresholder, fill,
                                dict(samples=samples, lo=lo, hi=hi, spacing=spacing, refine=refine))

    def normals_for_view(self, world_T_cam, invK: torch.Tensor, size: Sequence[int], thresholder=None, fill: float = 0.0,
                         smoothing_kernel_size: int = 5, smoothing_kernel_std: float = 2.0,
                         first_hit: Optional[dict] = None) -> Dict[str, Optional[torch.Tensor]]:
        """The orientation of the surface in the LIVE camera, also on the frames where ``step`` returned None: ``depth_for_view`` - or, with
        ``first_hit`` a dictionary of ``first_hit_for_view``'s march arguments (``samples``, ``lo``, ``hi``, ``spacing``, ``refine``; ``{}`` for
        its defaults), that search - followed by ``geometry.depth_normals`` on its depth map with the search's flags (``need = 3``: a normal
        is valid iff every depth in its footprint is a trustworthy one, so ``fill`` never enters a valid normal), the rotation of
        ``world_T_cam`` and ``orient=True``.  Returns the search's dictionary plus "view_normals" (1,3,h,w): unit normals in WORLD space that
        face the live camera, (0,0,0) where "view_normals_valid" (1,1,h,w) uint8 is 0.  ``smoothing_kernel_size`` in {1,3,5,7} and
        ``smoothing_kernel_std`` are the reference ``NormalGenerator``'s (utils/geometry_utils.py:92-138)."""
        from .geometry import depth_normals

        if first_hit is None:
            out, pre = self.depth_for_view(world_T_cam, invK, size, thresholder, fill), "view_search"
        else:
            out, pre = self.first_hit_for_view(world_T_cam, invK, size, thresholder, fill, **first_hit), "view_march"
        T, invK, _, _ = self._live_view(world_T_cam, invK, None)
        with torch.inference_mode():
            normals, valid = depth_normals(out[pre + "_depths"], invK, kernel_size=smoothing_kernel_size, std=smoothing_kernel_std,
                                           world_R_cam=T[:, :3, :3], orient=True, flags=out[pre + "_flags"], need=3)
        out["view_normals"], out["view_normals_valid"] = normals, valid
        return out

    def raycast_view_normals(self, rays: torch.Tensor, world_T_cam, invK: torch.Tensor, step: float = 1.0, thresholder=None,
                             fill: float = 0.0) -> Dict[str, Optional[torch.Tensor]]:
        """The hit test from the LIVE screen with the orientation of the surface at the hit: every ray of ``rays`` (1,N,2) becomes a 3x3
        patch of rays ``step`` pixels apart (``patch_rays``: (1,9N,2), patch-major, row-major inside a patch), ONE ``raycast_view`` launch
        answers all of them, and ``geometry.patch_normals`` turns each patch's nine WORLD points and flags into "view_normals" (1,N,3) -
        facing the live camera - and "view_normals_valid" (1,N) uint8 (all nine rays bracketed, flags == 3; else (0,0,0)).  The other
        entries are ``raycast_view``'s for the centre rays, sliced out of the 9N answers.  Building an anchor pose from point and normal is
        the caller's."""
        from .geometry import patch_normals

        _lib.require_cuda_f32(rays)
        if rays.dim() != 3 or rays.shape[0] != 1 or rays.shape[2] != 2:
            raise _lib.IdhError(f"rays {tuple(rays.shape)} must be (1,N,2)")
        N = rays.shape[1]
        res = self._view_search(world_T_cam, invK, None, patch_rays(rays, step), thresholder, fill)
        T, _, _, _ = self._live_view(world_T_cam, invK, rays)
        with torch.inference_mode():
            normals, valid = patch_normals(res["view_search_points"].view(1, N, 9, 3), cam_centre=T[:, :3, 3], orient=True,
                                           flags=res["view_search_flags"].view(1, N, 9), need=3)
        out = {k: (v if v is None else v.view(1, N, 9, *v.shape[2:])[:, :, 4].contiguous()) for k, v in res.items()}
        out["view_normals"], out["view_normals_valid"] = normals, valid
        return out

    def raycast(self, rays: torch.Tensor, thresholder=None) -> Dict[str, torch.Tensor]:
        """The hit test: where rays (1,N,2) - (x, y) in pixel-centre units of the keyframe's scale-0 map - meet the scene, against the LAST
        prediction's decoder features, also on the frames where ``step`` returned None.  ``HotPath.query_ray_depths`` with the keyframe's
        ``invK_s0`` and ``world_T_cam``: "ray_points" are WORLD points, "ray_hit" == 3 marks the rays whose surface lies inside the search
        range.  ``thresholder``: None = the model's.  With ``use_prior`` the network sees the constant -1 in its prior channel, as the
        reference does where no prior prediction exists (bd_model.py:433-434): the carried prior is a dense map of the PREVIOUS
        prediction in the keyframe's view, not a per-ray value."""
        if self._key is None:
            raise _lib.IdhError("no prediction has been made in this sequence yet (step() returned None so far)")
        _lib.require_cuda_f32(rays)
        k = self._key
        with torch.inference_mode():
            return self.hot.query_ray_depths(rays, thresholder=thresholder, invK_s0_b44=k["invK_s0_b44"], world_T_cam_b44=k["world_T_cam_b44"])
