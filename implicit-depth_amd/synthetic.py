"""Deterministic synthetic inputs and weights for the cost-volume hot path.

Nothing here comes from the reference; it reproduces the *shapes and statistics* the
reference's data pipeline would hand to ``BDModel.forward``:

* matching features ~ N(0,1) (the real encoder ends in InstanceNorm,
  reference ``modules/networks.py:283``),
* ScanNet-shaped pin-hole intrinsics (fx=fy=577.87, cx=319.5, cy=239.5 at 640x480,
  reference ``datasets/scannet_dataset.py:466-486``) rescaled to the requested size,
* DVMVS-like source poses: translation (0.1(k+1), 0.02k, 0.01k) m and a y-rotation of
  0.03(k+1) rad for source view k,
* weights drawn per parameter *name* (so a reference module and its drop-in twin get
  bit-identical tensors without shipping a state_dict).

numpy's PCG64 is used instead of torch's generator so the streams are stable across
torch versions and identical on the CPU container and the GPU box.
"""
from __future__ import annotations

import math
import zlib
from typing import Dict, Iterable, Tuple

import numpy as np
import torch


def _rng(seed: int, tag: str = "") -> np.random.Generator:
    return np.random.Generator(np.random.PCG64([seed & 0xFFFFFFFF, zlib.crc32(tag.encode())]))


def randn(shape, seed: int, tag: str = "", dtype=torch.float32) -> torch.Tensor:
    a = _rng(seed, tag).standard_normal(size=tuple(shape), dtype=np.float32)
    return torch.from_numpy(a).to(dtype)


def intrinsics(width: int, height: int) -> torch.Tensor:
    """4x4 pin-hole K for an image of ``width x height`` pixels (ScanNet-shaped)."""
    K = torch.eye(4, dtype=torch.float64)
    K[0, 0] = 577.87 * width / 640.0
    K[1, 1] = 577.87 * height / 480.0
    K[0, 2] = 319.5 * width / 640.0
    K[1, 2] = 239.5 * height / 480.0
    return K


def _rot_y(theta: float) -> torch.Tensor:
    c, s = math.cos(theta), math.sin(theta)
    R = torch.eye(4, dtype=torch.float64)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = c, s, -s, c
    return R


def source_pose(k: int, behind: bool = False, big_rotation: bool = False) -> torch.Tensor:
    """cur_T_src (source camera pose expressed in the current camera frame), 4x4 fp64."""
    T = _rot_y(0.03 * (k + 1))
    if big_rotation:
        T = _rot_y(0.6)
    if behind:
        # camera looking back at the current camera from far in front of it: every
        # back-projected point lies behind this view (exercises the z<=eps clamp).
        T = _rot_y(math.pi)
        T[2, 3] = 12.0
    T[0, 3] += 0.1 * (k + 1)
    T[1, 3] += 0.02 * k
    T[2, 3] += 0.01 * k
    return T


def cost_volume_inputs(
    B: int,
    K: int,
    C: int,
    H: int,
    W: int,
    seed: int = 0,
    behind_view: int = -1,
    big_rotation_view: int = -1,
    dtype=torch.float32,
) -> Dict[str, torch.Tensor]:
    """Inputs of ``CostVolumeManager.forward`` (reference ``modules/cost_volume.py:324``)."""
    cur = randn((B, C, H, W), seed, "cur_feats")
    src = randn((B, K, C, H, W), seed, "src_feats")
    Kmat = intrinsics(W, H)
    invK = torch.linalg.inv(Kmat)
    poses = torch.stack(
        [source_pose(k, behind=(k == behind_view), big_rotation=(k == big_rotation_view)) for k in range(K)]
    )
    # small per-batch perturbation so batch elements are not copies of each other
    poses_b = []
    for b in range(B):
        P = poses.clone()
        P[:, 0, 3] += 0.013 * b
        P[:, 1, 3] -= 0.007 * b
        poses_b.append(P)
    src_poses = torch.stack(poses_b)  # B,K,4,4  (src -> cur)
    src_extr = torch.linalg.inv(src_poses)  # cur -> src
    return {
        "cur_feats": cur.to(dtype),
        "src_feats": src.to(dtype),
        "src_extrinsics": src_extr.to(dtype),
        "src_poses": src_poses.to(dtype),
        "src_Ks": Kmat.expand(B, K, 4, 4).contiguous().to(dtype),
        "cur_invK": invK.expand(B, 4, 4).contiguous().to(dtype),
        "min_depth": torch.tensor(0.25, dtype=dtype).view(1, 1, 1, 1),
        "max_depth": torch.tensor(5.0, dtype=dtype).view(1, 1, 1, 1),
    }


def fill_state_dict(module: torch.nn.Module, seed: int = 0, gain: float = 1.0) -> None:
    """Deterministically (re)initialise every parameter of ``module`` from its *name*.

    Weights ~ N(0, gain^2/fan_in), biases ~ N(0, 0.05^2): activations stay O(1) through the
    deep residual stacks, so parity errors are not hidden by vanishing/exploding scales.
    """
    with torch.no_grad():
        for name, p in module.state_dict().items():
            if not torch.is_floating_point(p) or p.ndim == 0:
                continue
            if name.endswith("weight") and p.ndim >= 2:
                fan_in = int(np.prod(p.shape[1:]))
                w = randn(p.shape, seed, name) * (gain / math.sqrt(fan_in))
                p.copy_(w.to(p.dtype))
            elif name.endswith("bias"):
                p.copy_((randn(p.shape, seed, name) * 0.05).to(p.dtype))


def encoder_pyramid(
    B: int, img_h: int, img_w: int, seed: int = 0, channels: Iterable[int] = (24, 48, 64, 160, 256)
) -> Tuple[torch.Tensor, ...]:
    """Stand-in for the third-party image encoder's 5 feature maps (strides 2..32).

    timm's tf_efficientnetv2_s is not in the reference tree nor in this image
    (SURVEY.md §8c); only its output *shapes* (reference ``bd_model.py:47-51``) matter here.
    """
    outs = []
    for lvl, ch in enumerate(channels):
        s = 2 ** (lvl + 1)
        outs.append(randn((B, ch, img_h // s, img_w // s), seed, f"enc{lvl}") * 0.5)
    return tuple(outs)


def layer1_maps(B: int, K: int, H: int, W: int, seed: int = 0, channels: int = 64) -> torch.Tensor:
    """Stand-in for the matching backbone's output — conv1/bn1/relu/maxpool/layer1 of the third-party antialiased
    ResNet18 (reference ``modules/networks.py:262-268``): (B, K+1, 64, H, W), frame b's current image followed by its
    K source images (``bd_model.py:149-152``); non-negative like the ReLU-terminated residual block it replaces."""
    return torch.relu(randn((B, K + 1, channels, H, W), seed, "layer1"))


def rendered_depth_planes(B: int, H: int, W: int, P: int = 8) -> torch.Tensor:
    """P fronto-parallel query planes 1.5..5.0 m (reference ``generic_mvs_dataset.py:242``)."""
    d = torch.linspace(1.5, 5.0, P).view(1, P, 1, 1)
    return d.expand(B, P, H, W).contiguous()


class _FeatureInfo:
    def __init__(self, ch):
        self._ch = list(ch)

    def channels(self):
        return list(self._ch)


class StubImageEncoder(torch.nn.Module):
    """Random-init 5-level strided-conv pyramid with the output channels/strides of the
    reference's timm ``tf_efficientnetv2_s`` feature extractor (bd_model.py:47-51).  NOT the
    third-party network — a stand-in so that whole-model plumbing can run on both sides of a
    comparison with identical inputs to the hot path."""

    def __init__(self, channels=(24, 48, 64, 160, 256)):
        super().__init__()
        self._channels = list(channels)
        self.stages = torch.nn.ModuleList()
        cin = 3
        for c in channels:
            self.stages.append(torch.nn.Conv2d(cin, c, 3, 2, 1))
            cin = c
        self.feature_info = _FeatureInfo(self._channels)

    def forward(self, x):
        outs = []
        for st in self.stages:
            x = torch.tanh(st(x))
            outs.append(x)
        return outs


class StubResnetStem(torch.nn.Module):
    """Stand-in for antialiased_cnns.resnet18's conv1/bn1/relu/maxpool/layer1 (64 ch @ 1/4 res)."""

    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, 64, 7, 2, 3)
        self.bn1 = torch.nn.Identity()
        self.relu = torch.nn.ReLU()
        self.maxpool = torch.nn.MaxPool2d(3, 2, 1)
        self.layer1 = torch.nn.Conv2d(64, 64, 3, 1, 1)


def frame_tuple(B: int, K: int, img_h: int, img_w: int, seed: int = 0, P: int = 8):
    """cur_data / src_data dictionaries with the keys BDModel.forward reads
    (bd_model.py:186-194, :266-299; produced by generic_mvs_dataset.py:742-809)."""
    Hm, Wm = img_h // 4, img_w // 4
    cvi = cost_volume_inputs(B, K, 16, Hm, Wm, seed)
    cur_pose = torch.eye(4).expand(B, 4, 4).contiguous()  # world = current camera
    src_world_T_cam = cvi["src_poses"]  # src -> world(=cur)
    K1 = intrinsics(Wm, Hm).float()
    K0 = intrinsics(img_w // 2, img_h // 2).float()
    cur = {
        "image_b3hw": randn((B, 3, img_h, img_w), seed, "cur_img"),
        "K_s1_b44": K1.expand(B, 4, 4).contiguous(), "invK_s1_b44": torch.linalg.inv(K1).expand(B, 4, 4).contiguous(),
        "K_s0_b44": K0.expand(B, 4, 4).contiguous(), "invK_s0_b44": torch.linalg.inv(K0).expand(B, 4, 4).contiguous(),
        "cam_T_world_b44": cur_pose.clone(), "world_T_cam_b44": cur_pose.clone(),
        "rendered_depth": rendered_depth_planes(B, img_h // 2, img_w // 2, P),
    }
    src = {
        "image_b3hw": randn((B, K, 3, img_h, img_w), seed, "src_img"),
        "K_s1_b44": K1.expand(B, K, 4, 4).contiguous(), "invK_s1_b44": torch.linalg.inv(K1).expand(B, K, 4, 4).contiguous(),
        "cam_T_world_b44": torch.linalg.inv(src_world_T_cam), "world_T_cam_b44": src_world_T_cam.clone(),
    }
    return cur, src


def temporal_frame(t: int, K: int, img_h: int, img_w: int, seed: int = 0):
    """Frame ``t`` of a synthetic temporal sequence (BASELINE.json config 5; the loop of reference
    ``inference/inference.py:106-157`` with the ``plane_2.0`` asset): the camera drifts along x and pans about y, the K
    source views keep the DVMVS-like relative poses of ``frame_tuple``, the query is ONE fronto-parallel plane at 2 m
    (``:128-130``), feature maps are re-drawn per frame.  Returns (cur, src, layer1 maps (1,K+1,64,h/4,w/4), encoder
    pyramid).  The prior (previous prediction + previous cam_T_world) is carried by the caller."""
    cur, src = frame_tuple(1, K, img_h, img_w, seed=seed, P=1)
    world_T_cam = _rot_y(0.01 * t)
    world_T_cam[0, 3] = 0.05 * t
    world_T_cam[2, 3] = 0.01 * t
    world_T_cam = world_T_cam.float()[None]
    src_world_T_cam = world_T_cam.unsqueeze(1) @ src["world_T_cam_b44"]  # world <- cur <- src
    cur["world_T_cam_b44"], cur["cam_T_world_b44"] = world_T_cam, torch.linalg.inv(world_T_cam)
    src["world_T_cam_b44"], src["cam_T_world_b44"] = src_world_T_cam, torch.linalg.inv(src_world_T_cam)
    cur["rendered_depth"] = torch.full((1, 1, img_h // 2, img_w // 2), 2.0)
    l1 = layer1_maps(1, K, img_h // 4, img_w // 4, seed=1000 + 7 * t + seed)
    pyr = encoder_pyramid(1, img_h, img_w, seed=2000 + 7 * t + seed)
    return cur, src, l1, pyr


def custom_depth_planes(B: int, D: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """A caller-supplied ``depth_planes_bdhw`` (reference ``modules/cost_volume.py:324-347``): per-pixel planes —
    linearly spaced 0.4..4.5 m, tilted across the image and jittered per batch element — unlike the log-spaced,
    image-constant planes ``generate_depth_planes`` makes."""
    base = torch.linspace(0.4, 4.5, D).view(1, D, 1, 1)
    ys = torch.linspace(-1, 1, H).view(1, 1, H, 1)
    xs = torch.linspace(-1, 1, W).view(1, 1, 1, W)
    b = torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    return (base * (1.0 + 0.08 * xs - 0.05 * ys + 0.03 * b) + 0.01 * torch.sigmoid(randn((B, D, H, W), seed, "planes"))).contiguous()


def smooth_field(shape, seed: int, tag: str = "", cells=(6, 8)) -> np.ndarray:
    """A smooth (..., H, W) float64 field: the bilinear blend of a coarse (cells + 1) standard-normal grid.  Basic arithmetic
    only, so every host computes the same bits (thresholded masks of it can then be compared bit for bit)."""
    *lead, H, W = shape
    ch, cw = cells
    g = _rng(seed, tag).standard_normal(size=(*lead, ch + 1, cw + 1))
    y = np.arange(H, dtype=np.float64) * (ch / max(H - 1, 1))
    x = np.arange(W, dtype=np.float64) * (cw / max(W - 1, 1))
    y0 = np.minimum(np.floor(y).astype(np.int64), ch - 1)
    x0 = np.minimum(np.floor(x).astype(np.int64), cw - 1)
    fy, fx = (y - y0)[:, None], (x - x0)[None, :]
    Y, X = y0[:, None], x0[None, :]
    return (1 - fy) * ((1 - fx) * g[..., Y, X] + fx * g[..., Y, X + 1]) + fy * ((1 - fx) * g[..., Y + 1, X] + fx * g[..., Y + 1, X + 1])


def eval_frame_case(B: int, P: int, h: int, w: int, H: int, W: int, seed: int = 0):
    """(outputs, cur_data) for one test batch of reference test_bd.py / test_reg.py's evaluation block (:185-318 / :189-268):
    model-resolution ``depth_b1hw`` (with NaN and zero patches), ``rendered_depth`` (B, P, h, w) query planes 1.5..5 m with a
    smooth relief, full-resolution ``full_res_depth_b1hw`` (with zero and NaN patches), and the outputs ``pred_0`` (logits),
    ``search_depths`` and ``depth_pred_s0_b1hw``.  Basic float64 arithmetic, cast once to float32: identical on every host."""
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    depth = np.maximum(2.8 + 1.2 * smooth_field((B, 1, h, w), seed, "eval_depth"), 0.3)
    depth[:, :, h // 4: h // 4 + 5, w // 3: w // 3 + 9] = np.nan
    depth[:, :, -6:, :8] = 0.0
    planes = 1.5 + (3.5 / max(P - 1, 1)) * np.arange(P, dtype=np.float64) if P > 1 else np.array([2.5])
    rendered = planes.reshape(1, P, 1, 1) * (1.0 + 0.04 * smooth_field((B, P, h, w), seed, "eval_rendered"))
    gt = np.maximum(2.8 + 1.2 * smooth_field((B, 1, H, W), seed, "eval_gt") + 0.02 * _rng(seed, "eval_gt_noise").standard_normal((B, 1, H, W)), 0.3)
    gt[:, :, : H // 8, -(W // 6):] = 0.0
    gt[:, :, H // 2: H // 2 + 7, W // 2: W // 2 + 11] = np.nan
    logits = 2.0 * smooth_field((B, P, h, w), seed, "eval_logits", cells=(12, 16)) + 0.5 * _rng(seed, "eval_logits_noise").standard_normal((B, P, h, w))
    search = np.maximum(2.8 + 1.2 * smooth_field((B, 1, h, w), seed, "eval_search") + 0.05 * _rng(seed, "eval_search_noise").standard_normal((B, 1, h, w)), 0.25)
    dpred = np.maximum(2.8 + 1.2 * smooth_field((B, 1, h, w), seed, "eval_dpred") + 0.05 * _rng(seed, "eval_dpred_noise").standard_normal((B, 1, h, w)), 0.25)
    outputs = {"pred_0": f32(logits), "search_depths": f32(search), "depth_pred_s0_b1hw": f32(dpred)}
    cur = {"depth_b1hw": f32(depth), "rendered_depth": f32(rendered), "full_res_depth_b1hw": f32(gt)}
    return outputs, cur


def composite_case(B: int, h: int, w: int, H: int, W: int, seed: int = 0, render_hw: Tuple[int, int] | None = None):
    """Inputs of the AR compositing path (reference inference/inference.py:117-128, inference/composite.py:75-143) for B frames with a
    (h, w) model map and a (H, W) camera image.  Basic float64 arithmetic and PCG64 integers, cast once: identical on every host.
      image          uint8 (B,H,W,3) camera image
      rgba           uint8 (B,H,W,4) render of the asset: alpha exactly 0, exactly 255 and mixed regions
      logits         float32 (B,1,h,w) smooth occlusion logits with saturated patches (+-40)
      prob           float32 (B,1,h,w) occlusion probabilities clip(0.5 + 0.2 * logits, 0, 1): no transcendental, the same bits everywhere
      depth          float32 (B,1,h,w) regressed depth around the asset's
      virtual_depth  float32 (B,H,W) depth of the render, 0 where alpha is 0 (no asset)
      render         float32 (B,1,Hr,Wr) full-resolution asset depth for the preparation step (Hr, Wr = render_hw, default (2h+2, 2w+6)):
                     0 = no asset, with holes on every border and corner, isolated one-pixel holes and one 9 x 11 hole whose centre
                     stays 0 after the 7x7 fill."""
    u8 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    image = _rng(seed, "comp_image").integers(0, 256, size=(B, H, W, 3))
    alpha = np.clip(np.floor(255.0 * (0.5 + 0.9 * smooth_field((B, H, W), seed, "comp_alpha", cells=(3, 4))) + 0.5), 0, 255)
    alpha[:, : max(H // 6, 1), : max(W // 5, 1)] = 0
    alpha[:, H // 2: H // 2 + max(H // 6, 1), W // 2: W // 2 + max(W // 5, 1)] = 255
    rgba = np.concatenate([_rng(seed, "comp_rgb").integers(0, 256, size=(B, H, W, 3)), alpha[..., None]], -1)
    # moderate amplitude: outside the two patches sigmoid(2.5 * logit) stays away from exactly 0 and 1, where a blend lands on an integer
    logits = 1.2 * smooth_field((B, 1, h, w), seed, "comp_logits", cells=(4, 5)) + 0.3 * _rng(seed, "comp_logits_noise").standard_normal((B, 1, h, w))
    ph, pw = max(h // 8, 1), max(w // 10, 1)
    logits[:, :, h // 3: h // 3 + ph, w // 4: w // 4 + pw] = 40.0
    logits[:, :, 2 * h // 3: 2 * h // 3 + ph, 2 * w // 3: 2 * w // 3 + pw] = -40.0
    vdepth = 2.0 + 0.5 * smooth_field((B, H, W), seed, "comp_vdepth", cells=(3, 4))
    vdepth[alpha == 0] = 0.0
    depth = np.maximum(2.0 + 0.6 * smooth_field((B, 1, h, w), seed, "comp_depth", cells=(4, 5)) + 0.03 * _rng(seed, "comp_depth_noise").standard_normal((B, 1, h, w)), 0.25)
    Hr, Wr = render_hw if render_hw is not None else (2 * h + 2, 2 * w + 6)
    render = 1.5 + 0.5 * smooth_field((B, 1, Hr, Wr), seed, "comp_render", cells=(3, 4)) + 0.01 * _rng(seed, "comp_render_noise").standard_normal((B, 1, Hr, Wr))
    render[smooth_field((B, 1, Hr, Wr), seed, "comp_render_holes", cells=(3, 4)) > 0.9] = 0.0
    render[..., :2, :3] = render[..., :3, -2:] = render[..., -2:, :2] = render[..., -3:, -3:] = 0.0  # corners
    render[..., 0, Wr // 2: Wr // 2 + 4] = render[..., -1, Wr // 3: Wr // 3 + 2] = 0.0  # top / bottom border
    render[..., Hr // 2: Hr // 2 + 3, 0] = render[..., Hr // 3: Hr // 3 + 2, -1] = 0.0  # left / right border
    ys, xs = _rng(seed, "comp_render_dots").integers(0, Hr, size=12), _rng(seed, "comp_render_dots_x").integers(0, Wr, size=12)
    render[..., ys, xs] = 0.0  # isolated pixels
    y0, x0 = (Hr - 9) // 2, (Wr - 11) // 2
    render[..., y0: y0 + 9, x0: x0 + 11] = 0.0  # larger than the 7x7 window: the centre stays 0
    return {"image": u8(image), "rgba": u8(rgba), "logits": f32(logits), "prob": f32(np.clip(0.5 + 0.2 * logits, 0.0, 1.0)), "depth": f32(depth), "virtual_depth": f32(vdepth), "render": f32(render)}


# ---- temporal evaluation: meshes, cameras, vertex histories (raster.py, evaluation.TemporalEvaluator) ----------------------
def pinhole(fx: float, fy: float, cx: float, cy: float) -> torch.Tensor:
    K = torch.eye(4, dtype=torch.float64)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return K


def plane_pose(i: int) -> torch.Tensor:
    """world_T_cam (1,4,4) float32 of the camera a query plane is created from (pose 0: the world frame)."""
    T = _rot_y(0.2 * i)
    T[0, 3], T[1, 3], T[2, 3] = 0.3 * i, -0.1 * i, 0.05 * i
    return T.float()[None]


def vertex_histories(T: int, V: int, seed: int = 0) -> torch.Tensor:
    """(T,V) stacked per-frame vertex predictions as update_gt_vertex_predictions leaves them: probabilities, -1 where a vertex
    was not seen, and a share of exact 0.5 / 0 / 1 values."""
    r = _rng(seed, "vertex_hist")
    p = r.random((T, V), dtype=np.float32)
    kind = r.integers(0, 10, (T, V))
    p[kind == 0] = -1.0
    p[kind == 1] = 0.5
    p[kind == 2] = 0.0
    p[kind == 3] = 1.0
    return torch.from_numpy(p)


def _grid_faces(n: int, m: int, flip_every_other: bool = True) -> np.ndarray:
    """Two triangles per cell of an (n+1) x (m+1) vertex grid; with ``flip_every_other`` the second of each pair is wound the other way."""
    idx = (np.arange(n)[:, None] * (m + 1) + np.arange(m)[None, :]).reshape(-1)
    a, b, c, d = idx, idx + 1, idx + m + 1, idx + m + 2
    t1 = np.stack([a, d, c], 1)
    t2 = np.stack([a, d, b] if flip_every_other else [a, b, d], 1)
    return np.concatenate([t1, t2], 0).astype(np.int64)


def raster_scene(height: int, width: int, seed: int = 0, cells: int = 64, K: torch.Tensor | None = None, span_x=(-0.1, 0.85), span_y=(-0.1, 1.1)):
    """A mesh and two cameras for the rasteriser's tests: a noisy height field of ``cells`` x ``cells`` cells about 2.5 m in front of
    camera 0 spanning ``span_x`` x ``span_y`` of the image (every second triangle wound the other way), three near-camera triangles spanning large parts of the image, triangles
    that straddle z = 0, and triangles that must draw nothing (wholly behind, off screen, repeated index, collinear corners).
    Returns verts (V,3) float32, faces (F,3) int64, cam_T_world (2,4,4) and K (2,4,4) float32."""
    Km = (intrinsics(width, height) if K is None else K).double()
    fx, fy, cx, cy = float(Km[0, 0]), float(Km[1, 1]), float(Km[0, 2]), float(Km[1, 2])
    r = _rng(seed, "raster_scene")
    n = cells
    gy, gx = np.meshgrid(np.linspace(*span_y, n + 1), np.linspace(*span_x, n + 1), indexing="ij")  # in image widths / heights; the default leaves the right partly empty
    z = 2.5 + 0.3 * smooth_field((n + 1, n + 1), seed, "raster_relief") + 0.02 * r.standard_normal((n + 1, n + 1))
    jit = 0.2 / n * (r.random((2, n + 1, n + 1)) - 0.5)
    x = ((gx + jit[0]) * width - cx) / fx * z
    y = ((gy + jit[1]) * height - cy) / fy * z
    field = np.stack([x, y, z], -1).reshape(-1, 3)
    faces = [_grid_faces(n, n)]
    extra, ef = [], []

    def tri(p, q, s):
        base = len(field) + len(extra)
        extra.extend([p, q, s])
        ef.append([base, base + 1, base + 2])

    ray = lambda u, v, zz: [(u * width - cx) / fx * zz, (v * height - cy) / fy * zz, zz]
    # near-camera triangles over large parts of the image
    tri(ray(-0.2, 0.03, 0.7), ray(0.93, 0.11, 0.9), ray(0.41, 0.62, 0.6))
    tri(ray(0.07, 0.97, 0.8), ray(0.52, 0.35, 1.0), ray(1.3, 1.1, 0.75))
    tri(ray(0.61, 0.04, 1.1), ray(0.97, 0.83, 0.65), ray(0.78, 0.9, 0.95))
    # straddling z = 0: one corner behind, two corners behind
    tri(ray(0.13, 0.71, 1.4), ray(0.37, 0.93, 1.2), [0.3, 0.2, -0.6])
    tri(ray(0.88, 0.21, 1.3), [-0.4, 0.1, -0.3], [0.5, -0.6, -0.8])
    tri([0.9, -0.7, 0.4], [1.2, 0.9, -0.2], ray(0.66, 0.47, 1.6))
    # nothing to draw: wholly behind, off screen, collinear corners
    tri([0.1, 0.1, -1.0], [0.5, 0.2, -2.0], [-0.3, 0.6, -1.5])
    tri(ray(-2.0, 0.2, 2.0), ray(-1.5, 0.8, 2.0), ray(-1.2, 0.1, 2.2))
    tri([0.0, 0.0, 1.0], [0.1, 0.1, 1.1], [0.2, 0.2, 1.2])
    ef.append([5, 5, 9])  # repeated index
    verts = np.concatenate([field, np.asarray(extra, dtype=np.float64)], 0)
    faces = np.concatenate(faces + [np.asarray(ef, dtype=np.int64)], 0)
    cam1 = _rot_y(0.15)
    cam1[0, 3], cam1[1, 3], cam1[2, 3] = 0.2, -0.05, 0.1
    cams = torch.stack([torch.eye(4, dtype=torch.float64), torch.linalg.inv(cam1)]).float()
    return (torch.from_numpy(verts.astype(np.float32)), torch.from_numpy(faces), cams, Km.float().expand(2, 4, 4).contiguous())


def track_trajectory(T: int = 6):
    """cam_T_world (T,1,4,4) float32 of a camera that drifts and pans through a ``raster_scene``."""
    out = []
    for t in range(T):
        w = _rot_y(0.02 * t)
        w[0, 3], w[2, 3] = 0.03 * t, 0.01 * t
        out.append(torch.linalg.inv(w).float()[None])
    return torch.stack(out)


def track_predictions(T: int, height: int, width: int, seed: int = 0) -> torch.Tensor:
    """(T,1,1,height,width) float32 predictions in (0,1): a smooth function of pixel and frame whose 0.5 level set moves."""
    a = smooth_field((1, 1, height, width), seed, "track_a")
    b = smooth_field((1, 1, height, width), seed, "track_b")
    frames = [0.5 + 0.45 * np.tanh(1.5 * (np.cos(0.9 * t) * a + np.sin(0.9 * t) * b)) for t in range(T)]
    return torch.from_numpy(np.stack(frames).astype(np.float32))


def static_vertex_scene(height: int, width: int, step: int = 4):
    """A scene whose vertex sampling has no borderline case: a two-triangle tilted wall that fills the image of a camera at the world
    origin, and unreferenced vertices on the rays of every ``step``-th pixel centre, placed on the wall, 3 cm and 20 cm behind it and
    20 cm in front of it in turn.  Returns verts, faces, cam_T_world (1,4,4), K (1,4,4)."""
    Km = intrinsics(width, height)
    fx, fy, cx, cy = float(Km[0, 0]), float(Km[1, 1]), float(Km[0, 2]), float(Km[1, 2])
    wall = lambda dx, dy: 2.0 / (1.0 - 0.1 * dx + 0.05 * dy)  # z of the plane z = 2 + 0.1 x - 0.05 y along the ray (dx, dy, 1)
    corners = []
    for u, v in ((-7.3, -5.7), (width + 9.1, -6.4), (width + 8.2, height + 7.9), (-6.6, height + 5.3)):
        dx, dy = (u - cx) / fx, (v - cy) / fy
        zz = wall(dx, dy)
        corners.append([dx * zz, dy * zz, zz])
    pts, k = [], 0
    for i in range(step // 2, height, step):
        for j in range(step // 2, width, step):
            dx, dy = (j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy
            zz = wall(dx, dy) + (0.0, 0.03, 0.2, -0.2)[k % 4]
            pts.append([dx * zz, dy * zz, zz])
            k += 1
    verts = torch.tensor(corners + pts, dtype=torch.float64).float()
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int64)
    return verts, faces, torch.eye(4)[None], Km.float()[None]


KEYFRAME_TRAJECTORIES = ("orbit", "nan_gap", "jump", "stream12")


def keyframe_trajectory(kind: str, seed: int = 0):
    """A camera track for the keyframe buffer (keyframes.py): ``world_T_cam`` (T,4,4) float64 and the per-frame ``dist_to_last_valid``
    list ``try_new_keyframe`` takes (None entries: not given).  The camera orbits a point 1.5 m in front of it, with a seeded jitter of a
    few millimetres.  ``orbit``: 120 poses, 0.02 rad a frame (a keyframe about every third frame); ``nan_gap``: the same with poses
    50..89 NaN, ten more than the tracking-lost threshold; ``jump``: ``dist_to_last_valid`` is 1 except 45 at frame 60, where the camera
    also moves 3 m; ``stream12``: 12 poses at 0.08 rad a frame (every frame a keyframe) except frame 6, which repeats frame 5 within a
    millimetre, and frame 9, whose pose is NaN."""
    if kind not in KEYFRAME_TRAJECTORIES:
        raise ValueError(f"kind must be one of {KEYFRAME_TRAJECTORIES}, got {kind!r}")
    T, step = (12, 0.08) if kind == "stream12" else (120, 0.02)
    jitter = _rng(seed, "keyframe_" + kind).standard_normal(size=(T, 3)) * 0.004
    poses = np.empty((T, 4, 4), dtype=np.float64)
    back = np.eye(4)
    back[2, 3] = -1.5
    for t in range(T):
        if kind == "stream12" and t == 6:
            w = poses[5].copy()
            w[:3, 3] += jitter[t] * 0.25
        else:
            w = _rot_y(step * t).numpy() @ back
            w[:3, 3] += jitter[t]
        if kind == "jump" and t >= 60:
            w[0, 3] += 3.0
        poses[t] = w
    dists = [None] * T
    if kind == "nan_gap":
        poses[50:90] = np.nan
    elif kind == "jump":
        dists = [45 if t == 60 else 1 for t in range(T)]
    elif kind == "stream12":
        poses[9] = np.nan
    return poses, dists
