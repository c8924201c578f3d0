"""Keyframe feature bank on the GPU (csrc/feature_bank.hip, include/idh_bank.h): the device side of ``keyframes.KeyframeBuffer``.

A ring of ``N`` slots, each one frame's channels-last matching features (H,W,C) with its ``world_T_cam``, ``cam_T_world`` and ``K_s1``.
``commit`` stores a frame in the slot the buffer handed out; ``gather`` writes, for K slots per batch entry and in ONE launch, what the
volume kernels read: the (B,K,H,W,C) source features, ``src_K`` and the relative poses of bd_model.py:200-204, into buffers the bank
owns and reuses (a step allocates nothing).  Arithmetic contract: DESIGN.md §4.11.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence, Tuple

import torch

from . import _lib


class FeatureBank:
    def __init__(self, num_slots: int, height: int, width: int, channels: int = 16, device="cuda"):
        if not 1 <= int(num_slots) <= _lib.BANK_MAX_SLOTS:
            raise _lib.IdhError(f"num_slots must be in [1, {_lib.BANK_MAX_SLOTS}], got {num_slots}")
        if channels not in (16, 32):
            raise _lib.IdhError(f"matching features have 16 or 32 channels, got {channels}")
        if height < 1 or width < 1:
            raise _lib.IdhError(f"feature size must be positive, got {height}x{width}")
        self.N, self.H, self.W, self.C = int(num_slots), int(height), int(width), int(channels)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.IdhError("the feature bank lives on the MI355X (there is no CPU fallback)")
        self.feats = torch.zeros(self.N, self.H, self.W, self.C, device=self.device)
        self.mats = torch.zeros(self.N, 3, 4, 4, device=self.device)
        self._desc = _lib.Bank()
        self._desc.feats, self._desc.mats = self.feats.data_ptr(), self.mats.data_ptr()
        self._desc.N, self._desc.H, self._desc.W, self._desc.C = self.N, self.H, self.W, self.C
        self._out: Dict[Tuple[int, int], Dict[str, torch.Tensor]] = {}

    def commit(self, slot: int, feat_nhwc: torch.Tensor, world_T_cam: torch.Tensor, cam_T_world: torch.Tensor, K_s1: torch.Tensor) -> None:
        """``feat_nhwc`` (H,W,C) or (1,H,W,C); the matrices (4,4) or (1,4,4); all fp32 on the bank's device."""
        _lib.require_cuda_f32(feat_nhwc, world_T_cam, cam_T_world, K_s1)
        if feat_nhwc.numel() != self.H * self.W * self.C or tuple(feat_nhwc.shape[-3:]) != (self.H, self.W, self.C):
            raise _lib.IdhError(f"features {tuple(feat_nhwc.shape)} must be ({self.H},{self.W},{self.C}) channels-last")
        mats = []
        for name, m in (("world_T_cam", world_T_cam), ("cam_T_world", cam_T_world), ("K_s1", K_s1)):
            if m.numel() != 16 or tuple(m.shape[-2:]) != (4, 4):
                raise _lib.IdhError(f"{name} {tuple(m.shape)} must be (4,4)")
            mats.append(m if m.is_contiguous() else m.contiguous())
        f = feat_nhwc if feat_nhwc.is_contiguous() else feat_nhwc.contiguous()
        _lib.check(_lib.lib().idh_bank_commit_fwd(C.byref(self._desc), int(slot), f.data_ptr(), mats[0].data_ptr(), mats[1].data_ptr(),
                                                  mats[2].data_ptr(), _lib.stream_ptr()), "idh_bank_commit_fwd")

    def outputs(self, B: int, K: int) -> Dict[str, torch.Tensor]:
        """The persistent output buffers of a (B, K) gather: ``src_nhwc`` (B,K,H,W,C), ``src_K``, ``src_E``, ``src_poses`` (B,K,4,4)."""
        o = self._out.get((B, K))
        if o is None:
            o = {"src_nhwc": torch.empty(B, K, self.H, self.W, self.C, device=self.device)}
            for k in ("src_K", "src_E", "src_poses"):
                o[k] = torch.empty(B, K, 4, 4, device=self.device)
            self._out[(B, K)] = o
        return o

    def gather(self, slots: Sequence[Sequence[int]], cur_world_T_cam: torch.Tensor, cur_cam_T_world: torch.Tensor) -> Dict[str, torch.Tensor]:
        """``slots``: B lists of K slot numbers (host integers, order kept, repeats allowed); the current frames' poses (B,4,4) on the
        device.  Returns ``outputs(B, K)``, overwritten by the next gather of the same shape."""
        _lib.require_cuda_f32(cur_world_T_cam, cur_cam_T_world)
        B = len(slots)
        K = len(slots[0]) if B else 0
        if any(len(s) != K for s in slots):
            raise _lib.IdhError("every batch entry needs the same number of slots")
        for name, m in (("cur_world_T_cam", cur_world_T_cam), ("cur_cam_T_world", cur_cam_T_world)):
            if tuple(m.shape) != (B, 4, 4):
                raise _lib.IdhError(f"{name} {tuple(m.shape)} must be ({B},4,4)")
        wTc = cur_world_T_cam if cur_world_T_cam.is_contiguous() else cur_world_T_cam.contiguous()
        cTw = cur_cam_T_world if cur_cam_T_world.is_contiguous() else cur_cam_T_world.contiguous()
        flat = (C.c_int32 * max(B * K, 1))(*[int(s) for row in slots for s in row])
        o = self.outputs(B, K)
        _lib.check(_lib.lib().idh_bank_gather_fwd(C.byref(self._desc), flat, wTc.data_ptr(), cTw.data_ptr(), o["src_nhwc"].data_ptr(),
                                                  o["src_K"].data_ptr(), o["src_E"].data_ptr(), o["src_poses"].data_ptr(), B, K,
                                                  _lib.stream_ptr()), "idh_bank_gather_fwd")
        return o
