"""Keyframe selection of a live sequence on the host: the reference's DVMVS keyframe buffer (tools/keyframe_buffer.py, used by
data_scripts/generate_test_tuples.py:161-212) restated in numpy, handing out slot numbers of a fixed-size ring instead of images.

``pose_distance`` / ``is_pose_available``  keyframe_buffer.py:38-45, :69-85
``KeyframeBuffer.try_new_keyframe``        :115-179, return codes 0-5 kept (``CODE_*`` below)
``KeyframeBuffer.get_best_measurement_frames``  :181-205, the same ``np.argpartition`` call: the ORDER of the returned views is the
                                           reference's (the MLP feature volume is not permutation-invariant)
``DVMVS_Config`` / ``DVMVS_Hypersim_Config``  :12-35

Poses arrive as host arrays (4x4 ``world_T_cam``), as in ``FrameIngest``.  Where the reference stores ``(pose, image, index)`` the buffer
here stores ``(pose, slot, index)`` with ``slot = insertion count % buffer_size``: the ``deque(maxlen=buffer_size)`` holds the last
``buffer_size`` insertions at most, so the slots of its entries are distinct and the entry it evicts is the one whose slot the new entry takes.
The device side of a slot is ``feature_bank.FeatureBank``.  Needs no GPU."""
from __future__ import annotations

from collections import deque
from typing import List, Optional, Tuple

import numpy as np

# return codes of try_new_keyframe (keyframe_buffer.py:133-179)
CODE_FIRST_FRAME = 0      # pose available, buffer was empty: stored, no prediction
CODE_KEYFRAME = 1         # pose available and far enough from the last keyframe: stored, predict
CODE_NOT_ENOUGH_MOTION = 2
CODE_TRACKING_LOST = 3    # buffer cleared (over 30 frames without a pose), or reset by dist_to_last_valid > 30 (the frame is then stored)
CODE_STILL_LOST = 4
CODE_POSE_MISSING = 5     # no pose, not yet counted as lost


class DVMVS_Config:
    # train tuple settings
    train_minimum_pose_distance = 0.125
    train_maximum_pose_distance = 0.325
    train_crawl_step = 3

    # test tuple settings
    test_keyframe_buffer_size = 30
    test_keyframe_pose_distance = 0.1
    test_optimal_t_measure = 0.15
    test_optimal_R_measure = 0.0


class DVMVS_Hypersim_Config:
    # train tuple settings
    train_minimum_pose_distance = 0.125
    train_maximum_pose_distance = 2.5
    train_crawl_step = 3

    # test tuple settings
    test_keyframe_buffer_size = 30
    test_keyframe_pose_distance = 0.1
    test_optimal_t_measure = 0.15
    test_optimal_R_measure = 0.0


def is_pose_available(pose) -> bool:
    is_nan = np.isnan(pose).any()
    is_inf = np.isinf(pose).any()
    is_neg_inf = np.isneginf(pose).any()
    if is_nan or is_inf or is_neg_inf:
        return False
    else:
        return True


def pose_distance(reference_pose, measurement_pose):
    """(combined_measure, R_measure, t_measure) of two camera-to-world poses (keyframe_buffer.py:69-85)."""
    return _pose_distance(np.linalg.inv(reference_pose), measurement_pose)


def _pose_distance(inv_reference_pose, measurement_pose):
    """``pose_distance`` after its ``np.linalg.inv(reference_pose)``: the selection compares one reference with every stored keyframe, and
    the inverse of the same matrix is the same matrix each time."""
    rel_pose = np.dot(inv_reference_pose, measurement_pose)
    R = rel_pose[:3, :3]
    t = rel_pose[:3, 3]
    R_measure = np.sqrt(2 * (1 - min(3.0, np.trace(R)) / 3))
    t_measure = np.linalg.norm(t)
    combined_measure = np.sqrt(t_measure**2 + R_measure**2)
    return combined_measure, R_measure, t_measure


class KeyframeBuffer:
    """keyframe_buffer.py:88-205.  ``try_new_keyframe(pose, dist_to_last_valid, index)`` returns the reference's code; when it stored the
    pose, ``stored_slot`` is the ring slot the caller fills (None otherwise).  ``get_best_measurement_frames(n)`` returns
    ``(pose, slot, index)`` of the chosen keyframes in the reference's order."""

    def __init__(self, buffer_size: int = DVMVS_Config.test_keyframe_buffer_size,
                 keyframe_pose_distance: float = DVMVS_Config.test_keyframe_pose_distance,
                 optimal_t_score: float = DVMVS_Config.test_optimal_t_measure, optimal_R_score: float = DVMVS_Config.test_optimal_R_measure):
        if int(buffer_size) < 1:
            raise ValueError(f"buffer_size must be positive, got {buffer_size}")
        self.buffer_size = int(buffer_size)
        self.buffer = deque([], maxlen=self.buffer_size)
        self.keyframe_pose_distance = keyframe_pose_distance
        self.optimal_t_score = optimal_t_score
        self.optimal_R_score = optimal_R_score
        self.__tracking_lost_counter = 0
        self.__insertions = 0
        self.stored_slot: Optional[int] = None

    @classmethod
    def from_config(cls, config=DVMVS_Config, buffer_size: Optional[int] = None) -> "KeyframeBuffer":
        return cls(config.test_keyframe_buffer_size if buffer_size is None else buffer_size, config.test_keyframe_pose_distance,
                   config.test_optimal_t_measure, config.test_optimal_R_measure)

    def __len__(self) -> int:
        return len(self.buffer)

    def __append(self, pose, index) -> None:
        self.stored_slot = self.__insertions % self.buffer_size
        self.__insertions += 1
        self.buffer.append((pose, self.stored_slot, index))

    def calculate_penalty(self, t_score, R_score):
        degree = 2.0
        R_penalty = np.abs(R_score - self.optimal_R_score) ** degree
        t_diff = t_score - self.optimal_t_score
        if t_diff < 0.0:
            t_penalty = 5.0 * (np.abs(t_diff) ** degree)
        else:
            t_penalty = np.abs(t_diff) ** degree
        return R_penalty + t_penalty

    def try_new_keyframe(self, pose, dist_to_last_valid=None, index=None) -> int:
        self.stored_slot = None
        # In case valid frames are used, this helps guess if a gap in tracking happened when the indices are not indicative of time.
        if dist_to_last_valid is not None and dist_to_last_valid > 30:
            self.buffer.clear()
            self.__tracking_lost_counter = 0
            self.__append(pose, index)
            return CODE_TRACKING_LOST

        if is_pose_available(pose):
            self.__tracking_lost_counter = 0
            if len(self.buffer) == 0:
                self.__append(pose, index)
                return CODE_FIRST_FRAME
            else:
                last_pose, _, _ = self.buffer[-1]
                combined_measure, R_measure, t_measure = pose_distance(pose, last_pose)
                if combined_measure >= self.keyframe_pose_distance:
                    self.__append(pose, index)
                    return CODE_KEYFRAME
                else:
                    return CODE_NOT_ENOUGH_MOTION
        else:
            self.__tracking_lost_counter += 1
            if self.__tracking_lost_counter > 30:
                if len(self.buffer) > 0:
                    self.buffer.clear()
                    return CODE_TRACKING_LOST
                else:
                    return CODE_STILL_LOST
            else:
                return CODE_POSE_MISSING

    def get_best_measurement_frames(self, n_requested_measurement_frames: int) -> List[Tuple[np.ndarray, int, Optional[int]]]:
        buffer_array = list(self.buffer)
        reference_pose, _, _ = buffer_array[-1]

        n_requested_measurement_frames = min(n_requested_measurement_frames, len(buffer_array) - 1)

        inv_reference_pose = np.linalg.inv(reference_pose)  # pose_distance's first step, once for all entries
        penalties = []
        for i in range(len(buffer_array) - 1):
            measurement_pose = buffer_array[i][0]

            _, R_measure, t_measure = _pose_distance(inv_reference_pose, measurement_pose)
            penalty = self.calculate_penalty(t_measure, R_measure)
            penalties.append(penalty)
        indices = np.argpartition(penalties, n_requested_measurement_frames - 1)[:n_requested_measurement_frames]

        measurement_frames = []
        for index in indices:
            measurement_frames.append(buffer_array[index])
        return measurement_frames
