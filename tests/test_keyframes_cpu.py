"""keyframes.py against the reference's own KeyframeBuffer (tests/golden/keyframes.npz, written by tests/golden/gen_golden_keyframes.py):
every return code and every ORDERED list of selected frames, over four seeded tracks, buffer sizes 4 and 30 (eviction) and 2 / 3 / 7
requested measurement frames; and the ring slots the buffer hands out map back to those frames."""
import numpy as np
import pytest

import implicit_depth_amd.synthetic as syn
from conftest import load_golden
from implicit_depth_amd import keyframes as kf

CASES = [(kind, size, n) for kind in syn.KEYFRAME_TRAJECTORIES for size in (4, 30) for n in (2, 3, 7)]


@pytest.fixture(scope="module")
def golden():
    return load_golden("keyframes")


def _replay(kind, size, n):
    """(codes, selected frame indices, selected slots, slot -> frame map at each selection) of one run."""
    poses, dists = syn.keyframe_trajectory(kind, seed=0)
    buf = kf.KeyframeBuffer.from_config(kf.DVMVS_Config, buffer_size=size)
    codes = np.empty(len(poses), np.int8)
    sel = np.full((len(poses), n), -1, np.int32)
    in_slot = {}  # what a device-side bank of `size` slots would hold
    for i in range(len(poses)):
        codes[i] = buf.try_new_keyframe(poses[i].copy(), dists[i], index=i)
        if codes[i] == kf.CODE_TRACKING_LOST:
            in_slot.clear()
        assert (buf.stored_slot is not None) == (codes[i] in (0, 1) or (codes[i] == 3 and len(buf) == 1))
        if buf.stored_slot is not None:
            assert 0 <= buf.stored_slot < size
            in_slot[buf.stored_slot] = i
        if codes[i] == kf.CODE_KEYFRAME:
            frames = buf.get_best_measurement_frames(n)
            sel[i, :len(frames)] = [index for _, _, index in frames]
            # the slots name the same frames: a bank filled at `stored_slot` still holds each selected keyframe
            assert [in_slot[slot] for _, slot, _ in frames] == [index for _, _, index in frames]
            assert len({slot for _, slot, _ in buf.buffer}) == len(buf)
    return codes, sel


@pytest.mark.parametrize("kind,size,n", CASES)
def test_codes_and_ordered_selection_equal_the_reference(golden, kind, size, n):
    codes, sel = _replay(kind, size, n)
    np.testing.assert_array_equal(codes, golden[f"{kind}_b{size}_n{n}_codes"])
    np.testing.assert_array_equal(sel, golden[f"{kind}_b{size}_n{n}_sel"])


def test_fixture_covers_what_it_is_meant_to(golden):
    """Eviction, the tracking-lost threshold, the dist_to_last_valid reset and an order that is not sorted all occur in the recording."""
    assert set(np.unique(golden["nan_gap_b30_n7_codes"])) == {0, 1, 2, 3, 4, 5}
    assert golden["jump_b30_n7_codes"][60] == 3
    assert (golden["orbit_b4_n3_codes"] == 1).sum() > 30  # more keyframes than either buffer size
    sel = golden["orbit_b30_n7_sel"]
    full = sel[sel[:, -1] >= 0]
    assert len(full) > 10 and any(list(r) != sorted(r) for r in full) and any(list(r) != sorted(r, reverse=True) for r in full)
    # the 12-frame track of the streaming test: first frame, not enough motion at 6, no pose at 9
    assert golden["stream12_b4_n3_codes"].tolist() == [0, 1, 1, 1, 1, 1, 2, 1, 1, 5, 1, 1]


def test_pose_distance_and_configs():
    a = np.eye(4)
    b = np.eye(4)
    b[0, 3] = 0.3
    c, r, t = kf.pose_distance(a, b)
    assert (c, r, t) == (0.3, 0.0, 0.3)
    assert not kf.is_pose_available(np.full((4, 4), np.inf)) and not kf.is_pose_available(np.full((4, 4), np.nan)) and kf.is_pose_available(a)
    for cfg in (kf.DVMVS_Config, kf.DVMVS_Hypersim_Config):
        assert (cfg.test_keyframe_buffer_size, cfg.test_keyframe_pose_distance, cfg.test_optimal_t_measure, cfg.test_optimal_R_measure) == (30, 0.1, 0.15, 0.0)
    assert kf.DVMVS_Config.train_maximum_pose_distance == 0.325 and kf.DVMVS_Hypersim_Config.train_maximum_pose_distance == 2.5
