"""StreamingSession over a 12-frame synthetic sequence against ``fused_forward(native_matching_stem=True)`` fed the same current image
and the images of the selected keyframes, every matching feature recomputed from scratch.

Model: the smallest configuration tests/hot_helpers.py builds (24x32 matching maps of a 96x128 image, D = 16, synthetic weights) with the
native ResNet18 matching stem and the stand-in image encoder.  Keyframe buffer of 4, so K = 3 for the MLP feature volume (whose K is a
constructor argument) and the dot-product configuration's own K = 2.  Track: ``synthetic.keyframe_trajectory("stream12")``; which frames
predict, and from which keyframes, is the reference KeyframeBuffer's own recording (tests/golden/keyframes.npz)."""
import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn
from conftest import TOL, load_golden, rel_err
from hot_helpers import holder, to_cuda

pytestmark = pytest.mark.gpu

IMG_H, IMG_W, D, BUFFER = 96, 128, 16, 4
T = 12


class _RunOpts:
    matching_scale = 1
    min_matching_depth = 0.25
    max_matching_depth = 5.0

    def __init__(self, use_prior):
        self.use_prior = use_prior


def _model(volume, K, use_prior=False):
    from implicit_depth_amd import backbone
    from implicit_depth_amd import networks as net

    m = holder(K, volume, IMG_H // 4, IMG_W // 4, D, use_prior=use_prior, with_head=False)
    m.matching_model = net.ResnetMatchingEncoder(backbone.resnet18_stem(), 16)
    m.encoder = syn.StubImageEncoder()
    m.run_opts = _RunOpts(use_prior)
    m.thresholder = None
    syn.fill_state_dict(m, seed=30)  # name-keyed: the holder's modules keep the weights holder() gave them
    return m.cuda().eval()


def _frame(t, poses, P=3, own_K=False):
    """``FrameIngest``'s dictionary for frame t of the track, built by hand (float32, on the GPU).  ``own_K``: the frame's matching-scale
    intrinsics are its own (focal lengths 0.8 .. 1.25 of the shared ones, principal point up to 10 % of the map size away)."""
    Hm, Wm = IMG_H // 4, IMG_W // 4
    K1, K0 = syn.intrinsics(Wm, Hm).float(), syn.intrinsics(IMG_W // 2, IMG_H // 2).float()
    if own_K:
        K1[0, 0] *= 0.8 + 0.45 * ((5 * t + 2) % 12) / 11
        K1[1, 1] *= 0.8 + 0.45 * ((7 * t + 5) % 12) / 11
        K1[0, 2] += 0.1 * Wm * (((5 * t + 3) % 12) / 5.5 - 1)
        K1[1, 2] += 0.1 * Hm * (((7 * t + 1) % 12) / 5.5 - 1)
    w = poses[t].astype(np.float32)
    c = np.linalg.inv(w) if np.isfinite(w).all() else np.full((4, 4), np.nan, np.float32)
    return to_cuda({
        "image_b3hw": syn.randn((1, 3, IMG_H, IMG_W), 500 + t, "stream_img"),
        "K_s1_b44": K1[None].clone(), "invK_s1_b44": torch.linalg.inv(K1)[None], "K_s0_b44": K0[None].clone(), "invK_s0_b44": torch.linalg.inv(K0)[None],
        "world_T_cam_b44": torch.from_numpy(w)[None], "cam_T_world_b44": torch.from_numpy(c)[None],
        "rendered_depth": syn.rendered_depth_planes(1, IMG_H // 2, IMG_W // 2, P),
    })


def _src_of(frames, indices):
    """``src_data`` of the reference forward from the frames' own dictionaries: a view dimension after the batch."""
    keys = ("image_b3hw", "K_s1_b44", "invK_s1_b44", "world_T_cam_b44", "cam_T_world_b44")
    return {k: torch.stack([frames[i][k][0] for i in indices])[None] for k in keys}


def _compare(out, ref, where):
    assert set(out) == set(ref), (where, sorted(out), sorted(ref))
    for k, v in ref.items():
        if v is None:
            assert out[k] is None, (where, k)
        elif v.dtype == torch.bool or k == "overall_mask_bhw":
            print(f"{where} {k}: {int((out[k] != v).sum())} of {v.numel()} differ")
            assert torch.equal(out[k], v), (where, k)
        else:
            err = rel_err(out[k].cpu(), v.cpu())
            print(f"{where} {k}: scale-rel err {err:.2e}")
            assert err < TOL, (where, k, err)


@pytest.mark.parametrize("volume,K", [("mlp", 3), ("dot", 2)])
def test_session_equals_fused_forward_on_recomputed_keyframes(volume, K):
    from implicit_depth_amd.dropin import fused_forward, hot_path_of
    from implicit_depth_amd.streaming import StreamingSession

    g = load_golden("keyframes")
    codes, sel = g[f"stream12_b{BUFFER}_n{K}_codes"], g[f"stream12_b{BUFFER}_n{K}_sel"]
    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    m = _model(volume, K)
    session = StreamingSession(m, num_source_views=K, buffer_size=BUFFER)
    reference = fused_forward(m, native_matching_stem=True)
    hot = hot_path_of(m, native_matching_stem=True)
    frames = [_frame(t, poses) for t in range(T)]
    predicted, same_bits = [], []
    for t in range(T):
        out, code = session.step(frames[t], world_T_cam=poses[t], dist_to_last_valid=dists[t], return_mask=True)
        assert code == codes[t], (t, code, codes[t])
        due = codes[t] == 1 and sel[t, -1] >= 0  # a new keyframe with K earlier ones stored
        assert (out is not None) == due, (t, code)
        if out is None:
            continue
        predicted.append(t)
        assert list(session.last_indices) == sel[t].tolist(), (t, session.last_indices, sel[t])  # the reference's views in its order
        src = _src_of(frames, session.last_indices)
        ref = reference("test", dict(frames[t]), src, return_mask=True)
        torch.cuda.synchronize()
        _compare(out, ref, f"{volume} frame {t}")
        # recorded, not asserted: were the cached features the bits a from-scratch batch of K + 1 images gives?
        E = src["cam_T_world_b44"] @ frames[t]["world_T_cam_b44"].unsqueeze(1)
        Pm = frames[t]["cam_T_world_b44"].unsqueeze(1) @ src["world_T_cam_b44"]
        with torch.no_grad():
            o = hot(None, None, list(m.encoder(frames[t]["image_b3hw"])), E, Pm, src["K_s1_b44"], frames[t]["invK_s1_b44"],
                    rendered_depth=frames[t]["rendered_depth"], matching_images=torch.cat([frames[t]["image_b3hw"][:, None], src["image_b3hw"]], 1),
                    return_matching_feats=True)
        cur_n, src_n = session.last_matching
        same = torch.equal(cur_n.permute(0, 3, 1, 2), o["matching_cur_feats"]) and torch.equal(src_n.permute(0, 1, 4, 2, 3), o["matching_src_feats"])
        same_bits.append(same)
        print(f"{volume} frame {t}: cached matching features bit-identical to the recomputed batch: {same}; "
              f"scale-rel difference {rel_err(src_n.permute(0, 1, 4, 2, 3).cpu(), o['matching_src_feats'].cpu()):.2e}")
    expected = [t for t in range(T) if codes[t] == 1 and sel[t, -1] >= 0]
    assert predicted == expected and len(predicted) >= 6
    print(f"{volume}: predicted on frames {predicted}; cached == recomputed bits on {sum(same_bits)} of {len(same_bits)}")


@pytest.mark.parametrize("volume,K", [("mlp", 3), ("dot", 2)])
def test_session_follows_per_frame_intrinsics(volume, K):
    """Every frame of the track has its own K_s1_b44 / invK_s1_b44 (a stream that mixes cameras, or a zoom): the keyframe bank must hand each
    stored view its own K and the current frame its own inverse.  The first seven frames of the track, compared as above with the forward fed
    the selected keyframes by hand; the same keyframes with frame 0's K for every view must give another volume."""
    from implicit_depth_amd.dropin import fused_forward
    from implicit_depth_amd.streaming import StreamingSession

    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    m = _model(volume, K)
    session = StreamingSession(m, num_source_views=K, buffer_size=BUFFER)
    reference = fused_forward(m, native_matching_stem=True)
    frames = [_frame(t, poses, own_K=True) for t in range(7)]
    every = [tuple(f[k].flatten().tolist()) for f in frames for k in ("K_s1_b44", "invK_s1_b44")]
    assert len(set(every)) == len(every)
    n = 0
    for t in range(7):
        out, code = session.step(frames[t], world_T_cam=poses[t], dist_to_last_valid=dists[t], return_mask=True)
        if out is None:
            continue
        src = _src_of(frames, session.last_indices)
        ref = reference("test", dict(frames[t]), src, return_mask=True)
        torch.cuda.synchronize()
        _compare(out, ref, f"{volume} own K, frame {t}")
        shared = dict(src, K_s1_b44=frames[0]["K_s1_b44"][None].expand_as(src["K_s1_b44"]).contiguous())
        blind = reference("test", dict(frames[t]), shared, return_mask=True)
        moved = rel_err(blind["pred_0"].cpu(), ref["pred_0"].cpu())
        print(f"{volume} own K, frame {t}: one K for every view moves pred_0 by {moved:.2e} of its scale")
        assert moved > 100 * TOL, (t, moved)
        n += 1
    assert n >= 2, n


def test_prior_is_handed_over_between_predictions():
    """A BDModel with use_prior: three consecutive predictions (frames 3, 4, 5 of the track), each given the previous one's
    sigmoid(pred_0) and cam_T_world (inference/inference.py:139-157); the reference side carries them by hand."""
    from implicit_depth_amd.dropin import fused_forward
    from implicit_depth_amd.streaming import StreamingSession

    K = 3
    poses, dists = syn.keyframe_trajectory("stream12", seed=0)
    m = _model("mlp", K, use_prior=True)
    session = StreamingSession(m, buffer_size=BUFFER)
    assert session.use_prior and session.K == K
    reference = fused_forward(m, native_matching_stem=True)
    frames = [_frame(t, poses, P=1) for t in range(6)]
    prev = None
    n = 0
    for t in range(6):
        out, code = session.step(frames[t], world_T_cam=poses[t], dist_to_last_valid=dists[t], return_mask=True)
        if t < 3:
            assert out is None
            continue
        cur = dict(frames[t])
        cur.pop("prior_mask", None)
        if prev is not None:
            cur["prior_prediction"], cur["prior_cam_T_world"] = prev
        ref = reference("test", cur, _src_of(frames, session.last_indices), return_mask=True)
        torch.cuda.synchronize()
        _compare(out, ref, f"prior frame {t}")
        assert ("prior_mask" in frames[t]) == (prev is not None) == ("prior_mask" in cur)
        if prev is not None:
            assert rel_err(frames[t]["prior_mask"].cpu(), cur["prior_mask"].cpu()) < TOL
            assert float(frames[t]["prior_mask"].max()) > 0  # the warped prior reaches the image: the hand-over is exercised
        prev = (torch.sigmoid(ref["pred_0"]), frames[t]["cam_T_world_b44"])
        n += 1
    assert n == 3


def test_session_arguments():
    from implicit_depth_amd import _lib
    from implicit_depth_amd.streaming import StreamingSession

    m = _model("mlp", 3)
    with pytest.raises(_lib.IdhError, match="dense"):
        StreamingSession(m, buffer_size=BUFFER, mode="dense")
    with pytest.raises(_lib.IdhError, match="buffer_size"):
        StreamingSession(m, buffer_size=3)  # K + 1 keyframes are needed
    with pytest.raises(_lib.IdhError, match="buffer_size"):
        StreamingSession(m, buffer_size=65)
    with pytest.raises(_lib.IdhError, match="num_source_views"):
        StreamingSession(_model("dot", 2), buffer_size=BUFFER)
