"""The keyframe feature bank (csrc/feature_bank.hip, include/idh_bank.h): commit and the one-launch gather against torch.index_select and
float64 matrix products.  Features are copied bit for bit; a 4x4 product element is an fp32 sum of four fp32 products, so it lies within
4 * 2^-24 * sum_k |a_ik| |b_kj| of the exact value (the standard bound of a 4-term dot product, no tuned tolerance).

Shapes: 5x7 and 12x16 maps with 16 and 32 channels give 140 .. 1536 float4 per view against the workgroup's tile of 1024: views that are
one cut tile, and (12x16x32) one whole tile followed by a cut one; 24x32x16 is three whole tiles.  The ring has N = 3 slots and receives
five frames, so slots 0 and 1 are overwritten (frames 3, 4, 2 remain) and every K > 3 repeats slots."""
import ctypes

import numpy as np
import pytest
import torch

import implicit_depth_amd.synthetic as syn

pytestmark = pytest.mark.gpu

N_SLOTS, N_FRAMES = 3, 5
U = 2.0 ** -24


def _rigid(rng):
    """A random rigid world_T_cam (float64): rotation from a QR factorisation, translation of a few metres."""
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = q, rng.uniform(-3, 3, 3)
    return m


def _frames(H, W, C, seed):
    """N_FRAMES frames: features (H,W,C), world_T_cam, cam_T_world, K_s1, all float32 on the GPU."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(N_FRAMES):
        w = _rigid(rng)
        K = syn.intrinsics(W, H).numpy().copy()
        K[0, 0] += i  # per-frame intrinsics: a K copied from the wrong slot shows
        f = torch.from_numpy(rng.standard_normal((H, W, C), dtype=np.float32))
        out.append([t.cuda() for t in (f, torch.from_numpy(w).float(), torch.from_numpy(np.linalg.inv(w)).float(), torch.from_numpy(K).float())])
    return out


def _filled_bank(H, W, C, seed):
    """A bank of N_SLOTS after N_FRAMES commits (slot = i % N_SLOTS), and what each slot must hold."""
    from implicit_depth_amd.feature_bank import FeatureBank

    frames = _frames(H, W, C, seed)
    bank = FeatureBank(N_SLOTS, H, W, C)
    held = [None] * N_SLOTS
    for i, fr in enumerate(frames):
        bank.commit(i % N_SLOTS, *fr)
        held[i % N_SLOTS] = fr
    return bank, held


def _slot_lists(B, K, seed):
    """B lists of K slots: the first starts on both sides of the ring's wrap point (slot 2 holds frame 2, slot 0 frame 3) and repeats a slot."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    lists = rng.integers(0, N_SLOTS, (B, K)).tolist()
    lists[0][:3] = [2, 0, 2][:K]
    return lists


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("K", [1, 7, 8])
@pytest.mark.parametrize("C", [16, 32])
@pytest.mark.parametrize("H,W", [(5, 7), (12, 16)])
def test_gather_matches_index_select_and_float64_products(H, W, C, K, B):
    bank, held = _filled_bank(H, W, C, seed=H * C + K)
    torch.cuda.synchronize()
    # commit: every slot holds its last frame bit for bit, the matrices too
    assert torch.equal(bank.feats, torch.stack([h[0] for h in held]))
    assert torch.equal(bank.mats, torch.stack([torch.stack(h[1:]) for h in held]))

    rng = np.random.Generator(np.random.PCG64(7))
    cur_w = np.stack([_rigid(rng) for _ in range(B)])
    cur_wTc, cur_cTw = torch.from_numpy(cur_w).float().cuda(), torch.from_numpy(np.linalg.inv(cur_w)).float().cuda()
    slots = _slot_lists(B, K, seed=K + B)
    out = bank.gather(slots, cur_wTc, cur_cTw)
    torch.cuda.synchronize()

    idx = torch.tensor(slots, device="cuda").flatten()
    assert torch.equal(out["src_nhwc"], torch.index_select(bank.feats, 0, idx).view(B, K, H, W, C))
    assert torch.equal(out["src_K"], torch.index_select(bank.mats[:, 2], 0, idx).view(B, K, 4, 4))
    src_wTc = torch.index_select(bank.mats[:, 0], 0, idx).view(B, K, 4, 4).double()
    src_cTw = torch.index_select(bank.mats[:, 1], 0, idx).view(B, K, 4, 4).double()
    cw, cc = cur_wTc.double().unsqueeze(1), cur_cTw.double().unsqueeze(1)
    for name, got, a, b in (("src_E", out["src_E"], src_cTw, cw), ("src_poses", out["src_poses"], cc, src_wTc)):
        err = (got.double() - a @ b).abs()
        bound = 4 * U * (a.abs() @ b.abs())
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{name} {H}x{W}x{C} K={K} B={B}: max |err| / bound = {worst:.3f}")
        assert bool((err <= bound).all()), (name, worst)
    # the persistent buffers are reused: a second gather of the same shape allocates nothing new
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    out2 = bank.gather(slots, cur_wTc, cur_cTw)
    assert {k: v.data_ptr() for k, v in out2.items()} == ptrs


def test_three_whole_tiles_and_neighbouring_slots_untouched():
    """24x32x16 (3072 float4: whole tiles only), and a commit changes its own slot alone."""
    H, W, C = 24, 32, 16
    bank, held = _filled_bank(H, W, C, seed=3)
    before_f, before_m = bank.feats.clone(), bank.mats.clone()
    fr = _frames(H, W, C, seed=99)[0]
    bank.commit(1, *fr)
    torch.cuda.synchronize()
    before_f[1], before_m[1] = fr[0], torch.stack(fr[1:])
    assert torch.equal(bank.feats, before_f) and torch.equal(bank.mats, before_m)
    eye = torch.eye(4, device="cuda")[None]
    out = bank.gather([[1, 1, 0, 2]], eye, eye)
    torch.cuda.synchronize()
    assert torch.equal(out["src_nhwc"][0], bank.feats[[1, 1, 0, 2]])
    assert torch.equal(out["src_E"][0], bank.mats[[1, 1, 0, 2], 1]) and torch.equal(out["src_poses"][0], bank.mats[[1, 1, 0, 2], 0])


def test_invalid_arguments_are_refused_without_a_launch():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    H, W, C, B, K = 5, 7, 16, 1, 2
    bank, _ = _filled_bank(H, W, C, seed=5)
    eye = torch.eye(4, device="cuda")[None].contiguous()
    outs = [torch.full((B, K, H, W, C), 7.0, device="cuda")] + [torch.full((B, K, 4, 4), 7.0, device="cuda") for _ in range(3)]
    feats0, mats0 = bank.feats.clone(), bank.mats.clone()
    sp = _lib.stream_ptr()

    def desc(**over):
        d = _lib.Bank()
        d.feats, d.mats, d.N, d.H, d.W, d.C = bank.feats.data_ptr(), bank.mats.data_ptr(), N_SLOTS, H, W, C
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def gather(d, slots, ptrs=None, cur=(eye.data_ptr(), eye.data_ptr()), slots_null=False):
        p = [o.data_ptr() for o in outs] if ptrs is None else ptrs
        arr = None if slots_null else (ctypes.c_int32 * len(slots))(*slots)
        return L.idh_bank_gather_fwd(ctypes.byref(d) if d is not None else None, arr, cur[0], cur[1], *p, B, K, sp)

    def commit(d, slot, ptrs=None):
        p = [bank.feats[0].data_ptr(), eye.data_ptr(), eye.data_ptr(), eye.data_ptr()] if ptrs is None else ptrs
        return L.idh_bank_commit_fwd(ctypes.byref(d) if d is not None else None, slot, *p, sp)

    EINVAL = -1
    assert L.idh_error_string(EINVAL).decode().lower().find("invalid") >= 0
    good = [o.data_ptr() for o in outs]
    assert gather(desc(), [0, N_SLOTS]) == EINVAL and gather(desc(), [-1, 0]) == EINVAL  # a slot outside [0, N)
    for c in (0, 8, 24, 64):
        assert gather(desc(C=c), [0, 1]) == EINVAL and commit(desc(C=c), 0) == EINVAL
    assert gather(desc(N=0), [0, 0]) == EINVAL and gather(desc(N=65), [0, 0]) == EINVAL
    assert gather(None, [0, 1]) == EINVAL and gather(desc(feats=None), [0, 1]) == EINVAL and gather(desc(mats=None), [0, 1]) == EINVAL
    assert gather(desc(), [0, 1], slots_null=True) == EINVAL
    assert gather(desc(), [0, 1], cur=(None, eye.data_ptr())) == EINVAL and gather(desc(), [0, 1], cur=(eye.data_ptr(), None)) == EINVAL
    for i in range(4):
        assert gather(desc(), [0, 1], ptrs=[None if j == i else g for j, g in enumerate(good)]) == EINVAL
    assert gather(desc(), [0, 1], ptrs=[good[0] + 4] + good[1:]) == EINVAL  # features not 16-byte aligned
    short = desc()
    short.struct_size = ctypes.sizeof(_lib.Bank) - 8
    assert gather(short, [0, 1]) == EINVAL
    assert commit(desc(), -1) == EINVAL and commit(desc(), N_SLOTS) == EINVAL and commit(None, 0) == EINVAL
    cp = [bank.feats[0].data_ptr(), eye.data_ptr(), eye.data_ptr(), eye.data_ptr()]
    for i in range(4):
        assert commit(desc(), 0, ptrs=[None if j == i else g for j, g in enumerate(cp)]) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)  # nothing was launched
    assert torch.equal(bank.feats, feats0) and torch.equal(bank.mats, mats0)
    assert gather(desc(), [2, 2]) == 0  # and the same call with valid arguments runs
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0, 0], bank.feats[2])
    with pytest.raises(_lib.IdhError):
        bank.gather([[0, 3]], eye, eye)
