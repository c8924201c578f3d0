"""Seeded camera geometries for the plane-sweep volume tests (not a conftest: a plain helper module).  Everything is built on the CPU in
float64 and handed out as float32 CPU tensors; a test moves what it needs to the GPU.

Families (``FAMILIES``; ``build_case(family, seed, B, K, C, H, W)`` returns the whole input dictionary of a manager's forward):
  random      rotations up to ~1 rad about random axes, translations up to 2 m in any direction (views beside, behind and inside the
              swept volume), one random intrinsic matrix for every view and batch element (``random_geometry``).
  zcross      ``random`` with every other view replaced by a camera that looks across the swept volume, its z = 0 plane through the
              centre of the current frustum at the geometric-mean depth (``cross_source_plane``).
  roll_pitch  deterministic: rolls of 30 and 90 degrees about the optical axis and pitches of 20 degrees about x with translations of a
              few centimetres, so that column 1 of the homography (how u and z depend on the pixel row) is large.
  intrinsics  ``random`` rotations; every (b, k) has its own fx, fy (each scaled by a factor in [0.8, 1.25]) and cx, cy (shifted by up to
              10 % of the map size), every batch element its own current-frame K with cur_invK[b] its inverse.  No two matrices equal.

``MUTATIONS`` are the faults a kernel's matrix indexing could have; on inputs with one shared K and rotations about y alone (every
``synthetic.cost_volume_inputs`` case) none of them changes a single output value (tests/test_volume_geometry_cpu.py).
"""
import math

import numpy as np
import torch

FAMILIES = ("random", "zcross", "roll_pitch", "intrinsics")
MATRICES = ("src_extrinsics", "src_poses", "src_Ks", "cur_invK")


def rot(axis, ang):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)


def _f32(a):
    return torch.tensor(a, dtype=torch.float32).contiguous()


def random_geometry(rng, B, K, H, W):
    """One random intrinsic matrix (shared by all views) and B x K random source poses -> the four matrix inputs."""
    f = rng.uniform(0.6, 2.0) * W
    Kmat = np.eye(4)
    Kmat[0, 0] = f
    Kmat[1, 1] = f * rng.uniform(0.9, 1.1)
    Kmat[0, 2] = W * rng.uniform(0.4, 0.6)
    Kmat[1, 2] = H * rng.uniform(0.4, 0.6)
    poses = np.tile(np.eye(4), (B, K, 1, 1))
    for b in range(B):
        for k in range(K):
            mode = rng.integers(0, 4)
            ang = rng.uniform(0, 0.15) if mode == 0 else rng.uniform(0, 1.0)
            poses[b, k, :3, :3] = rot(rng.standard_normal(3), ang)
            scale = (0.2, 0.8, 2.0, 0.05)[mode]
            poses[b, k, :3, 3] = rng.standard_normal(3) * scale
    E = np.linalg.inv(poses)
    return {"src_extrinsics": _f32(E), "src_poses": _f32(poses), "src_Ks": _f32(np.tile(Kmat, (B, K, 1, 1))),
            "cur_invK": _f32(np.tile(np.linalg.inv(Kmat), (B, 1, 1)))}


def cross_source_plane(rng, inp, H, W, lo, hi):
    """z crosses 0 INSIDE a tile: every other view becomes a camera that looks across the swept volume (rotation of 70..110 degrees about
    the x or y axis), placed so that its z = 0 plane passes through the centre of the current frustum at the geometric-mean depth.
    Replaces ``src_extrinsics`` / ``src_poses`` of ``inp`` in place."""
    E = inp["src_extrinsics"].double().numpy()
    invK = inp["cur_invK"].double().numpy()
    B, K = E.shape[:2]
    for b in range(B):
        for k in range(0, K, 2):  # every other view is a crossing view, the rest stay random
            axis = np.array([0.0, 1.0, 0.0]) if rng.integers(0, 2) else np.array([1.0, 0.0, 0.0])
            R = rot(axis + 0.05 * rng.standard_normal(3), rng.uniform(1.22, 1.92) * (1 if rng.integers(0, 2) else -1))
            px = np.array([W * rng.uniform(0.3, 0.7), H * rng.uniform(0.3, 0.7), 1.0])
            X = math.sqrt(lo * hi) * (invK[b, :3, :3] @ px)
            t = -R @ X  # the point lands on the source camera's centre: z (and x, y) change sign around it
            t[:2] += rng.standard_normal(2) * 0.3
            E[b, k, :3, :3], E[b, k, :3, 3] = R, t
    inp["src_extrinsics"] = _f32(E)
    inp["src_poses"] = _f32(np.linalg.inv(E))
    return inp


def roll_pitch_geometry(B, K, H, W, variant=0):
    """No random numbers: view k of batch element b is, in turn, a roll of 30 degrees and one of 90 degrees about the optical axis and a
    pitch of 20 degrees about x (the sign alternates from one round of three to the next, ``variant`` and b shift the turn), a few
    centimetres away from the current camera.  Pin-hole intrinsics with fx = 0.9 W, fy = 1.2 H for every view."""
    Kmat = np.eye(4)
    Kmat[0, 0], Kmat[1, 1], Kmat[0, 2], Kmat[1, 2] = 0.9 * W, 1.2 * H, 0.5 * W - 0.25, 0.5 * H + 0.25
    z, x = np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])
    poses = np.tile(np.eye(4), (B, K, 1, 1))
    for b in range(B):
        for k in range(K):
            turn, sign = (k + b + variant) % 3, 1.0 if ((k + variant) // 3) % 2 == 0 else -1.0
            poses[b, k, :3, :3] = (rot(z, sign * math.radians(30)), rot(z, sign * math.radians(90)), rot(x, sign * math.radians(20)))[turn]
            poses[b, k, :3, 3] = [0.06 * (k % 4 - 1.5) + 0.013 * b, 0.05 * ((k + variant) % 3 - 1) - 0.007 * b, 0.02 * (k % 5) - 0.03]
    E = np.linalg.inv(poses)
    return {"src_extrinsics": _f32(E), "src_poses": _f32(poses), "src_Ks": _f32(np.tile(Kmat, (B, K, 1, 1))),
            "cur_invK": _f32(np.tile(np.linalg.inv(Kmat), (B, 1, 1)))}


def per_view_intrinsics(rng, inp, H, W):
    """Every (b, k) gets its own source K and every b its own current K, derived from the shared matrix of ``inp`` (fx, fy each scaled by a
    factor in [0.8, 1.25], cx, cy shifted by up to 10 % of the map size); cur_invK[b] is the inverse of the current K of b.  In place."""
    base = inp["src_Ks"][0, 0].double().numpy()
    B, K = inp["src_Ks"].shape[:2]

    def one():
        M = base.copy()
        M[0, 0] *= rng.uniform(0.8, 1.25)
        M[1, 1] *= rng.uniform(0.8, 1.25)
        M[0, 2] += rng.uniform(-0.1, 0.1) * W
        M[1, 2] += rng.uniform(-0.1, 0.1) * H
        return M

    src = np.stack([np.stack([one() for _ in range(K)]) for _ in range(B)])
    cur = np.stack([one() for _ in range(B)])
    inp["src_Ks"], inp["cur_invK"] = _f32(src), _f32(np.linalg.inv(cur))
    every = [tuple(m.tolist()) for m in torch.cat([inp["src_Ks"].reshape(-1, 16), _f32(cur).reshape(-1, 16)])]
    assert len(set(every)) == len(every), "two intrinsic matrices of the case are equal"
    assert len({tuple(m.tolist()) for m in inp["cur_invK"].reshape(-1, 16)}) == B, "two cur_invK of the case are equal"
    return inp


def build_case(family, seed, B, K, C, H, W):
    """The whole input of CostVolumeManager / FeatureVolumeManager.forward for one seeded case: features ~ N(0, 1), the four matrix
    inputs of the family and a depth range (plain floats)."""
    if family not in FAMILIES:
        raise ValueError(f"family must be one of {FAMILIES}, got {family!r}")
    rng = np.random.default_rng([FAMILIES.index(family), seed])
    lo = float(rng.uniform(0.2, 1.0))
    hi = lo * float(rng.uniform(3.0, 20.0))
    if family == "roll_pitch":
        inp = roll_pitch_geometry(B, K, H, W, variant=seed)
    else:
        inp = random_geometry(rng, B, K, H, W)
    if family == "zcross":
        cross_source_plane(rng, inp, H, W, lo, hi)
    if family == "intrinsics":
        per_view_intrinsics(rng, inp, H, W)
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    inp["cur_feats"] = torch.randn(B, C, H, W, generator=g)
    inp["src_feats"] = torch.randn(B, K, C, H, W, generator=g)
    inp["min_depth"], inp["max_depth"] = lo, hi
    return inp


# ---- the faults the geometry cases are there to catch, as functions on the input dictionary (each returns a changed copy) ----------
def _copy(inp):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in inp.items()}


def drop_row_terms(inp):
    """(a) E[0][1] = E[2][1] = 0: u and z no longer depend on the pixel row through the rotation."""
    out = _copy(inp)
    out["src_extrinsics"][..., 0, 1] = 0
    out["src_extrinsics"][..., 2, 1] = 0
    return out


def first_view_K_for_every_view(inp):
    """(b) src_K + (b * K) * 16 instead of src_K + (b * K + k) * 16"""
    out = _copy(inp)
    out["src_Ks"][:] = inp["src_Ks"][:, :1]
    return out


def first_batch_invK_for_every_batch(inp):
    """(c) cur_invK instead of cur_invK + b * 16"""
    out = _copy(inp)
    out["cur_invK"][:] = inp["cur_invK"][:1]
    return out


def first_batch_K_for_every_batch(inp):
    """(d) src_K + k * 16 instead of src_K + (b * K + k) * 16"""
    out = _copy(inp)
    out["src_Ks"][:] = inp["src_Ks"][:1]
    return out


MUTATIONS = {"a_row_terms_zero": drop_row_terms, "b_view0_K": first_view_K_for_every_view, "c_batch0_invK": first_batch_invK_for_every_batch,
             "d_batch0_K": first_batch_K_for_every_batch}


# ---- oracle calls on a case --------------------------------------------------------------------------------------------------------
def oracle_feature_volume(inp, D, mlp_weights, dtype=torch.float64):
    """oracle/cost_volume.py's feature volume of a case in ``dtype`` -> (volume, lowest, mask)"""
    from oracle import cost_volume as ocv

    d = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in inp.items()}
    w = {k: v.to(dtype) for k, v in mlp_weights.items()}
    vol, low, _, mask = ocv.feature_volume(d["cur_feats"], d["src_feats"], d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"],
                                           inp["min_depth"], inp["max_depth"], D, w, return_mask=True)
    return vol, low, mask


def oracle_dot_volume(inp, D, dtype=torch.float64):
    from oracle import cost_volume as ocv

    d = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in inp.items()}
    vol, low, _ = ocv.cost_volume_dot(d["cur_feats"], d["src_feats"], d["src_extrinsics"], d["src_Ks"], d["cur_invK"], inp["min_depth"],
                                      inp["max_depth"], D)
    return vol, low
