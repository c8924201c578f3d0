"""The fp64 reference of the TSDF fusion (tests/tsdf_ref.py) on its own: the committed scenes stay under the ambiguity cap by the
reference alone, they hold what they are there for, and the block flags the header defines are a superset that makes empty-space
skipping exact - checked in numpy on the reference's volume, whose skip-free march is the definition."""
import numpy as np
import pytest

import tsdf_ref as R


@pytest.mark.parametrize("name", sorted(R.SCENES))
@pytest.mark.parametrize("M", [1, None])
def test_integrate_scenes_stay_under_the_cap_and_hold_their_cases(name, M):
    r = R.scene_integrated(name, M)
    touched = int(r["touched"].sum())
    amb = int((r["touched"] & r["ambiguous"]).sum())
    print(f"{name} M={M}: {touched} of {r['touched'].size} voxels touched, {amb} of them ambiguous ({amb / touched:.4%}), "
          f"behind {r['behind']}, outside {r['outside']}, invalid taps {r['invalid']}")
    assert touched > 0.2 * r["touched"].size
    assert amb <= R.CAP * touched
    assert int(r["ambiguous"].sum()) <= R.CAP * r["touched"].size  # untouched voxels are compared too
    assert r["behind"] > 100 and r["outside"] > 100 and r["invalid"] > 10
    assert (~r["touched"]).sum() > 100  # voxels no map updates
    W = r["W"]
    assert W.dtype == np.float32 and W.max() == (r["touched"].any() and (1 if M == 1 else R.SCENES[name][5]))
    assert (r["T"][~r["touched"]] == 1).all() and (W[~r["touched"]] == 0).all()
    assert r["T"].max() <= 1 and r["T"].min() >= -1


def test_weight_cap_is_restated_in_float32():
    r = R.scene_integrated("room24x32", None, 2.0)
    assert r["W"].max() == 2 and set(np.unique(r["W"])) == {0.0, 1.0, 2.0}
    full = R.scene_integrated("room24x32")
    three = full["W"] == 3
    assert three.any() and (r["W"][three] == 2).all()
    assert (r["T"] == full["T"]).all()  # the cap changes the weight a LATER observation meets: a second pass over the same maps
    dims, v, origin, depth, K, E = R.scene_inputs("room24x32")
    again = [R.integrate(np.stack([x["T"].astype(np.float32), x["W"]], -1), depth, K, E, origin, v, 3.0, mw) for x, mw in ((r, 2.0), (full, 64.0))]
    assert (again[0]["W"][three] == 2).all() and (again[1]["W"][three] == 6).all()
    assert np.abs(again[0]["T"][three] - again[1]["T"][three]).max() > 1e-3


@pytest.mark.parametrize("scene,pose,cam", R.RAYCAST_CASES)
def test_raycast_scenes_stay_under_the_cap_and_hold_their_cases(scene, pose, cam):
    dims, v, origin = R.SCENES[scene][0], R.SCENES[scene][1], R.SCENES[scene][2]
    values = R.reference_values(scene)
    E, iK, H, W = R.live_camera(pose, cam)
    r = R.raycast(values, origin, v, E, iK, H, W, near=R.NEAR, max_steps=R.max_steps_for(v))
    n = H * W
    hits = (r["flags"] & R.HIT) > 0
    print(f"{scene} {pose} {cam}: {hits.sum()} hits of {n}, ambiguous {r['ambiguous'].sum()}, normal-ambiguous {r['normal_ambiguous'].sum()}, "
          f"missed {r['missed'].sum()}, none known {((r['flags'] & R.NONE_KNOWN) > 0).sum()}, some known {((r['flags'] & R.SOME_KNOWN) > 0).sum()}")
    assert r["ambiguous"].sum() <= R.CAP * n
    assert hits.sum() > 0.2 * n
    assert (r["depth"][~hits] == -1).all() and (r["depth"][hits] > R.NEAR * 0.5).all()
    assert not (hits & ((r["flags"] & R.NONE_KNOWN) > 0)).any()
    if pose == "side":
        assert r["missed"].sum() > 5                                        # rays that miss the volume
        assert ((r["flags"] & R.NONE_KNOWN) > 0).sum() > r["missed"].sum()  # rays through unobserved space inside it
    assert ((r["flags"] & R.SOME_KNOWN) > 0).sum() > 10
    # hits in the partial blocks at the high ends
    last = np.array([(d - 2) // 8 for d in dims])
    partial = np.array([(d - 1) % 8 != 0 for d in dims])
    assert partial.all()
    in_partial = hits & (r["hit_cell"] // 8 == last).any(-1)
    assert in_partial.sum() > 5
    nrm = np.linalg.norm(r["normals"], axis=0)
    with_normal = hits & ((r["flags"] & R.NO_NORMAL) == 0)
    assert np.allclose(nrm[with_normal], 1) and (nrm[~with_normal] == 0).all() and with_normal.sum() > 0.9 * hits.sum()


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_block_flags_are_a_superset_that_makes_skipping_exact(name):
    values = R.reference_values(name)
    seen, surf = R.block_flags(values)
    assert seen.shape == tuple((d + 6) // 8 for d in values.shape[:3])
    assert (seen >= surf).all() and surf.any() and (seen == 0).any()
    known = R.known_cells(values)
    for bz, by, bx in zip(*np.nonzero(seen == 0)):
        assert not known[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8].any()  # nothing to find in a block the march jumps
    # a sign change needs a voxel with T < 1 among the corners of the sample at or below zero: those blocks are all flagged
    T = values[..., 0]
    for z, y, x in zip(*np.nonzero(known)):
        if (T[z:z + 2, y:y + 2, x:x + 2] < 1).any():
            assert surf[z // 8, y // 8, x // 8] and seen[z // 8, y // 8, x // 8]


def test_plain_march_ignores_surfaces_entered_from_behind_or_from_unobserved_space():
    """A slab of negative values behind a known positive layer: the ray from the front hits it; a ray that starts inside it, or reaches
    it through unknown cells, marches on."""
    v = R.empty_volume((6, 6, 12))
    v[..., 1] = 1
    v[:, :, 5:8, 0] = -0.5  # a slab across x
    E = np.eye(4, dtype=np.float32)
    E[:3, :3] = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float32)  # the camera looks along +x
    E[:3, 3] = (0.3, 2.4, 2.6)
    iK = np.linalg.inv(R._pinhole(50, 50, 1.0, 1.0)).astype(np.float32)
    kw = dict(near=0.0, max_steps=10)
    front = R.raycast(v, (0, 0, 0), 1.0, E, iK, 2, 2, **kw)
    assert (front["flags"] == R.HIT).all() and np.allclose(front["depth"], 4 + 0.55 / 1.05, atol=2e-2)  # t = 4 and 5: samples at x = 4.3 (f = 0.55) and 5.3 (f = -0.5)
    E2 = E.copy()
    E2[0, 3] = 5.5  # starts inside the slab: f_0 <= 0
    inside = R.raycast(v, (0, 0, 0), 1.0, E2, iK, 2, 2, **kw)
    assert (inside["flags"] & R.HIT == 0).all()
    v[:, :, 3:5, 1] = 0  # the layer in front is not observed
    blind = R.raycast(v, (0, 0, 0), 1.0, E, iK, 2, 2, **kw)
    assert (blind["flags"] == R.SOME_KNOWN).all() and (blind["depth"] == -1).all()
