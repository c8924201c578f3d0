"""Every feature-volume kernel family (csrc/feature_volume.hip: fv_mlp_k<7|8|0, *>, fv_mlp_gen_k<1|2>, fv_mlp_f16_k<7|8|0>; `*`: the all-views
or the view-dropping instantiation, whichever the launch picks for the case's cameras) against the fp64 oracle under general camera geometry: the
four families of tests/volume_geometry.py — random rotations, source cameras whose z = 0 plane cuts the swept volume, camera roll and pitch, and intrinsics that differ for every (b, k) with a current-frame K per batch element.

The other fv tests take their cameras from synthetic.cost_volume_inputs: rotations about y alone and one K for every view and batch element,
for which E[0][1] = E[2][1] = 0 and the indexing src_K + (b * K + k) * 16 / cur_invK + b * 16 of fv_setup_k cannot be told from a constant
(tests/test_volume_geometry_cpu.py shows both, and that every case used here is admissible: the oracle in float32 stays within TOL / 2 of
the oracle in float64 with no mask and next to no `lowest` disagreement).

Measured on an MI355X, scale-relative error against the fp64 oracle: worst over this file's cases per kernel instantiation (variant, family,
seed, shape of the worst case) | the float32 ORACLE against the float64 one on that same case (the admission figure) | the worst of
test_feature_volume_planes_gpu.py (cameras of synthetic.cost_volume_inputs, 120k to 280k voxels):
    fv_mlp_k<7, *>    6.4e-05  k7 zcross 20 (3, 24, 40, 13)       | 4.5e-05 | 8.2e-06
    fv_mlp_k<8, *>    1.6e-05  k8 random 1 (2, 13, 19, 5)         | 1.6e-05 | 5.7e-06
    fv_mlp_k<0, *>    5.3e-06  k0 zcross 2 (2, 13, 19, 5)         | 3.5e-06 | 5.1e-06
    fv_mlp_gen_k<1>   2.3e-05  gen1_16 zcross 8 (2, 13, 19, 5)    | 2.2e-05 | 7.3e-06
    fv_mlp_gen_k<2>   5.4e-06  gen2 intrinsics 4 (2, 13, 19, 5)   | 2.8e-06 | 8.4e-06
    fv_mlp_f16_k<7>   2.4e-05  f16_7 zcross 25 (3, 24, 40, 13)    | 1.6e-05 | 5.8e-06
    fv_mlp_f16_k<8>   5.0e-06  f16_8 zcross 9 (2, 13, 19, 5)      | 6.1e-06 | (not run there)
    fv_mlp_f16_k<0>   1.4e-05  f16_0 zcross 6 (2, 13, 19, 5)      | 3.6e-06 | 5.0e-06
The large figures are the case's, not the kernel's: where a source camera's z = 0 plane cuts the volume (or a random view stands inside it)
samples sit next to the 1e-5 clamp of z, and the reference arithmetic in float32 is as far from float64 as the kernels are (second column).
`lowest` and the mask agreed with the oracle in every pixel of every case (caps 5e-3 and 2e-3).
Wall time of the file on the MI355X host: 2.6 s for the 56 cases (slowest case 0.6 s, the first one; the others at most 0.07 s).
"""
import functools

import pytest
import torch

import test_feature_volume_gpu as base
import test_feature_volume_planes_gpu as planes
import volume_geometry as vg
from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu

# kernel variant -> (source views K, matching channels C, MLP math)
VARIANTS = dict(planes.VARIANTS)
VARIANTS.update({
    "k0_5": (5, 16, "fp32"),      # fv_mlp_k<0, *> with a real view in a quarter's second slot (view 4 = quarter 0, j = 1)
    "gen1_16": (16, 16, "fp32"),  # fv_mlp_gen_k<1>, every slot of four view groups taken
    "f16_8": (8, 16, "f16x3"),    # fv_mlp_f16_k<8>
    "f16_0_5": (5, 16, "f16x3"),  # fv_mlp_f16_k<0>, as k0_5
})
KERNEL = {"k7": "fv_mlp_k<7, *>", "k8": "fv_mlp_k<8, *>", "k0": "fv_mlp_k<0, *>", "k0_5": "fv_mlp_k<0, *>", "gen1": "fv_mlp_gen_k<1>",
          "gen1_16": "fv_mlp_gen_k<1>", "gen2": "fv_mlp_gen_k<2>", "f16_7": "fv_mlp_f16_k<7>", "f16_8": "fv_mlp_f16_k<8>",
          "f16_0": "fv_mlp_f16_k<0>", "f16_0_5": "fv_mlp_f16_k<0>"}

SMALL = (2, 13, 19, 5)     # 247 pixels: the last 16-pixel tile is partial, W is odd, one plane group
GROUPS = (3, 24, 40, 13)   # three frames, several plane groups (asserted with the library's own query)
TWO_SHAPES = ("k7", "gen1", "f16_7")

# Seeds: the variant's position in VARIANTS (+ 20 at the second shape), so that no two variants see the same cameras.  A case that the
# admission test of tests/test_volume_geometry_cpu.py turns down (the float32 ORACLE is not within TOL / 2 of the float64 one there, or
# disagrees on the mask / `lowest`: a sample on an image border or on the z clamp) takes another seed here - the bar is never moved.
REPLACED_SEEDS = {}
SECOND_INTRINSICS_SEED = 50  # added to the seed for the second set of matrices of the two-call check


def seed_of(variant, family, shape):
    s = list(VARIANTS).index(variant) + (20 if shape == GROUPS else 0)
    return REPLACED_SEEDS.get((variant, family, shape), s)


def second_seed_of(variant):
    return REPLACED_SEEDS.get((variant, "intrinsics", "second"), seed_of(variant, "intrinsics", SMALL) + SECOND_INTRINSICS_SEED)


def case_list():
    """(variant, family, shape) of every parametrised case: every variant runs every family at SMALL, three variants also at GROUPS"""
    return [(v, f, s) for v in VARIANTS for s in ((SMALL, GROUPS) if v in TWO_SHAPES else (SMALL,)) for f in vg.FAMILIES]


def oracle_keys():
    """(family, seed, K, C, shape) of every set of inputs this file runs, the second intrinsics of the two-call check included"""
    keys = [(f, seed_of(v, f, s)) + VARIANTS[v][:2] + (s,) for v, f, s in case_list()]
    keys += [("intrinsics", second_seed_of(v)) + VARIANTS[v][:2] + (SMALL,) for v in VARIANTS]
    assert len(set(keys)) == len(keys)
    return keys


@functools.lru_cache(maxsize=None)
def inputs(family, seed, K, C, shape):
    B, H, W, D = shape
    return vg.build_case(family, seed, B, K, C, H, W)


@functools.lru_cache(maxsize=None)
def mlp_weights(K, C):
    return {k: v.detach().clone() for k, v in base._manager(K, 8, 8, 2, 91 + K, C=C).mlp.state_dict().items()}


@functools.lru_cache(maxsize=None)
def oracle(family, seed, K, C, shape):
    """fp64 volume / lowest / mask of the case, computed once and shared (read-only)."""
    return vg.oracle_feature_volume(inputs(family, seed, K, C, shape), shape[3], mlp_weights(K, C))


def _check(m, variant, family, seed, shape):
    K, C, _ = VARIANTS[variant]
    B, H, W, D = shape
    inp = inputs(family, seed, K, C, shape)
    fv, low, _, mask = m(**{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}, return_mask=True)
    torch.cuda.synchronize()
    ref, rlow, rmask = oracle(family, seed, K, C, shape)
    assert fv.shape == (B, D, H, W) and mask.dtype == torch.bool
    finite = bool(torch.isfinite(fv).all()) and bool(torch.isfinite(low).all())
    err = rel_err(fv.cpu(), ref)
    low_off = ((low.cpu().double() - rlow).abs() > 1e-5).float().mean().item()
    mask_off = (mask.cpu() != rmask).float().mean().item()
    print(f"GEOM {KERNEL[variant]} {variant} {family} seed {seed} {shape}: rel err {err:.3e}, lowest off {low_off:.2e}, mask off {mask_off:.2e}")
    assert finite, "non-finite output"
    assert err < TOL, err
    # caps on near ties of the arg-max / the mask's comparisons, as in test_feature_volume_gpu.py (limits, not measurements)
    assert low_off < 5e-3 and mask_off < 2e-3, (low_off, mask_off)
    return fv, low, mask


@pytest.mark.parametrize("variant,family,shape", [pytest.param(v, f, s, id=f"{v}-{f}-" + "x".join(map(str, s))) for v, f, s in case_list()])
def test_general_geometry_vs_oracle(variant, family, shape):
    K, C, math = VARIANTS[variant]
    B, H, W, D = shape
    G, DP = planes._partition(*shape)
    print(f"shape {shape}: partition (G, DP) = {(G, DP)}")
    assert (G >= 2) if shape == GROUPS else (G == 1), f"{shape}: the library now splits the planes as {(G, DP)}"
    m = base._manager(K, H, W, D, 91 + K, C=C)
    m.mlp_math = math
    m.cuda()
    seed = seed_of(variant, family, shape)
    first = _check(m, variant, family, seed, shape)
    if family == "intrinsics" and shape == SMALL:
        # the same manager and shapes with other matrices, then the first again: a pointer or a matrix kept from an earlier call shows here
        _check(m, variant, family, second_seed_of(variant), shape)
        again = _check(m, variant, family, seed, shape)
        assert all(torch.equal(a, b) for a, b in zip(first, again)), "the first inputs give other bits after a call with other matrices"
