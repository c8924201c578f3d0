"""The per-task plane loop of the feature-volume kernels (csrc/feature_volume.hip: fv_mlp_k, fv_mlp_gen_k, fv_mlp_f16_k) with more than four
planes per task, ragged and misaligned plane groups, every NHWC store path, caller-supplied planes and non-dense batch strides — against
the fp64 oracle and against the same frames launched alone (another partition of the planes).

Every case first asks the library for the partition of its shape (idh_feature_volume_plane_groups, the function the launch calls) and
asserts the (groups, planes per group) it was written for: after a retune of the rule these tests fail instead of testing nothing.  Shapes
whose partition changed are found again with the query (neighbouring B, H, W), not by touching the kernel.

Measured on an MI355X, scale-relative error against the fp64 oracle: worst over this file's cases (shape, layout or argument of the worst
case) | the same kernel in the small-shape oracle cases of test_feature_volume_gpu.py / test_mlp_split_gpu.py (at most four planes per
task, 351 to 49152 voxels):
    fv_mlp_k<7, *>    8.2e-06  (6, 45, 65, 7)                  | 3.5e-06  (1, 24, 32, 64)
    fv_mlp_k<8, *>    5.7e-06  (6, 48, 40, 13)                 | 1.8e-06  (1, 12, 20, 5)
    fv_mlp_k<0, *>    5.1e-06  (6, 59, 37, 17), K = 3          | 2.4e-06  (2, 17, 23, 6), K = 5
    fv_mlp_gen_k<1>   7.3e-06  (6, 48, 40, 16), batch strides  | 2.5e-06  (2, 17, 23, 6), K = 12
    fv_mlp_gen_k<2>   8.4e-06  (6, 48, 40, 13)                 | 2.3e-06  (1, 24, 32, 8), K = 7
    fv_mlp_f16_k<7>   5.8e-06  (6, 48, 40, 16), pixel planes   | 3.4e-06  (1, 24, 32, 64)
    fv_mlp_f16_k<0>   5.0e-06  (6, 59, 37, 17), K = 3          | 2.3e-06  (2, 17, 23, 6), K = 5
Two to 3.6 times the small-shape figures, all below a tenth of TOL.  The partition is not the cause: every frame launched alone runs with
at most five planes per task and gives the same bits (_check_partition_independence, torch.equal, held in all 46 cases that run it), so
these voxels carry the same error under the small partitions.  What differs is the sample: the figure is a maximum over 120k to 280k
voxels instead of at most 49k, with a behind-camera and a large-rotation view in every case.  `lowest` was off in at most 8.7e-05 of the
pixels (cap 5e-3), the mask in none.
Wall time of the file on the MI355X host: 8.6 s for the 102 cases (slowest case 0.8 s).
"""
import ctypes
import functools

import pytest
import torch

import implicit_depth_amd.synthetic as syn
from conftest import TOL, rel_err
from oracle import cost_volume as ocv

import test_feature_volume_gpu as base

pytestmark = pytest.mark.gpu

# kernel variant -> (source views K, matching channels C, MLP math)
VARIANTS = {
    "k7": (7, 16, "fp32"),      # fv_mlp_k<7, *>
    "k8": (8, 16, "fp32"),      # fv_mlp_k<8, *>: the plane depth takes the extra MFMA block
    "k0": (3, 16, "fp32"),      # fv_mlp_k<0, *>: absent-view stand-ins in quarters 3 and q + 4
    "gen1": (9, 16, "fp32"),    # fv_mlp_gen_k<1>
    "gen2": (3, 32, "fp32"),    # fv_mlp_gen_k<2>
    "f16_7": (7, 16, "f16x3"),  # fv_mlp_f16_k<7>
    "f16_0": (3, 16, "f16x3"),  # fv_mlp_f16_k<0>
}

# (B, H, W, D) -> (groups, planes per group): what the case exercises
SHAPES = {
    (6, 48, 64, 7): (1, 7),    # one task, tail of 3
    (6, 48, 40, 13): (2, 7),   # second group starts at d0 = 7, ragged 7 + 6
    (3, 48, 64, 14): (3, 5),   # groups of 5, 5, 4; d0 = 5, 10
    (6, 48, 24, 22): (4, 6),   # groups of 6, 6, 6, 4
    (6, 48, 40, 16): (2, 8),   # two full vectors per task, aligned d0
    (6, 64, 64, 9): (1, 9),    # one task of nine planes
    (4, 64, 40, 27): (3, 9),   # groups of 9, 9, 9
    (6, 49, 39, 13): (2, 7),   # odd W, H * W = 16 * 119 + 7: nine dead lanes in the last pixel tile of a 7-plane task, d0 = 7
    (6, 45, 65, 7): (1, 7),    # odd W, H * W % 16 = 13
    (6, 59, 37, 17): (2, 9),   # odd W, H * W % 16 = 7, nine planes per task, ragged 9 + 8, d0 = 9
}
MISALIGNED = (6, 48, 40, 13)  # several groups, d0 % 4 != 0 after the first
DEEP = (6, 48, 40, 16)        # >= 8 planes per task
SUBSET = [MISALIGNED, DEEP, (6, 59, 37, 17)]  # what the variants other than fv_mlp_k<7, *> run

LAYOUTS = ["bdn", "nhwc_vec", "nhwc_odd_cs", "nhwc_offset_base", "nhwc_wide"]


def _partition(B, H, W, D):
    from implicit_depth_amd import _lib

    g, dp = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(_lib.lib().idh_feature_volume_plane_groups(B, H, W, D, ctypes.byref(g), ctypes.byref(dp)), "idh_feature_volume_plane_groups")
    return g.value, dp.value


def _assert_partition(shape):
    got = _partition(*shape)
    print(f"shape {shape}: partition (G, DP) = {got}")
    assert got == SHAPES[shape], f"{shape}: the library now splits the planes as {got}, this case was written for {SHAPES[shape]}"
    return got


def _planes(kind, B, H, W, D):
    """Caller-supplied planes (B, D, H, W) on the CPU, or None.  "pixel": different for every pixel and in no order along d (a kernel that
    indexed the planes by d - d0, or used the prefetched plane d + 1, reads another depth); "batch": a (B, D, 1, 1) tensor, another range and
    another order for every batch element."""
    if kind is None:
        return None
    g = torch.Generator().manual_seed(1234 + D)
    if kind == "pixel":
        return 0.3 + 4.5 * torch.rand(B, D, H, W, generator=g)
    ramp = torch.linspace(0, 1, D)[torch.randperm(D, generator=g)]
    lo, hi = 0.25 + 0.1 * torch.arange(B), 3.0 + 0.4 * torch.arange(B)
    return torch.exp(torch.log(lo)[:, None] + torch.log(hi / lo)[:, None] * ramp[None]).view(B, D, 1, 1)


@functools.lru_cache(maxsize=None)
def _inputs(K, C, shape):
    B, H, W, D = shape
    return syn.cost_volume_inputs(B, K, C, H, W, seed=K + C, behind_view=K - 1, big_rotation_view=0)


@functools.lru_cache(maxsize=None)
def _oracle(K, C, shape, planes_kind=None):
    """fp64 volume / lowest / mask of the case, computed once and shared by every test that compares against it (read-only)."""
    B, H, W, D = shape
    m = base._manager(K, H, W, D, 91 + K, C=C)
    w = {k: v.double() for k, v in m.mlp.state_dict().items()}
    d = {k: v.double() for k, v in _inputs(K, C, shape).items()}
    pl = _planes(planes_kind, B, H, W, D)
    ref, rlow, _, rmask = ocv.feature_volume(d["cur_feats"], d["src_feats"], d["src_extrinsics"], d["src_poses"], d["src_Ks"], d["cur_invK"],
                                             0.25, 5.0, D, w, return_mask=True,
                                             planes_bdhw=None if pl is None else pl.double().expand(B, D, H, W))
    return ref, rlow, rmask


class _Case:
    """Device-side state of one (variant, shape): manager, NHWC features (dense or inside a wider NaN-filled allocation), matrices."""

    def __init__(self, variant, shape, planes_kind=None, strided=False):
        from implicit_depth_amd.cost_volume import to_nhwc

        self.K, self.C, math = VARIANTS[variant]
        self.shape, self.planes_kind = shape, planes_kind
        B, H, W, D = shape
        K, C = self.K, self.C
        self.m = base._manager(K, H, W, D, 91 + K, C=C)
        self.m.mlp_math = math
        self.m.cuda()
        inp = {k: v.cuda() for k, v in _inputs(K, C, shape).items()}
        self.mats = [inp[k] for k in ("src_extrinsics", "src_poses", "src_Ks", "cur_invK")]
        cur, src = to_nhwc(inp["cur_feats"]).view(B, -1), to_nhwc(inp["src_feats"]).view(B, -1)
        self.cur_bs = self.src_bs = 0
        if strided:  # batch strides larger than dense (multiples of 4 floats), NaN between the frames: a wrong stride poisons the result
            self.cur_bs, self.src_bs = cur.shape[1] + 20, src.shape[1] + 36
            wide_c = torch.full((B, self.cur_bs), float("nan"), device="cuda")
            wide_s = torch.full((B, self.src_bs), float("nan"), device="cuda")
            wide_c[:, :cur.shape[1]], wide_s[:, :src.shape[1]] = cur, src
            cur, src = wide_c, wide_s
        self.cur, self.src = cur, src
        pl = _planes(planes_kind, B, H, W, D)
        self.planes = None if pl is None else pl.cuda()

    def run(self, vol_ptr, vol_cs, frame=None):
        """One launch: the whole batch, or frame ``frame`` alone as a batch of one.  -> (lowest, mask)"""
        B, H, W, D = self.shape
        sl = slice(None) if frame is None else slice(frame, frame + 1)
        nb = B if frame is None else 1
        pl = None if self.planes is None else self.planes[sl]
        if pl is not None and pl.shape[2:] == (1, 1):
            pl = pl.expand(nb, D, H, W)  # stride-0 view: passed by stride
        dmin, dmax = (0.25, 5.0) if pl is None else (1.0, 1.0)
        lowest, _, mask = self.m._run(self.cur[sl].data_ptr(), self.src[sl].data_ptr(), (nb, self.K, self.C, H, W),
                                      *[t[sl] for t in self.mats], dmin, dmax, vol_ptr, vol_cs, True, self.cur.device, planes_t=pl,
                                      cur_batch_stride=self.cur_bs, src_batch_stride=self.src_bs)
        torch.cuda.synchronize()
        return lowest, mask

    def run_layout(self, layout, nb=None, frame=None):
        """Launch into a freshly filled buffer of the given layout -> (buffer, (nb, N, D) view of the volume, lowest, mask, rerun)."""
        B, H, W, D = self.shape
        nb, N = nb or B, H * W
        c16 = (D + 15) // 16 * 16
        if layout == "bdn":
            buf = torch.full((nb, D, N), float("nan"), device="cuda")
            view, cs = buf.transpose(1, 2), 0
        else:
            # channel stride, first channel of the slice: aligned vector stores | cs % 4 != 0 | base 4 bytes past a 16-byte boundary |
            # a slice in the middle of a wider concat buffer
            cs, off = {"nhwc_vec": (c16, 0), "nhwc_odd_cs": (D + 1 if (D + 1) % 4 else D + 3, 0), "nhwc_offset_base": (c16 + 16, 1),
                       "nhwc_wide": (c16 + 32, 16)}[layout]
            buf = torch.full((nb, N, cs), 7.0, device="cuda")
            view = buf[..., off:off + D]
            assert buf.data_ptr() % 16 == 0 and (cs % 4 != 0) == (layout == "nhwc_odd_cs")
            assert (view.data_ptr() % 16 != 0) == (layout == "nhwc_offset_base")
        rerun = lambda: self.run(view.data_ptr(), cs, frame)
        lowest, mask = rerun()
        return buf, view, lowest, mask, rerun

    def check_against_oracle(self, view, lowest, mask, what):
        B, H, W, D = self.shape
        ref, rlow, rmask = _oracle(self.K, self.C, self.shape, self.planes_kind)
        err = rel_err(view.transpose(1, 2).reshape(B, D, H, W).cpu(), ref)
        low_off = ((lowest.cpu().double() - rlow).abs() > 1e-5).float().mean().item()
        mask_off = (mask.cpu() != rmask).float().mean().item()
        print(f"{what}: rel err {err:.3e}, lowest off {low_off:.2e}, mask off {mask_off:.2e}")
        assert err < TOL, err
        # caps on near ties of the arg-max / the mask's comparisons, as in test_feature_volume_gpu.py (limits, not measurements)
        assert low_off < 5e-3 and mask_off < 2e-3, (low_off, mask_off)
        return err


def _check_replay_and_padding(view, buf, lowest, mask, rerun, layout):
    """A second launch into the same buffer, its volume elements overwritten with NaN first, gives the same bits (a value left in a wave's `ob`
    from an earlier task, or a tail element nobody writes, shows here); channels of the declared layout outside the slice keep their fill."""
    first = view.clone()
    assert not torch.isnan(first).any(), f"{layout}: volume elements never written"
    view.fill_(float("nan"))
    low2, mask2 = rerun()
    assert torch.equal(view, first) and torch.equal(low2, lowest) and torch.equal(mask2, mask), f"{layout}: replay differs"
    if layout != "bdn":
        pad = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
        off = view.storage_offset() - buf.storage_offset()
        pad[off:off + view.shape[-1]] = False
        assert (buf[..., pad] == 7.0).all(), f"{layout}: channels outside the volume's slice were written"


def _check_partition_independence(case, view, lowest, mask):
    """Every frame launched alone (the library picks another partition for a batch of one) must give the bits of the batched launch: the
    instruction sequence of a voxel does not depend on where its task's plane range starts."""
    B, H, W, D = case.shape
    alone = _partition(1, H, W, D)
    print(f"  batch of one: partition (G, DP) = {alone}")
    assert alone != SHAPES[case.shape], "a batch of one takes the same partition: the comparison would prove nothing"
    for b in range(B):
        _, v1, l1, m1, _ = case.run_layout("bdn", nb=1, frame=b)
        assert torch.equal(v1[0], view[b]), f"frame {b}: volume depends on the plane partition"
        assert torch.equal(l1[0], lowest[b]) and torch.equal(m1[0], mask[b]), f"frame {b}: lowest / mask depend on the plane partition"


def _cases():
    for v in VARIANTS:
        for s in (SHAPES if v == "k7" else SUBSET):
            yield pytest.param(v, s, id=f"{v}-" + "x".join(map(str, s)))


@pytest.mark.parametrize("variant,shape", _cases())
def test_plane_groups_vs_oracle_and_single_frames(variant, shape):
    _assert_partition(shape)
    case = _Case(variant, shape)
    buf, view, lowest, mask, rerun = case.run_layout("bdn")
    case.check_against_oracle(view, lowest, mask, f"{variant} {shape} bdn")
    _check_partition_independence(case, view, lowest, mask)
    _check_replay_and_padding(view, buf, lowest, mask, rerun, "bdn")
    nbuf, nview, nlow, nmask, nrerun = case.run_layout("nhwc_vec")
    assert torch.equal(nview, view) and torch.equal(nlow, lowest) and torch.equal(nmask, mask), "NHWC stores differ from (B, D, N) stores"
    _check_replay_and_padding(nview, nbuf, nlow, nmask, nrerun, "nhwc_vec")


@pytest.mark.parametrize("layout", LAYOUTS[1:])
@pytest.mark.parametrize("shape", [MISALIGNED, DEEP], ids=["misaligned_d0", "deep"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_output_layouts(variant, shape, layout):
    """Vector stores, the scalar fallback (channel stride or base not 16-byte friendly) and slices of wider buffers: only the stores differ
    from the (B, D, N) launch, so the values must be the same bits."""
    _assert_partition(shape)
    case = _Case(variant, shape)
    _, view, lowest, mask, _ = case.run_layout("bdn")
    nbuf, nview, nlow, nmask, nrerun = case.run_layout(layout)
    case.check_against_oracle(nview, nlow, nmask, f"{variant} {shape} {layout}")
    assert torch.equal(nview, view) and torch.equal(nlow, lowest) and torch.equal(nmask, mask), f"{layout} differs from (B, D, N)"
    _check_replay_and_padding(nview, nbuf, nlow, nmask, nrerun, layout)


@pytest.mark.parametrize("kind", ["planes_pixel", "planes_batch", "batch_strides"])
@pytest.mark.parametrize("shape", [MISALIGNED, DEEP], ids=["misaligned_d0", "deep"])
@pytest.mark.parametrize("variant", ["k7", "gen1", "f16_7"])
def test_planes_and_batch_strides(variant, shape, kind):
    """Caller-supplied planes (per pixel; per batch element with pixel stride 0) and feature batch strides larger than dense, with more than
    four planes per task: also the clamped prefetch min(d + 1, d1 - 1) of the next plane at a group's end."""
    _assert_partition(shape)
    case = _Case(variant, shape, planes_kind={"planes_pixel": "pixel", "planes_batch": "batch"}.get(kind), strided=kind == "batch_strides")
    buf, view, lowest, mask, rerun = case.run_layout("bdn")
    case.check_against_oracle(view, lowest, mask, f"{variant} {shape} {kind} bdn")
    _check_partition_independence(case, view, lowest, mask)
    nbuf, nview, nlow, nmask, nrerun = case.run_layout("nhwc_odd_cs" if shape == MISALIGNED else "nhwc_vec")
    assert torch.equal(nview, view) and torch.equal(nlow, lowest) and torch.equal(nmask, mask), "NHWC stores differ from (B, D, N) stores"
    _check_replay_and_padding(nview, nbuf, nlow, nmask, nrerun, "nhwc")
