"""Hand-built ``idh_op`` descriptors for the conv ABI (include/idh_ops.h) and their fp64 reference.

``nhwc.Plan.conv`` only emits the kernel variants its heuristics choose at a given shape; the tests of
test_conv_op_matrix_cpu.py / test_conv_op_matrix_gpu.py build the descriptor themselves, so that every template
instantiation behind ``idh_run_ops`` (csrc/conv.hip: prep_conv, launch_conv, launch_group, launch_level) is reached at a
small shape with row, column and channel tails.  One table of case specs (``CASES``, ``GROUPS``, ``REFUSALS``) serves both
files: each spec names the variant ``idh_conv_variant`` must report - a request that silently ran on another kernel fails
on the CPU already.  That includes the Winograd F(2x2) / F(4x4) and split-precision kernels (tile_m 12 / 13 / 11), whose source-0 weights are packed
by their own pack entry points and whose tolerance follows their own arithmetic (``tolerance``).

Buffers are hostile on purpose: the output is a channel slice of a wider buffer prefilled with a NaN bit pattern, the
residual and dense inputs carry NaN-filled channel padding the kernels have no business reading, split-K workspaces start
as NaN.  Inputs whose channel count is no multiple of 16 live in zero-filled ceil16 buffers, as the header requires.
"""
import ctypes as C
import zlib

import torch
import torch.nn.functional as F

U = 2.0 ** -24  # fp32 unit roundoff
PREFILL = 0x7FC5A5A5  # quiet NaN with a payload: an unwritten output element fails the comparison, a stray store changes the bits
ACT_NONE, ACT_LRELU, ACT_ELU = 0, 1, 2
PAD_ZEROS, PAD_REPLICATE = 0, 1
OK, EINVAL, EUNSUPPORTED, EWORKSPACE = 0, -1, -2, -4
SLOPE = 0.2
K_MAX_GROUP = 12  # kMaxGroup of csrc/conv.hip
K_WINO_MAX_GROUP = 6  # kWinoMaxGroup of csrc/conv_wino.hip
TILE_SPLIT, TILE_WINO, TILE_WINO4 = 11, 12, 13  # IDH_SPLIT_F16X3, IDH_TILE_WINO, IDH_TILE_WINO4 of include/idh_ops.h

# Largest |fp32 F.elu(pre) - fp64 elu(pre)| over the pre-activations of every ELU case of CASES / GROUPS, measured on the CPU by
# test_conv_op_matrix_cpu.py::test_elu_constant_covers_the_cpu_measurement (which fails if a case exceeds it): 2.381e-7, mostly the
# rounding of the largest pre-activations (|pre| ~ 4) to fp32.  The device's exp may be a few ulp looser: the tolerance adds 4x this.
ELU_F32_ERR = 2.4e-7


def ceil16(v):
    return (v + 15) & ~15


class Src:
    """One conv source.  hw = input size (default: the output's for stride 1, (2Ho-1, 2Wo-1) for stride 2);
    up = (up_c0, up_C, (up_cs0[, up_cs1])): fused x2-upsampled segments; norm: normalise on load."""

    def __init__(self, cin, ks=3, stride=1, hw=None, up=None, norm=False):
        self.cin, self.ks, self.stride, self.hw, self.up, self.norm = cin, ks, stride, hw, up, norm


class Spec:
    """variant = what idh_conv_variant must answer: (lds_rows, nj, tm, tn, S after clamping, up, norm, s2)."""

    kind = "conv"

    def __init__(self, name, N, Ho, Wo, cout, srcs, tile_m, tile_n, variant, pad=PAD_ZEROS, split_k=1, bias=True, res=True,
                 act=ACT_LRELU, slope=SLOPE):
        self.name, self.N, self.Ho, self.Wo, self.cout, self.srcs = name, N, Ho, Wo, cout, tuple(srcs)
        self.tile_m, self.tile_n, self.variant, self.pad, self.split_k = tile_m, tile_n, tuple(variant), pad, split_k
        self.bias, self.res, self.act, self.slope = bias, res, act, slope

    @property
    def family(self):  # which source file the kernel lives in - and which error model the tolerance takes
        return {TILE_SPLIT: "split", TILE_WINO: "wino", TILE_WINO4: "wino4"}.get(self.tile_m, "lds" if self.variant[0] else "direct")

    @property
    def template(self):
        """The template arguments launch_conv_wino / launch_conv_wino4 / launch_conv_split choose and idh_conv_variant does not show."""
        src2 = len(self.srcs) > 1
        if self.family == "wino":
            return ("conv3x3_wino_k", src2)
        if self.family == "wino4":
            return ("conv3x3_wino4_k", src2, self.res and not src2)  # <PROJ, RES>
        if self.family == "split":
            return ("conv3x3_split_k", src2, self.variant[3])  # <SRC2> x tile rows
        return None

    def in_hw(self, s):
        if s.hw is not None:
            return s.hw
        return (self.Ho, self.Wo) if s.stride == 1 else (2 * self.Ho - 1, 2 * self.Wo - 1)

    @property
    def S(self):
        return self.variant[4]

    @property
    def branch(self):  # the launch_conv branch: the variant without the split count
        return self.variant[:4] + self.variant[5:]

    @property
    def launches(self):  # the conv, plus the reduce of its partials
        return 1 + (self.S > 1)

    @property
    def K(self):
        return sum(s.ks * s.ks * s.cin for s in self.srcs)


class UpSpec:
    """An IDH_OP_UPSAMPLE2 member of a level launch."""

    kind = "up"

    def __init__(self, name, N, H, W, Cch):
        self.name, self.N, self.H, self.W, self.C = name, N, H, W, Cch


# ------------------------------------------------------------------------------------------------------------------
# case table
# ------------------------------------------------------------------------------------------------------------------
DIRECT_COUT = {4: 60, 2: 28, 1: 20}  # the last channel quad(s) of the last 16-channel sub-tile are masked (co >= Cout)
NJ = {0: 4, 2: 2, 1: 1}
EPILOGUES = [(b, r, a) for (b, r) in ((False, False), (True, False), (True, True)) for a in (ACT_NONE, ACT_LRELU, ACT_ELU)]
ACT_NAME = {ACT_NONE: "none", ACT_LRELU: "lrelu", ACT_ELU: "elu"}


def _direct(name, tm, tn, srcs, Ho=7, Wo=9, split_k=1, S=1, **kw):
    # N = 2, 7 x 9: M = 126 (stride 2: 2 x 4 x 5 = 40) is no multiple of 16, 32 or 64 - every TM has a row tail
    return Spec(name, 2, Ho, Wo, DIRECT_COUT[tn], srcs, tm, tn, (0, 0, tm, tn, S, 0, 0, 0), split_k=split_k, **kw)


def _lds(name, tm, tn, cout, srcs, Ho=9, Wo=19, N=2, split_k=1, S=1, up=0, norm=0, s2=0, **kw):
    # 9 x 19: row and column tails at both tile heights (8 / 4 rows x 16 columns)
    return Spec(name, N, Ho, Wo, cout, srcs, tm, tn, (8 if tm == 8 else 4, NJ[tn], 0, 0, S, up, norm, s2), split_k=split_k, **kw)


def _wino(name, cout, srcs, Ho=9, Wo=35, N=2, **kw):
    # 9 x 35: row and column tails against the 32 x 8 tiles and the 2 x 2 output blocks (Ho, Wo odd)
    return Spec(name, N, Ho, Wo, cout, srcs, TILE_WINO, 0, (32, 0, TILE_WINO, 0, 1, 0, 0, 0), **kw)


def _wino4(name, cout, srcs, Ho=9, Wo=35, N=2, **kw):
    # 9 x 35: tails against the 32 x 8 tile groups and the 4 x 4 output blocks (9 = 2 * 4 + 1, 35 = 8 * 4 + 3)
    return Spec(name, N, Ho, Wo, cout, srcs, TILE_WINO4, 0, (36, 0, TILE_WINO4, 0, 1, 0, 0, 0), **kw)


def _split(name, tn, cout, srcs, Ho=9, Wo=35, N=2, **kw):
    # 9 x 35: tails against the 16 x 16 and 8 x 16 tiles; tile_n = 8 -> 8-row tiles, 0 / 16 -> 16 rows
    return Spec(name, N, Ho, Wo, cout, srcs, TILE_SPLIT, tn, (16, 0, TILE_SPLIT, 8 if tn == 8 else 16, 1, 0, 0, 0), **kw)


def _epi(b, r, a):
    return f"{'bias' if b else 'nobias'}{'-res' if r else ''}-{ACT_NAME[a]}"


def _cases():
    cs = []
    # ---- direct kernel ------------------------------------------------------------------------------------------
    for tm in (1, 2, 4):
        for tn in (1, 2, 4):
            cs.append(_direct(f"direct-{tm}x{tn}-3x3", tm, tn, [Src(24)]))
    for tm, tn in ((4, 4), (1, 1)):
        t = f"direct-{tm}x{tn}"
        cs.append(_direct(f"{t}-3x3s2", tm, tn, [Src(24, 3, 2, hw=(7, 9))], Ho=4, Wo=5))
        cs.append(_direct(f"{t}-1x1", tm, tn, [Src(24, 1)]))
        cs.append(_direct(f"{t}-1x1s2", tm, tn, [Src(24, 1, 2, hw=(7, 9))], Ho=4, Wo=5))
        cs.append(_direct(f"{t}-replicate", tm, tn, [Src(24)], pad=PAD_REPLICATE))
        cs.append(_direct(f"{t}-replicate-s2", tm, tn, [Src(24, 3, 2, hw=(7, 9))], Ho=4, Wo=5, pad=PAD_REPLICATE))
        cs.append(_direct(f"{t}-proj1x1", tm, tn, [Src(24), Src(32, 1)]))
        cs.append(_direct(f"{t}-proj1x1s2", tm, tn, [Src(24), Src(32, 1, 2)]))  # source 1 is 13 x 17
        # one source: 9 taps x 2 channel blocks = 18 steps; 3 -> 6 steps each, 18 -> one step each (the ping-pong loop's null step), 23 clamps to 18
        for sk, S in ((2, 2), (3, 3), (18, 18), (23, 18)):
            cs.append(_direct(f"{t}-split{sk}", tm, tn, [Src(24)], split_k=sk, S=S))
        # two sources: 18 + 2 steps; 3 -> 6 / 7 / 7 steps (odd counts), 10 -> 2 steps each and split 9 starts exactly at source 1
        for sk in (3, 10):
            cs.append(_direct(f"{t}-proj1x1-split{sk}", tm, tn, [Src(24), Src(32, 1)], split_k=sk, S=sk))
            cs.append(_direct(f"{t}-proj1x1s2-split{sk}", tm, tn, [Src(24), Src(32, 1, 2)], split_k=sk, S=sk))
    for b, r, a in EPILOGUES:
        e = f"{'bias' if b else 'nobias'}{'-res' if r else ''}-{ACT_NAME[a]}"
        cs.append(_direct(f"direct-4x4-epi-{e}", 4, 4, [Src(24)], bias=b, res=r, act=a))
        cs.append(_direct(f"direct-1x1-split3-epi-{e}", 1, 1, [Src(24)], split_k=3, S=3, bias=b, res=r, act=a))
    # a request the LDS kernel cannot take (Wo < 16) runs on the direct kernel with its default 64-pixel tile: only the query tells
    cs.append(Spec("direct-fallthrough-from-8row", 2, 7, 9, 60, [Src(24)], 8, 0, (0, 0, 4, 4, 1, 0, 0, 0)))
    # ---- LDS kernel ---------------------------------------------------------------------------------------------
    for tm in (8, 9):
        shapes = [(0, 64), (2, 64), (1, 64), (2, 96), (1, 48)]
        for tn, cout in shapes:
            # Cin = 40: three chunks, the last one padded
            cs.append(_lds(f"lds{tm}-n{tn}-c{cout}", tm, tn, cout, [Src(40)]))
            cs.append(_lds(f"lds{tm}-n{tn}-c{cout}-replicate", tm, tn, cout, [Src(40)], pad=PAD_REPLICATE))
        cs.append(_lds(f"lds{tm}-n0-w16", tm, 0, 64, [Src(40)], Wo=16))
        # 1x1 second source of 80 channels = 5 chunks: one full lds_g1 round (4 / 3 / 2 / 1 chunks per round over RW x NJ) plus a remainder.
        # cost units T = 9 * 3 + 5 = 32: at most T / 9 = 3 splits
        for tn in (0, 2, 1):
            for sk, S in ((1, 1), (2, 2), (3, 3), (9, 3)):
                cs.append(_lds(f"lds{tm}-n{tn}-proj1x1-split{sk}", tm, tn, 64, [Src(40), Src(80, 1)], split_k=sk, S=S))
        # 3x3 stride-2 second source, odd and even input sizes (both give 9 x 19)
        for tn in (0, 2):
            for hw in ((17, 37), (18, 38)):
                for sk in (1, 2):
                    cs.append(_lds(f"lds{tm}-n{tn}-proj3x3s2-{hw[0]}x{hw[1]}-split{sk}", tm, tn, 64, [Src(40), Src(24, 3, 2, hw=hw)],
                                   split_k=sk, S=sk, s2=1))
        # lone 3x3 stride-2 source: runs as the stride-2 second source behind an empty first one
        for tn, cout in ((0, 64), (2, 96)):
            for hw in ((17, 37), (18, 38)):
                cs.append(_lds(f"lds{tm}-n{tn}-lone3x3s2-{hw[0]}x{hw[1]}", tm, tn, cout, [Src(24, 3, 2, hw=hw)], s2=1))
        # normalise on load
        for pad in (PAD_ZEROS, PAD_REPLICATE):
            cs.append(_lds(f"lds{tm}-norm-{'replicate' if pad else 'zeros'}", tm, 1, 16, [Src(32, norm=True)], pad=pad, norm=1))
        # fused upsample: 10 x 18 (row tail at 8 and at 4 rows, column tail), 32-channel segments behind 0 / 16 direct channels
        for c0 in (0, 16):
            for nseg, ucs in ((1, (36,)), (2, (36, 44))):
                for sk in (1, 2):
                    cs.append(_lds(f"lds{tm}-up-c{c0}-seg{nseg}-split{sk}", tm, 0, 64, [Src(c0 + 32 * nseg, up=(c0, 32, ucs))],
                                   Ho=10, Wo=18, split_k=sk, S=sk, up=1))
    # ---- Winograd F(2x2, 3x3): conv3x3_wino_k<4, 2, 8, SRC2> (32 x 8 pixel x 32 channel tiles) ---------------------------------
    for b, r, a in EPILOGUES:  # Cin = 40: a zero-filled ceil16 buffer, K steps of 8 channels
        cs.append(_wino(f"wino-epi-{_epi(b, r, a)}", 64, [Src(40)], bias=b, res=r, act=a))
    for cout in (32, 96):  # NT = 1, 3 (64: above)
        cs.append(_wino(f"wino-c{cout}", cout, [Src(40)]))
    cs.append(_wino("wino-cin16", 64, [Src(16)]))  # two K steps: the fewest the store / residual schedule allows
    cs.append(_wino("wino-5x7", 64, [Src(40)], Ho=5, Wo=7))  # a map smaller than one tile
    for c1 in (24, 80):  # P steps of 32 channels: one half-empty step / two steps and a half-empty third
        for r in (False, True):
            cs.append(_wino(f"wino-proj{c1}{'-res' if r else ''}", 64, [Src(40), Src(c1, 1)], res=r))
    cs.append(_wino("wino-proj24-nobias-elu", 32, [Src(40), Src(24, 1)], bias=False, res=False, act=ACT_ELU))
    # ---- Winograd F(4x4, 3x3): conv3x3_wino4_k<PROJ, RES> (32 x 8 pixel x 64 channel tiles) ------------------------------------
    for b, r, a in EPILOGUES:  # <false, false> and <false, true> with each activation
        cs.append(_wino4(f"wino4-epi-{_epi(b, r, a)}", 64, [Src(40)], bias=b, res=r, act=a))
    for c1 in (16, 24, 112):  # <true, false>: one chunk, a padded chunk, an odd chunk count (the P phase double-buffers its chunks)
        for a in (ACT_NONE, ACT_LRELU, ACT_ELU):
            cs.append(_wino4(f"wino4-proj{c1}-{ACT_NAME[a]}", 64, [Src(40), Src(c1, 1)], res=False, act=a))
    cs.append(_wino4("wino4-proj24-nobias", 64, [Src(40), Src(24, 1)], bias=False, res=False))
    for sl in (0.0, 1.0):  # LeakyReLU is max(x, slope x): the ends of the accepted range
        cs.append(_wino4(f"wino4-slope{sl:g}", 64, [Src(40)], res=False, slope=sl))
        cs.append(_wino4(f"wino4-res-slope{sl:g}", 64, [Src(40)], slope=sl))
        cs.append(_wino4(f"wino4-proj24-slope{sl:g}", 64, [Src(40), Src(24, 1)], res=False, slope=sl))
    cs.append(_wino4("wino4-c192", 192, [Src(40)]))
    cs.append(_wino4("wino4-cin17", 64, [Src(17)]))    # the smallest accepted: two 16-channel blocks, 15 channels of padding
    cs.append(_wino4("wino4-cin136", 64, [Src(136)]))  # deep: 17 stages, an odd number of 16-channel stage pairs
    cs.append(_wino4("wino4-5x7", 64, [Src(40)], Ho=5, Wo=7))
    # more tiles than the persistent grid of 2 x 256 workgroups: 171 images x 1 tile group x 3 channel tiles = 513 (= 1 mod 8)
    cs.append(_wino4("wino4-513-tiles", 192, [Src(24)], Ho=5, Wo=7, N=171))
    # ---- split precision: conv3x3_split_k<4, G, f16x3, SRC2> (16 / 8 rows x 16 columns x 64 channels) -----------------------------
    for b, r, a in EPILOGUES:
        cs.append(_split(f"split-epi-{_epi(b, r, a)}", 0, 64, [Src(40)], bias=b, res=r, act=a))
    for tn in (0, 8, 16):
        for cout in (64, 128):
            cs.append(_split(f"split-n{tn}-c{cout}", tn, cout, [Src(40)]))
            cs.append(_split(f"split-n{tn}-c{cout}-proj1x1", tn, cout, [Src(40), Src(48, 1)]))  # (a dense buffer of 56 with NaN padding)
    for tn in (8, 16):
        cs.append(_split(f"split-n{tn}-5x16", tn, 64, [Src(40)], Ho=5, Wo=16))  # smaller than one tile; Wo = 16 is the narrowest accepted
        cs.append(_split(f"split-n{tn}-19x35-proj1x1", tn, 64, [Src(24), Src(48, 1)], Ho=19, Wo=35))  # two / three tile rows, the last one short
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = _cases()

# Every kernel launch_conv (csrc/conv.hip) can pick, written out in idh_conv_variant's numbering (lds_rows, nj, tm, tn, up, norm, s2): the non-null
# entries of its tables kLdsRow<rows / 4>[nj][flavour] (14) and kDirectKernels[tm][tn] (9), and the launchers of the other three kernels.
# A new table entry needs a line here and a case above, or test_conv_op_matrix_cpu.py::test_every_launch_conv_branch_has_a_case fails.
LAUNCH_CONV_BRANCHES = {
    (16, 0, TILE_SPLIT, 16, 0, 0, 0),  # launch_conv_split: conv3x3_split_k<4, 2, f16x3, SRC2>
    (16, 0, TILE_SPLIT, 8, 0, 0, 0),   # launch_conv_split: conv3x3_split_k<4, 1, f16x3, SRC2>
    (32, 0, TILE_WINO, 0, 0, 0, 0),    # launch_conv_wino: conv3x3_wino_k<4, 2, 8, SRC2>
    (36, 0, TILE_WINO4, 0, 0, 0, 0),   # launch_conv_wino4: conv3x3_wino4_k<PROJ, RES>
    (8, 4, 0, 0, 1, 0, 0),  # conv3x3_lds_up_k<2>
    (8, 4, 0, 0, 0, 0, 1),  # conv3x3_lds_k<2, false, 4, false, true>
    (8, 2, 0, 0, 0, 0, 1),  # conv3x3_lds_k<2, false, 2, false, true>
    (4, 4, 0, 0, 0, 0, 1),  # conv3x3_lds_k<1, false, 4, false, true>
    (4, 2, 0, 0, 0, 0, 1),  # conv3x3_lds_k<1, false, 2, false, true>
    (8, 1, 0, 0, 0, 1, 0),  # conv3x3_lds_k<2, false, 1, true>
    (4, 1, 0, 0, 0, 1, 0),  # conv3x3_lds_k<1, false, 1, true>
    (8, 2, 0, 0, 0, 0, 0),  # conv3x3_lds_k<2, false, 2>
    (8, 1, 0, 0, 0, 0, 0),  # conv3x3_lds_k<2, false, 1>
    (4, 2, 0, 0, 0, 0, 0),  # conv3x3_lds_k<1, false, 2>
    (4, 1, 0, 0, 0, 0, 0),  # conv3x3_lds_k<1, false, 1>
    (8, 4, 0, 0, 0, 0, 0),  # conv3x3_lds_k<2, false>
    (4, 4, 0, 0, 1, 0, 0),  # conv3x3_lds_up_k<1>
    (4, 4, 0, 0, 0, 0, 0),  # conv3x3_lds_k<1, false>
    (0, 0, 4, 4, 0, 0, 0), (0, 0, 2, 4, 0, 0, 0), (0, 0, 1, 4, 0, 0, 0),  # conv_mfma_k<TM, TN>
    (0, 0, 4, 2, 0, 0, 0), (0, 0, 2, 2, 0, 0, 0), (0, 0, 1, 2, 0, 0, 0),
    (0, 0, 4, 1, 0, 0, 0), (0, 0, 2, 1, 0, 0, 0), (0, 0, 1, 1, 0, 0, 0),
}

# The kernel templates behind the first three branches of launch_conv that the variant tuple does not distinguish (Spec.template), and the two
# of launch_conv_wino_group: test_conv_op_matrix_cpu.py::test_every_hidden_kernel_template_has_a_case asserts CASES / GROUPS reach exactly these.
KERNEL_TEMPLATES = {
    ("conv3x3_wino_k", False), ("conv3x3_wino_k", True),
    ("conv3x3_wino4_k", False, False), ("conv3x3_wino4_k", False, True), ("conv3x3_wino4_k", True, False),
    ("conv3x3_split_k", False, 16), ("conv3x3_split_k", True, 16), ("conv3x3_split_k", False, 8), ("conv3x3_split_k", True, 8),
}
GROUP_KERNEL_TEMPLATES = {("conv3x3_wino_group_k", False), ("conv3x3_wino_group_k", True)}


def _groups():
    """(name, members, launches): members share a non-zero group id and have disjoint buffers."""
    gs = []
    # 4-row groups, one per channel tile, members of different shapes: conv3x3_lds_group_k<1, false, NJ>
    for tn, couts in ((0, (64, 128, 64)), (2, (64, 96, 32)), (1, (48, 16, 32))):
        m = [_lds(f"g-n{tn}-a", 9, tn, couts[0], [Src(40)]),
             _lds(f"g-n{tn}-b", 9, tn, couts[1], [Src(16)], N=1, Ho=5, Wo=16, pad=PAD_REPLICATE),
             _lds(f"g-n{tn}-c", 9, tn, couts[2], [Src(24), Src(48, 1)], N=1, Ho=12, Wo=33)]
        gs.append((f"group-4row-n{tn}", m, 1))
    # a fused-upsample member next to a plain one: conv3x3_lds_group_k<1, true> hosts both loaders
    gs.append(("group-4row-up-and-plain",
               [_lds("g-up-a", 9, 0, 64, [Src(80, up=(16, 32, (36, 44)))], Ho=10, Wo=18, up=1),
                _lds("g-up-b", 9, 0, 64, [Src(40), Src(48, 1)]),
                _lds("g-up-c", 9, 0, 64, [Src(32, up=(0, 32, (36,)))], N=1, Ho=6, Wo=20, up=1)], 1))
    # two split members (M * Cout = 342 * 64 and 80 * 64 + ... are no multiples of 256) and an unsplit one: one conv grid + ONE reduce grid
    gs.append(("group-4row-two-splits",
               [_lds("g-sp-a", 9, 0, 64, [Src(40)], split_k=2, S=2),
                _lds("g-sp-b", 9, 0, 64, [Src(40)], act=ACT_ELU),
                _lds("g-sp-c", 9, 0, 64, [Src(40), Src(80, 1)], N=1, Ho=5, Wo=17, split_k=3, S=3, res=False)], 2))
    # heterogeneous level: 64- and 32-channel 4-row LDS convs, the 16x64 direct conv at stride 2, a bilinear upsample -> level_k<true>
    level = lambda t: [_lds(f"{t}-lds32", 9, 2, 96, [Src(40)]),
                       Spec(f"{t}-direct14s2", 2, 4, 5, 64, [Src(24, 3, 2, hw=(7, 9))], 1, 4, (0, 0, 1, 4, 1, 0, 0, 0)),
                       UpSpec(f"{t}-up2", 2, 5, 7, 24)]
    gs.append(("level-wide", [_lds("lv-w-lds64", 9, 0, 64, [Src(40)])] + level("lv-w"), 1))
    gs.append(("level-narrow", level("lv-n"), 1))  # level_k<false>
    # a run longer than kMaxGroup: the first 12 share a grid, the 13th runs alone
    gs.append(("group-longer-than-kmaxgroup", [_lds(f"g-long-{i}", 9, 0, 64, [Src(16)], N=1, Ho=4, Wo=16) for i in range(K_MAX_GROUP + 1)], 2))
    # ---- grouped F(2x2) launches: conv3x3_wino_group_k<4, 2, 8, SRC2>, one persistent grid for up to kWinoMaxGroup members -------------
    gs.append(("wino-group-three-shapes",
               [_wino("wg-a", 64, [Src(40)]),
                _wino("wg-b", 32, [Src(16)], N=1, Ho=5, Wo=7, act=ACT_ELU),
                _wino("wg-c", 96, [Src(24)], N=1, Ho=12, Wo=33, res=False)], 1))
    # a run longer than kWinoMaxGroup: the first 6 share a grid, the 7th runs alone
    gs.append(("wino-group-longer-than-kwinomaxgroup",
               [_wino(f"wg-long-{i}", 32, [Src(16)], N=1, Ho=4 + i, Wo=33 + i) for i in range(K_WINO_MAX_GROUP + 1)], 2))
    # members without a second source, then members with one: the run splits where the kind of source 1 changes -> two grids
    gs.append(("wino-group-plain-then-projected",
               [_wino("wg-mix-a", 64, [Src(40)]),
                _wino("wg-mix-b", 32, [Src(16)], N=1, Ho=5, Wo=33),
                _wino("wg-mix-c", 64, [Src(40), Src(24, 1)], res=False),
                _wino("wg-mix-d", 32, [Src(16), Src(80, 1)], N=1, Ho=10, Wo=20)], 2))
    # 1 + 2 tiles: the grid is still 8 workgroups (whole XCD octets), five of them without a tile
    gs.append(("wino-group-fewer-than-8-tiles",
               [_wino("wg-tiny-a", 32, [Src(16)], N=1, Ho=5, Wo=7),
                _wino("wg-tiny-b", 64, [Src(24)], N=1, Ho=3, Wo=9, act=ACT_NONE)], 1))
    return gs


GROUPS = _groups()


def _refusals():
    """(name, spec, mutation of the built op, expected code).  The spec's variant is unused."""
    base = lambda **kw: _direct("r", 4, 4, [Src(24)], **kw)
    no_ws = lambda op: setattr(op, "ws", None)

    def set_(**kw):
        def f(op):
            for k, v in kw.items():
                setattr(op, k, v)
        return f

    rs = [
        ("cout-not-multiple-of-4", base(), set_(Cout=58), EINVAL),
        ("out-cs-not-multiple-of-4", base(), set_(out_cs=70), EINVAL),
        ("out-not-16-byte-aligned", base(), lambda op: setattr(op, "out", op.out + 4), EINVAL),
        ("ho-inconsistent", base(), set_(Ho=8), EINVAL),
        ("ho-inconsistent-stride2", _direct("r", 4, 4, [Src(24, 3, 2, hw=(7, 9))], Ho=4, Wo=5), set_(Ho=3), EINVAL),
        ("tile-n-does-not-divide", _direct("r", 4, 2, [Src(24)]), set_(tile_n=4), EINVAL),  # ceil16(28) / 16 = 2 sub-tiles
        ("split-without-workspace-direct", base(split_k=3, S=3), no_ws, EWORKSPACE),
        ("clamped-split-without-workspace-direct", base(split_k=23, S=18), no_ws, EWORKSPACE),
        ("split-without-workspace-lds", _lds("r", 8, 0, 64, [Src(40), Src(80, 1)], split_k=9, S=3), no_ws, EWORKSPACE),
        # split_k that clamps to 1: accepted without a workspace (direct: a single step; LDS: a single chunk)
        ("split-clamps-to-1-direct", _direct("r", 4, 4, [Src(16, 1)], split_k=3, S=1), no_ws, OK),
        ("split-clamps-to-1-lds", _lds("r", 9, 0, 64, [Src(16)], split_k=4, S=1), no_ws, OK),
        ("up-with-32-channel-tiles", _lds("r", 9, 2, 64, [Src(48, up=(16, 32, (36,)))], Ho=10, Wo=18, up=1), None, EUNSUPPORTED),
        ("up-with-16-channel-tiles", _lds("r", 8, 1, 64, [Src(48, up=(16, 32, (36,)))], Ho=10, Wo=18, up=1), None, EUNSUPPORTED),
        ("up-on-the-direct-kernel", _lds("r", 8, 0, 64, [Src(48, up=(16, 32, (36,)))], Ho=10, Wo=14, up=1), None, EUNSUPPORTED),  # Wo < 16
        ("norm-with-64-channel-tiles", _lds("r", 8, 0, 64, [Src(32, norm=True)], norm=1), None, EUNSUPPORTED),
        ("norm-with-32-channel-tiles", _lds("r", 9, 2, 64, [Src(32, norm=True)], norm=1), None, EUNSUPPORTED),
        ("norm-on-the-direct-kernel", _direct("r", 1, 1, [Src(32, norm=True)]), None, EUNSUPPORTED),
        # ---- Winograd F(2x2) / F(4x4) and split precision: what the header promises IDH_EUNSUPPORTED for --------------------------------------
    ]
    fams = (("wino", lambda srcs, **kw: _wino("r", 64, srcs, **kw)), ("wino4", lambda srcs, **kw: _wino4("r", 64, srcs, **kw)),
            ("split", lambda srcs, **kw: _split("r", 0, 64, srcs, **kw)))
    for f, mk in fams:
        rs += [
            (f"{f}-replicate-padding", mk([Src(40)], pad=PAD_REPLICATE), None, EUNSUPPORTED),
            (f"{f}-stride-2", mk([Src(40, 3, 2)]), None, EUNSUPPORTED),  # (a 17 x 69 input)
            (f"{f}-split-k-2", mk([Src(40)], split_k=2), None, EUNSUPPORTED),  # (with a workspace: the refusal is the kernel's, not IDH_EWORKSPACE)
            (f"{f}-fused-upsample", mk([Src(48, up=(16, 32, (36,)))], Ho=10, Wo=34), None, EUNSUPPORTED),
            (f"{f}-normalise-on-load", mk([Src(32, norm=True)]), None, EUNSUPPORTED),
        ]
    rs += [
        ("wino-cout-48", _wino("r", 48, [Src(40)]), None, EUNSUPPORTED),
        ("wino4-cout-96", _wino4("r", 96, [Src(40)]), None, EUNSUPPORTED),
        ("wino4-cin-16", _wino4("r", 64, [Src(16)]), None, EUNSUPPORTED),
        ("wino4-projection-with-residual", _wino4("r", 64, [Src(40), Src(24, 1)], res=True), None, EUNSUPPORTED),
        ("wino4-lrelu-slope-negative", _wino4("r", 64, [Src(40)]), set_(slope=-0.1), EUNSUPPORTED),
        ("wino4-lrelu-slope-above-1", _wino4("r", 64, [Src(40)]), set_(slope=1.5), EUNSUPPORTED),
        ("split-cout-96", _split("r", 0, 96, [Src(40)]), None, EUNSUPPORTED),
        ("split-wo-15", _split("r", 0, 64, [Src(40)], Wo=15), None, EUNSUPPORTED),
        ("split-tile-n-4", _split("r", 0, 64, [Src(40)]), set_(tile_n=4), EUNSUPPORTED),
        # the second source of the split-precision kernel is a 1x1 stride-1 projection of an output-sized tensor, nothing else: the kernel walks
        # src[1] with source 0's H / W and reads one tap of weights per chunk
        ("split-3x3-stride-2-second-source", _split("r", 0, 64, [Src(40), Src(24, 3, 2)]), None, EUNSUPPORTED),
        ("split-1x1-stride-2-second-source", _split("r", 0, 64, [Src(40), Src(24, 1, 2)]), None, EUNSUPPORTED),
        ("split-upsampled-second-source", _split("r", 0, 64, [Src(40), Src(48, 1, up=(16, 32, (36,)))], Ho=10, Wo=34), None, EUNSUPPORTED),
    ]
    return rs


REFUSALS = _refusals()


# ------------------------------------------------------------------------------------------------------------------
# descriptors
# ------------------------------------------------------------------------------------------------------------------
OUT_C0 = 4  # the output is channels [4, 4 + Cout) of a buffer of Cout + 8


def buffer_layout(spec):
    """Channel strides of every buffer of a conv case (what build_op writes into the descriptor)."""
    lay = {"out_cs": spec.cout + 8, "res_cs": spec.cout + 4, "in_cs": []}
    for s in spec.srcs:
        if s.up:
            lay["in_cs"].append(s.up[0] + 8 if s.up[0] else 16)
        else:
            lay["in_cs"].append(ceil16(s.cin) if s.cin % 16 else s.cin + 8)
    return lay


def build_op(nhwc, spec, ptr, group=0):
    """The idh_op of a conv spec; ptr(name) -> device address of "x0", "x1", "w0", "w1", "up0_0", ..., "norm0", "bias", "res", "out"
    (the wider output buffer), "ws"."""
    lay = buffer_layout(spec)
    op = nhwc.Op()
    op.kind, op.N = nhwc.OP_CONV, spec.N
    for i, s in enumerate(spec.srcs):
        d = op.src[i]
        H, W = spec.in_hw(s)
        d.in_, d.w, d.cs, d.H, d.W, d.Cin, d.ks, d.stride, d.pad_mode = ptr(f"x{i}"), ptr(f"w{i}"), lay["in_cs"][i], H, W, s.cin, s.ks, s.stride, spec.pad
        if s.up:
            c0, uC, ucs = s.up
            d.up_c0, d.up_C = c0, uC
            for j, v in enumerate(ucs):
                d.up_in[j], d.up_cs[j] = ptr(f"up{i}_{j}"), v
        if s.norm:
            d.norm, d.norm_slope, d.norm_act = ptr(f"norm{i}"), SLOPE, ACT_LRELU
    op.bias = ptr("bias") if spec.bias else None
    op.res = ptr("res") if spec.res else None
    op.res_cs = lay["res_cs"] if spec.res else 0
    op.out, op.out_cs = ptr("out") + 4 * OUT_C0, lay["out_cs"]
    op.ws = ptr("ws") if spec.split_k > 1 else None
    op.Ho, op.Wo, op.Cout, op.act, op.slope = spec.Ho, spec.Wo, spec.cout, spec.act, spec.slope
    op.split_k, op.tile_m, op.tile_n, op.group = spec.split_k, spec.tile_m, spec.tile_n, group
    return op


def build_up_op(nhwc, spec, ptr, group=0):
    op = nhwc.Op()
    op.kind, op.N, op.group = nhwc.OP_UPSAMPLE2, spec.N, group
    s = op.src[0]
    s.in_, s.cs, s.H, s.W, s.Cin = ptr("x0"), spec.C + 4, spec.H, spec.W, spec.C
    op.out, op.out_cs = ptr("out") + 4 * OUT_C0, spec.C + 8
    return op


def fake_ptr(name):
    """16-byte-aligned made-up addresses for the dry-run entry points (idh_conv_variant, idh_count_launches: nothing is dereferenced)."""
    return 0x10000 * (1 + zlib.crc32(name.encode()) % 4096)


def op_array(nhwc, ops):
    arr = (nhwc.Op * len(ops))(*ops)
    return arr, C.cast(arr, C.c_void_p)


def variant_of(L, nhwc, op):
    out = (C.c_int32 * 8)(*([-7] * 8))
    arr, p = op_array(nhwc, [op])
    rc = L.idh_conv_variant(p, out)
    return rc, tuple(out)


# ------------------------------------------------------------------------------------------------------------------
# tensors (logical values on the CPU; device buffers when a device is given)
# ------------------------------------------------------------------------------------------------------------------
def _padded(x_nhwc, cs, fill):
    buf = torch.full(x_nhwc.shape[:3] + (cs,), fill, dtype=torch.float32)
    buf[..., : x_nhwc.shape[3]] = x_nhwc
    return buf


def logical_tensors(spec):
    """Seeded CPU fp32 values of a case: NHWC activations, OIHW weights scaled so that outputs are O(1)."""
    g = torch.Generator().manual_seed(zlib.crc32(spec.name.encode()))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    t = {}
    if spec.kind == "up":
        t["x0"] = rn(spec.N, spec.H, spec.W, spec.C)
        return t
    for i, s in enumerate(spec.srcs):
        H, W = spec.in_hw(s)
        if s.up:
            c0, uC, ucs = s.up
            if c0:
                t[f"x{i}"] = rn(spec.N, H, W, c0)
            for j in range(len(ucs)):
                t[f"up{i}_{j}"] = rn(spec.N, H // 2, W // 2, uC)
        else:
            t[f"x{i}"] = rn(spec.N, H, W, s.cin) * (2.0 if s.norm else 1.0) + (0.5 if s.norm else 0.0)
        t[f"w{i}"] = rn(spec.cout, s.cin, s.ks, s.ks) / spec.K ** 0.5
    if spec.bias:
        t["bias"] = rn(spec.cout)
    if spec.res:
        t["res"] = rn(spec.N, spec.Ho, spec.Wo, spec.cout)
    return t


class Case:
    pass


def _pack_special(spec, t, device):
    """Source-0 weights of a Winograd / split-precision case, packed by the library's own pack entry point for that kernel."""
    from implicit_depth_amd import _lib

    L, co, ci = _lib.lib(), spec.cout, spec.srcs[0].cin
    w = t["w0"].to(device).contiguous()
    if spec.family == "split":  # the 1x1 weights of the second source ride in the same blob
        ci1 = spec.srcs[1].cin if len(spec.srcs) > 1 else 0
        w1 = t["w1"].reshape(co, ci1).to(device).contiguous() if ci1 else None
        n = L.idh_packed_split_weight_bytes(co, ci, ci1, TILE_SPLIT)
        assert n > 0 and n % 4 == 0
        dst = torch.empty(n // 4, dtype=torch.int32, device=device)
        rc = L.idh_pack_conv_weight_split(w.data_ptr(), w1.data_ptr() if ci1 else None, dst.data_ptr(), co, ci, ci1, TILE_SPLIT, _lib.stream_ptr())
    elif spec.family == "wino":
        dst = torch.empty(L.idh_packed_wino_weight_floats(co, ci), dtype=torch.float32, device=device)
        rc = L.idh_pack_conv_weight_wino(w.data_ptr(), dst.data_ptr(), co, ci, _lib.stream_ptr())
    else:
        dst = torch.empty(L.idh_packed_wino4_weight_floats(co, ci), dtype=torch.float32, device=device)
        rc = L.idh_pack_conv_weight_wino4(w.data_ptr(), dst.data_ptr(), co, ci, _lib.stream_ptr())
    _lib.check(rc, f"packing the weights of {spec.name}")
    torch.cuda.synchronize()  # (w / w1 are temporaries)
    return dst


def make_conv_case(spec, device, group=0):
    """Device buffers + one nhwc.Op for a spec (conv or upsample).  For a normalise-on-load source the IDH_OP_INSTNORM statistics
    pass runs here, and its (N, 2, C) mean / rstd result is read back into ``case.t`` for the reference."""
    from implicit_depth_amd import _lib, nhwc

    c = Case()
    c.spec, c.t, c.dev = spec, logical_tensors(spec), {}
    t, dev = c.t, c.dev
    nan = float("nan")
    if spec.kind == "up":
        dev["x0"] = _padded(t["x0"], spec.C + 4, nan).to(device)
        c.out_shape, c.cout = (spec.N, 2 * spec.H, 2 * spec.W, spec.C + 8), spec.C
    else:
        lay = buffer_layout(spec)
        for i, s in enumerate(spec.srcs):
            H, W = spec.in_hw(s)
            cs = lay["in_cs"][i]
            if s.up:
                c0, uC, ucs = s.up
                x = t[f"x{i}"] if c0 else torch.empty(spec.N, H, W, 0)
                dev[f"x{i}"] = _padded(x, cs, nan).to(device)  # up_c0 = 0: a buffer the kernel never reads
                for j, v in enumerate(ucs):
                    dev[f"up{i}_{j}"] = _padded(t[f"up{i}_{j}"], v, nan).to(device)
            else:
                dev[f"x{i}"] = _padded(t[f"x{i}"], cs, 0.0 if s.cin % 16 else nan).to(device)
            conv = torch.nn.Conv2d(s.cin, spec.cout, s.ks, bias=False)
            conv.weight.data = t[f"w{i}"].clone()
            if i == 0 and spec.family in ("wino", "wino4", "split"):
                dev["w0"] = _pack_special(spec, t, device)
            else:  # (a fused 1x1 of the Winograd kernels is packed as usual; the split kernel ignores src[1].w, which must still be non-NULL)
                dev[f"w{i}"] = nhwc.packed_weight(conv.to(device))
        if spec.bias:
            dev["bias"] = t["bias"].to(device)
        if spec.res:
            dev["res"] = _padded(t["res"], lay["res_cs"], nan).to(device)
        if spec.split_k > 1:  # as the header states: split_k x M x ceil16(Cout) floats
            dev["ws"] = torch.full((spec.split_k * spec.N * spec.Ho * spec.Wo * ceil16(spec.cout),), nan, dtype=torch.float32, device=device)
        c.out_shape, c.cout = (spec.N, spec.Ho, spec.Wo, lay["out_cs"]), spec.cout
        for i, s in enumerate(spec.srcs):
            if not s.norm:
                continue
            H, W = spec.in_hw(s)
            nchunks = -(-(H * W) // 1024)
            ws = torch.zeros(spec.N * (nchunks + 1) * 2 * s.cin, dtype=torch.float32, device=device)
            st = nhwc.Op()
            st.kind, st.N = nhwc.OP_INSTNORM, spec.N
            st.src[0].in_, st.src[0].cs, st.src[0].H, st.src[0].W, st.src[0].Cin = dev[f"x{i}"].data_ptr(), lay["in_cs"][i], H, W, s.cin
            st.ws = ws.data_ptr()
            arr, p = op_array(nhwc, [st])
            _lib.check(_lib.lib().idh_run_ops(p, 1, _lib.stream_ptr()), "IDH_OP_INSTNORM")
            torch.cuda.synchronize()
            dev[f"norm_ws{i}"] = ws
            dev[f"norm{i}"] = ws[spec.N * nchunks * 2 * s.cin:]
            t[f"norm{i}"] = dev[f"norm{i}"].cpu().view(spec.N, 2, s.cin)
    dev["out"] = torch.empty(c.out_shape, dtype=torch.int32, device=device)
    prefill(c)
    ptr = lambda name: dev[name].data_ptr()
    c.op = build_up_op(nhwc, spec, ptr, group) if spec.kind == "up" else build_op(nhwc, spec, ptr, group)
    return c


def prefill(case):
    case.dev["out"].fill_(PREFILL)
    if "ws" in case.dev:
        case.dev["ws"].fill_(float("nan"))


def read_output(case):
    """(the written slice as fp32 NHWC on the CPU, True when every element outside the slice still holds the prefill pattern)."""
    raw = case.dev["out"].cpu()
    inside = raw[..., OUT_C0: OUT_C0 + case.cout].contiguous().view(torch.float32)
    outside = torch.cat([raw[..., :OUT_C0], raw[..., OUT_C0 + case.cout:]], -1)
    return inside, bool((outside == PREFILL).all())


# ------------------------------------------------------------------------------------------------------------------
# fp64 reference and tolerance
# ------------------------------------------------------------------------------------------------------------------
def _act64(x, act, slope=SLOPE):
    if act == ACT_LRELU:
        return F.leaky_relu(x, slope)
    if act == ACT_ELU:
        return F.elu(x)
    return x


def source_input64(spec, i, t):
    """Logical (N, C, H, W) fp64 input of source i: the virtual concat with upsampled segments / the normalised tensor."""
    s = spec.srcs[i]
    nchw = lambda a: a.double().permute(0, 3, 1, 2)
    if s.up:
        parts = [nchw(t[f"x{i}"])] if s.up[0] else []
        for j in range(len(s.up[2])):
            parts.append(F.interpolate(nchw(t[f"up{i}_{j}"]), scale_factor=2, mode="bilinear", align_corners=False))
        return torch.cat(parts, 1)
    x = nchw(t[f"x{i}"])
    if s.norm:
        st = t[f"norm{i}"].double()  # (N, 2, C): means, then 1 / sqrt(var + eps), as the statistics kernel left them
        x = F.leaky_relu((x - st[:, 0, :, None, None]) * st[:, 1, :, None, None], SLOPE)
    return x


# The transforms of Y = A^T [ (G g G^T) .* (B^T d B) ] A as the kernels apply them.  F(2x2, 3x3): csrc/conv_wino.hip - B^T from the register transform of
# `compute` (d0 - d2, d1 + d2, d2 - d1, d1 - d3), G from pack_wino_weight_k, A^T from the epilogue ([1 1 1 0; 0 1 -1 -1]).  F(4x4, 3x3), interpolation
# points {0, +-1/2, +-2, inf}: csrc/conv_wino4.hip - B^T from bt3 / bt3_step, G from pack_wino4_weight_k, A^T from at6.
# test_conv_op_matrix_cpu.py::test_winograd_matrices_reproduce_the_convolution proves they are a 3x3 convolution.
WINO_MATRICES = {
    2: ([[1, 1, 1, 0], [0, 1, -1, -1]],
        [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]],
        [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]),
    4: ([[1, 1, 1, 1, 1, 0], [0, 0.5, -0.5, 2, -2, 0], [0, 0.25, 0.25, 4, 4, 0], [0, 0.125, -0.125, 8, -8, 1]],
        [[1, 0, 0], [-8 / 15, -4 / 15, -2 / 15], [-8 / 15, 4 / 15, -2 / 15], [1 / 30, 1 / 15, 2 / 15], [1 / 30, -1 / 15, 2 / 15], [0, 0, 1]],
        [[1, 0, -4.25, 0, 1, 0], [0, -2, -4, 0.5, 1, 0], [0, 2, -4, -0.5, 1, 0], [0, -0.5, -0.25, 2, 1, 0], [0, 0.5, -0.25, -2, 1, 0], [0, 1, 0, -4.25, 0, 1]]),
}


def wino_matrices(m, dtype=torch.float64):
    return tuple(torch.tensor(a, dtype=torch.float64).to(dtype) for a in WINO_MATRICES[m])


def wino_conv(x, w, m, dtype=torch.float64, magnitude=False, matrices=None):
    """Zero-padded 3x3 stride-1 convolution of x (N, C, H, W) with w (O, C, 3, 3) by the Winograd algorithm F(m x m, 3x3) on m x m output blocks
    anchored at the image origin (as the kernels tile), every transform, product and sum in ``dtype``.  magnitude = True: the same expression
    with every matrix and operand replaced by its absolute value - B_wino of ``tolerance``."""
    AT, G, BT = matrices if matrices is not None else wino_matrices(m, dtype)
    x, w = x.to(dtype), w.to(dtype)
    if magnitude:
        AT, G, BT, x, w = AT.abs(), G.abs(), BT.abs(), x.abs(), w.abs()
    N, Cc, H, W = x.shape
    ty, tx, t = -(-H // m), -(-W // m), m + 2
    x = F.pad(x, (1, tx * m + 1 - W, 1, ty * m + 1 - H))
    d = x.unfold(2, t, m).unfold(3, t, m)  # (N, C, ty, tx, t, t)
    V = torch.einsum("ai,ncyxij,bj->ncyxab", BT, d, BT)
    Uw = torch.einsum("ai,ocij,bj->ocab", G, w, G)
    M = torch.einsum("ocab,ncyxab->noyxab", Uw, V)
    Y = torch.einsum("ia,noyxab,jb->noyixj", AT, M, AT)
    return Y.reshape(N, w.shape[0], ty * m, tx * m)[:, :, :H, :W]


def reference(spec, t):
    """fp64 result of the op (NHWC), its pre-activation, and the magnitude B = conv(|x|, |w|) + |bias| + |res| - for the Winograd kernels with
    B_wino = |A^T| [ (|G| |w| |G^T|) .* (|B^T| |x| |B|) ] |A| (summed over the input channels) in place of source 0's conv(|x|, |w|)."""
    if spec.kind == "up":
        x = t["x0"].double().permute(0, 3, 1, 2)
        up = lambda a: F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous()
        return up(x), up(x), up(x.abs())
    pre, B = 0.0, 0.0
    for i, s in enumerate(spec.srcs):
        x, w, p = source_input64(spec, i, t), t[f"w{i}"].double(), s.ks // 2
        if p:
            x = F.pad(x, (p, p, p, p), mode="replicate") if spec.pad == PAD_REPLICATE else F.pad(x, (p, p, p, p))
        pre = pre + F.conv2d(x, w, stride=s.stride)
        if i == 0 and spec.family in ("wino", "wino4"):
            B = B + wino_conv(source_input64(spec, 0, t), w, 2 if spec.family == "wino" else 4, magnitude=True)
        else:
            B = B + F.conv2d(x.abs(), w.abs(), stride=s.stride)
    pre, B = pre.permute(0, 2, 3, 1), B.permute(0, 2, 3, 1)
    assert tuple(pre.shape) == (spec.N, spec.Ho, spec.Wo, spec.cout), (spec.name, pre.shape)
    if spec.bias:
        pre, B = pre + t["bias"].double(), B + t["bias"].double().abs()
    if spec.res:
        pre, B = pre + t["res"].double(), B + t["res"].double().abs()
    return _act64(pre, spec.act, spec.slope).contiguous(), pre.contiguous(), B.contiguous()


SPLIT_PRODUCT_ERR = 2.0 ** -21  # (1 + 2^-22)^2 - 1, rounded up: two operands each represented to 2^-22 (tests/test_split_arithmetic_cpu.py)


def wino_steps(spec):
    """Roundings on the longest path from the operands to one output of F(m x m, 3x3), m + 2 = t points: the two passes of the input transform
    (t terms each), of the filter transform (3 terms each; the pack kernels work in fp64 and round once, which is fewer) and of the output transform
    (t terms each), one product and one accumulation per input channel of either source, + bias, residual and the final roundings (4, as for
    the direct kernels)."""
    t = 4 if spec.family == "wino" else 6
    return 4 * t + 6 + sum(s.cin for s in spec.srcs) + 4


def tolerance(spec, ref, B, t=None):
    """Elementwise bound, derived: fp32 accumulation of K products (+ S partials, + bias, residual and the final roundings) in any
    order errs by at most (K + S + 4) u B before the activation; twice that is allowed (the rounding mode inside the matrix unit is
    unspecified).  NONE / LRELU / ELU are 1-Lipschitz: the bound carries over, plus u |ref| for the result's own rounding, plus - for
    ELU - 4 x the measured fp32 error of the host's elu.  Blended / normalised inputs: 8 u B for their own roundings.

    Winograd F(2x2) / F(4x4) (tile_m 12 / 13): the kernels do not form the K products of B = conv(|x|, |w|) but sums and differences of
    transformed operands, whose intermediate magnitudes are larger (up to ~300 x for the corner outputs of F(4x4), whose A^T row holds +-8).
    Every rounding on the way is relative to a partial sum of B_wino = |A^T| [ (|G| |w| |G^T|) .* (|B^T| |x| |B|) ] |A| (``reference`` returns it
    as B for these cases, + the fused 1x1's conv(|x1|, |w1|) + |bias| + |res|), and there are at most ``wino_steps`` of them on a path: the bound
    is 2 x wino_steps x u x B_wino, with the same factor 2, u |ref| and ELU term as above.  test_conv_op_matrix_cpu.py checks that the matrices
    are the kernels' (they reproduce conv2d in fp64), that an all-fp32 evaluation stays inside, and that a wrong tap / coefficient does not.

    Split precision (tile_m 11): each fp32 operand is replaced by two f16 pieces that represent it to 2^-22 of its value
    (tests/test_split_arithmetic_cpu.py asserts that figure; elements more than 2^17 below their scale group's maximum keep 2^-22 of that
    maximum instead, covered here by a term in max|x| max|w|) and the piece products are exact in fp32, so every product carries a relative
    error of at most (1 + 2^-22)^2 - 1 < 2^-21 before the fp32 accumulation the first paragraph bounds (the dropped x1 w1 term is 2^-44): the
    bound is that of the direct kernels + 2^-21 B + 2^-21 2^-17 K max|x| max|w| (``t``: the case's tensors, needed for this family only).

    The GPU test prints the worst err / bound of every case; for comparison, the all-fp32 CPU evaluation of the Winograd cases peaks at 0.004
    (F(2x2) and F(4x4) alike): the bound follows worst-case magnitudes, the roundings average out."""
    if spec.kind == "up":
        return 8 * U * B + U * ref.abs()
    if spec.family in ("wino", "wino4"):
        tol = 2 * wino_steps(spec) * U * B + U * ref.abs()
    else:
        tol = 2 * (spec.K + spec.S + 4) * U * B + U * ref.abs()
    if spec.family == "split":
        floor = sum(s.ks * s.ks * s.cin * t[f"x{i}"].abs().max().item() * t[f"w{i}"].abs().max().item() for i, s in enumerate(spec.srcs))
        tol = tol + SPLIT_PRODUCT_ERR * B + SPLIT_PRODUCT_ERR * 2.0 ** -17 * floor
    if any(s.up or s.norm for s in spec.srcs):
        tol = tol + 8 * U * B
    if spec.act == ACT_ELU:
        tol = tol + 4 * ELU_F32_ERR
    return tol
