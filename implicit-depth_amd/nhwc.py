"""Host-side execution plans for the conv stage of the hot path.

A *plan* is a flat array of ``idh_op`` descriptors (include/idh_ops.h) plus the NHWC
activation buffers they point into, built once per (module, input shape, device) and replayed
with a single C-ABI call (``idh_run_ops``).  torch only owns the memory and the stream.

What the plans encode (reference modules/networks.py + modules/layers.py):
  BasicBlock   -> conv1(+LeakyReLU)  then ONE launch for conv2 + residual: the 1x1 / strided-3x3
                  projection of the block input is a second K-source of that launch, the identity
                  residual is added in the epilogue
  torch.cat    -> producers write into channel slices of the consumer's input buffer
  upsample     -> bilinear x2 kernel writing straight into that slice
  heads        -> only the ``output_i`` results that survive in the reference's dict are
                  computed (the reference evaluates and discards the others, networks.py:80)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _lib

# --- ctypes mirrors of include/idh_ops.h -------------------------------------------------
OP_CONV, OP_UPSAMPLE2, OP_IMPORT, OP_EXPORT, OP_SPLITK, OP_HEAD, OP_INSTNORM, OP_UPSAMPLE2_NEAREST, OP_COPY, OP_POINTWISE_NCHW, OP_POINTWISE_UP = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
OP_STEM = 12
ACT_NONE, ACT_LRELU, ACT_ELU = 0, 1, 2
PAD_ZEROS, PAD_REPLICATE = 0, 1


class ConvSrc(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("w", C.c_void_p), ("cs", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("Cin", C.c_int32), ("ks", C.c_int32), ("stride", C.c_int32), ("pad_mode", C.c_int32), ("_r", C.c_int32),
                ("up_in", C.c_void_p * 2), ("up_cs", C.c_int32 * 2), ("up_c0", C.c_int32), ("up_C", C.c_int32),
                ("norm", C.c_void_p), ("norm_slope", C.c_float), ("norm_act", C.c_int32)]


class Op(C.Structure):
    _fields_ = [("kind", C.c_int32), ("N", C.c_int32), ("src", ConvSrc * 2), ("bias", C.c_void_p), ("res", C.c_void_p),
                ("out", C.c_void_p), ("ws", C.c_void_p), ("res_cs", C.c_int32), ("out_cs", C.c_int32), ("Ho", C.c_int32),
                ("Wo", C.c_int32), ("Cout", C.c_int32), ("act", C.c_int32), ("slope", C.c_float), ("split_k", C.c_int32),
                ("tile_m", C.c_int32), ("tile_n", C.c_int32), ("group", C.c_int32)]


def _bind():
    return _lib.lib()


# --- NHWC views ---------------------------------------------------------------------------
@dataclass
class View:
    """Channel slice [c0, c0+C) of a dense NHWC buffer (N,H,W,CS)."""

    buf: torch.Tensor
    c0: int
    C: int

    @property
    def N(self):
        return self.buf.shape[0]

    @property
    def H(self):
        return self.buf.shape[1]

    @property
    def W(self):
        return self.buf.shape[2]

    @property
    def cs(self):
        return self.buf.shape[3]

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.c0

    def slice(self, c0, C):
        return View(self.buf, self.c0 + c0, C)

    def dense(self) -> torch.Tensor:
        return self.buf[..., self.c0 : self.c0 + self.C]


@dataclass
class CatView:
    """``torch.cat([direct, upsample(ups[0]), upsample(ups[1])], 1)`` that is never materialised: the consumer conv
    reads ``direct`` as it is and interpolates the x2 bilinear upsampling of the low-resolution ``ups`` maps while it
    stages its halo (idh_conv_src.up_*; reference networks.py:64-76 + generic_utils.py:94-103)."""

    direct: View
    ups: List[View]

    @property
    def N(self):
        return self.direct.N

    @property
    def H(self):
        return self.direct.H

    @property
    def W(self):
        return self.direct.W

    @property
    def C(self):
        return self.direct.C + sum(u.C for u in self.ups)


def ceil16(v: int) -> int:
    return (v + 15) & ~15


def _region(v: "View", pad16: bool = False):
    """(buffer id, first channel, one-past-last channel) touched through view ``v``."""
    return (v.buf.data_ptr(), v.c0, v.c0 + (ceil16(v.C) if pad16 else v.C))


def packed_weight(conv: nn.Conv2d) -> torch.Tensor:
    """[tap][ci/4][co][ci%4] copy of a Conv2d weight, cached on the module and refreshed when
    the parameter is modified in place or moved."""
    w = conv.weight
    key = (w.data_ptr(), _lib.param_version(w), str(w.device))
    cached = getattr(conv, "_idh_packed", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    _lib.require_cuda_f32(w)
    L = _bind()
    co, ci, kh, kw = w.shape
    if kh != kw or kh not in (1, 3):
        raise _lib.IdhError(f"conv kernel {kh}x{kw} not covered by the gfx950 conv kernel (1x1 / 3x3 only)")
    n = L.idh_packed_weight_floats(co, ci, kh)
    dst = torch.empty(n, device=w.device, dtype=torch.float32)
    wc = w.detach().contiguous()
    _lib.check(L.idh_pack_conv_weight(wc.data_ptr(), dst.data_ptr(), co, ci, kh, _lib.stream_ptr()), "idh_pack_conv_weight")
    conv._idh_packed = (key, dst)
    return dst


def packed_wino_weight(conv: nn.Conv2d) -> torch.Tensor:
    """Winograd-domain copy U = G g G^T of a 3x3 Conv2d weight in the MFMA A-fragment order of csrc/conv_wino.hip
    (idh_pack_conv_weight_wino); cached like ``packed_weight``."""
    w = conv.weight
    key = (w.data_ptr(), _lib.param_version(w), str(w.device))
    cached = getattr(conv, "_idh_packed_wino", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    _lib.require_cuda_f32(w)
    L = _bind()
    co, ci, kh, kw = w.shape
    if (kh, kw) != (3, 3):
        raise _lib.IdhError("the Winograd F(2x2,3x3) kernel covers 3x3 convolutions only")
    dst = torch.empty(L.idh_packed_wino_weight_floats(co, ci), device=w.device, dtype=torch.float32)
    wc = w.detach().contiguous()
    _lib.check(L.idh_pack_conv_weight_wino(wc.data_ptr(), dst.data_ptr(), co, ci, _lib.stream_ptr()), "idh_pack_conv_weight_wino")
    conv._idh_packed_wino = (key, dst)
    return dst


def packed_wino4_weight(conv: nn.Conv2d) -> torch.Tensor:
    """Winograd F(4x4,3x3)-domain copy of a 3x3 Conv2d weight in the A-fragment order of csrc/conv_wino4.hip
    (idh_pack_conv_weight_wino4); cached like ``packed_weight``."""
    w = conv.weight
    key = (w.data_ptr(), _lib.param_version(w), str(w.device))
    cached = getattr(conv, "_idh_packed_wino4", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    _lib.require_cuda_f32(w)
    L = _bind()
    co, ci, kh, kw = w.shape
    if (kh, kw) != (3, 3):
        raise _lib.IdhError("the Winograd F(4x4,3x3) kernel covers 3x3 convolutions only")
    dst = torch.empty(L.idh_packed_wino4_weight_floats(co, ci), device=w.device, dtype=torch.float32)
    wc = w.detach().contiguous()
    _lib.check(L.idh_pack_conv_weight_wino4(wc.data_ptr(), dst.data_ptr(), co, ci, _lib.stream_ptr()), "idh_pack_conv_weight_wino4")
    conv._idh_packed_wino4 = (key, dst)
    return dst


TILE_WINO = 12  # IDH_TILE_WINO of include/idh_ops.h == the op's tile_m
TILE_WINO4 = 13  # IDH_TILE_WINO4
# Winograd F(2x2,3x3) for the eligible 3x3 stride-1 layers of fp32 plans (csrc/conv_wino.hip): fp32 operands and
# accumulation, 2.25x fewer MFMAs; measured 1.67-1.84x over the direct LDS kernel at B=32 (tools/perf_wino.py).
# Tiles are 32 x 8 pixels x 32 channels; WINO_MIN_TILES: below this many tiles the direct kernels' finer tiles fill the
# chip better (conv stage of the hot path with thresholds off / 512 / 256 / 128 / 64, tools/perf_levels.py: B=1 2.67 / 2.66 /
# 2.46 / 2.45 / 2.66 ms, B=2 4.43 / 3.90 / 3.91 / 3.80 / 3.89, B=4 7.75 / 6.64 / 6.36 / 6.26 / 6.47); WINO_MIN_FILL: smallest useful fraction of the tile grid that lies inside the map.
WINOGRAD = True
WINO_MIN_TILES = 128
WINO_MIN_FILL = 0.74
# the Winograd convs of one dependency level as ONE persistent grid (conv3x3_wino_group_k): bit-identical, fewer launch tails
WINO_GROUP = True


def wino_eligible(srcs, cout: int, N: int, Ho: int, Wo: int, pad_mode: int) -> bool:
    return bool(select(srcs, cout, N, Ho, Wo, pad_mode).families & FAMILY_WINO)


# Winograd F(4x4,3x3) (csrc/conv_wino4.hip, conv3x3_wino4_k) for the plain 3x3 layers: 1.78x fewer MFMAs than F(2x2); 32 x 8 pixel x 64
# channel tiles on two persistent workgroups per CU (512 slots).  Measured against F(2x2) (tools/perf_wino4.py, profiles/r04/perf_wino4_final.txt):
# 1.11-1.39x at B = 32 on every eligible layer of the network.  Layer by layer it wins or ties down to ~192 tiles and loses below
# (96 tiles: 0.6-0.8x), but inside a whole step the threshold that never loses is 384 (bench.py --batch 1 / 4 / 8 / 16 with 192:
# -5 / -4 / 0 / +1 %; with 384: 0 / +2 / +6 / +7 %; profiles/r04/experiments.md): below it the F(2x2) convs of a UNet++ level share ONE
# grouped launch, which a half-filled grid of F(4x4) tiles does not beat.  A fused 1x1 projection rides in the same kernel (conv3x3_wino4_k<true>:
# 1.07-1.25x over F(2x2)'s); layers with a normalised source stay where they were.
# activation-buffer liveness reuse (Plan.release): BasicBlock intermediates of >= REUSE_MIN_BYTES are recycled by later blocks of the same shape
BUFFER_REUSE = True
REUSE_MIN_BYTES = 64 << 20
WINOGRAD4 = True
WINOGRAD4_PROJ = True  # ... also for the blocks with a fused 1x1 projection (conv3x3_wino4_k<true>)
WINO4_MIN_TILES = 768  # (re-swept late in round 5, tools/perf_levels.py: 384 / 768 -> conv plan 8.73 / 8.64 ms at B = 8, 12.88 / 12.67 at B = 12, equal at 4, 16, 24, 32: a
# level of exactly 384 tile groups - 0.75 of a round of the 512 resident workgroups - runs no faster than the grouped F(2x2) launch of the level)
WINO4_MIN_FILL = 0.85


def wino4_eligible(srcs, cout: int, N: int, Ho: int, Wo: int, pad_mode: int, act: int, out=None, res=None, slope: float = 0.2, any_size: bool = False) -> bool:
    """``idh_conv::wino4_supported`` (csrc/conv_wino4.hip) plus the fill / tile-count rules.  ``out`` / ``res``: the views the op writes / adds -
    their per-image byte sizes are 32-bit buffer ranges in the kernel, so a layer that exceeds them is planned onto F(2x2) / the direct kernels."""
    return bool(select(srcs, cout, N, Ho, Wo, pad_mode, act, slope, out, res, any_size=any_size).families & FAMILY_WINO4)


SPLIT_CODE = {"f16x3": 11}  # IDH_SPLIT_F16X3 of include/idh_ops.h == the op's tile_m


def split_packed_weight(conv: nn.Conv2d, math: str, proj: Optional[nn.Conv2d] = None) -> torch.Tensor:
    """16-bit-piece copy of a 3x3 Conv2d weight (and, fused behind it, of the 1x1 projection that shares
    its accumulator) in the LDS image order of csrc/conv_split.hip (idh_pack_conv_weight_split);
    cached like ``packed_weight``."""
    w = conv.weight
    w1 = proj.weight if proj is not None else None
    key = (w.data_ptr(), _lib.param_version(w), str(w.device), math) + ((w1.data_ptr(), _lib.param_version(w1)) if w1 is not None else ())
    cached = getattr(conv, "_idh_packed_split", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    _lib.require_cuda_f32(w)
    L = _bind()
    co, ci, kh, kw = w.shape
    ci1 = 0
    w1c = None
    if w1 is not None:
        _lib.require_cuda_f32(w1)
        if tuple(w1.shape[2:]) != (1, 1) or w1.shape[0] != co:
            raise _lib.IdhError("the fused second source of a split-precision conv must be a 1x1 conv with the same Cout")
        ci1 = w1.shape[1]
        w1c = w1.detach().reshape(co, ci1).contiguous()
    n = L.idh_packed_split_weight_bytes(co, ci, ci1, SPLIT_CODE[math])
    if kh != 3 or kw != 3 or n == 0:
        raise _lib.IdhError("split-precision conv covers 3x3 kernels with Cout % 64 == 0")
    dst = torch.empty(n // 4, device=w.device, dtype=torch.int32)
    wc = w.detach().contiguous()
    _lib.check(L.idh_pack_conv_weight_split(wc.data_ptr(), _lib.ptr(w1c), dst.data_ptr(), co, ci, ci1, SPLIT_CODE[math], _lib.stream_ptr()),
               "idh_pack_conv_weight_split")
    conv._idh_packed_split = (key, dst)
    return dst


# Arithmetic of the 3x3 stride-1 convs: "fp32" = v_mfma_f32_16x16x4_f32 everywhere (default);
# "f16x3" (opt-in) = the layers of the split_eligible() family run on the f16 matrix cores with every fp32 operand
# expanded into 2 scaled f16 pieces and the 3 significant cross products accumulated in fp32
# (csrc/conv_split.hip) — fp32-equivalent results at 3/16 of the fp32-MFMA cost.
MATH_MODES = ("fp32", "f16x3")
DEFAULT_MATH = "fp32"  # process-wide default; per-plan: Plan(math=...) / the module's ``conv_math`` attribute
SPLIT_MIN_BLOCKS = 256  # fewer 8x16x64 tiles than CUs: the fp32 kernels' finer tiles win


def split_eligible(srcs, cout: int, N: int, Ho: int, Wo: int, pad_mode: int) -> bool:
    return bool(select(srcs, cout, N, Ho, Wo, pad_mode).families & FAMILY_SPLIT)


def choose_split_rows(N: int, Ho: int, Wo: int, cout: int) -> int:
    """16-row tiles (best weight-panel amortisation) when they fill 256 CUs x 3 resident workgroups
    without wasting rows, else 8-row tiles (twice the workgroups, no waste on 24-row maps)."""
    return select([(None, _conv_shape(16, 3))], cout, N, Ho, Wo).split_rows


# Decoder concats: optionally fold the x2 upsampling (and the concat itself) into the consumer conv's halo loader
# instead of running upsample2_k into a concat buffer.  Bit-identical, 16 launches and ~1 GB of HBM traffic less per
# 32-frame step — and SLOWER on MI355X (tools/perf_up.py, profiles/r02/fused_upsample_experiment.txt: 82.2 ms
# materialised vs 91.0 ms fused with 8-row tiles / 85.8 ms with 4-row tiles at B=32; 4.10 vs 4.16 ms at B=1): the 4x
# register prefetch of the loader either spills (8-row tile) or costs the tile's operand reuse (4-row), which outweighs
# the 2.6 ms upsample2_k takes at HBM speed.  Off by default; FUSED_UP_ROWS = tile rows of the convs that read such a
# concat.
FUSE_UPSAMPLE = False
FUSED_UP_ROWS = 4

# One launch per dependency level where its members are small (one frame, low-resolution maps): idh_run_ops merges the
# consecutive ops of a level that carry its group id into one ``level_k`` grid when each has <= 512 workgroups.
MERGE_LEVELS = True
# Matching-encoder head: InstanceNorm2d(128) + LeakyReLU applied by the following 3x3 conv while it stages its halo
# (idh_conv_src.norm) instead of a normalised copy of the tensor; False = materialise (bit-identical, tests compare).
FUSE_HEAD_NORM = True
# ... and its first 1x1 conv reading the backbone's NCHW map in place (IDH_OP_POINTWISE_NCHW) instead of after a
# layout-import pass; False = import_nchw + the generic conv (bit-identical).
FUSE_HEAD_IMPORT = True

TARGET_WAVES = 2048  # ~2 waves per SIMD over 256 CUs x 4 SIMDs
MIN_WAVES = 1024


def lds_eligible(srcs, cout: int, Wo: int, pad_mode: int) -> bool:
    """Shape family of the LDS-staged kernel (csrc/conv.hip conv3x3_lds_k)."""
    return bool(select(srcs, cout, 1, 1, Wo, pad_mode).families & FAMILY_LDS)


# A lone 3x3 stride-2 conv (conv1 of a stride-2 BasicBlock, layers.py:62-66) on the LDS-staged kernel's stride-2 loader (the one the strided
# projections use: halo de-interleaved by column parity, every tap's fragment read conflict-free) instead of the direct-fragment kernel, which
# re-reads each input pixel 9 times through L1 (46-55 % MFMA-busy).  Below S2_FIRST_MIN_BLOCKS 4-row workgroups the direct kernel stays: at
# one or two frames it is a member of the level launch (level_k).
S2_FIRST = True
S2_FIRST_MIN_BLOCKS = 512


def s2_first_eligible(srcs, cout: int, N: int, Ho: int, Wo: int, pad_mode: int) -> bool:
    return bool(select(srcs, cout, N, Ho, Wo, pad_mode).families & FAMILY_S2_FIRST)


def lds_subtiles(cout: int) -> int:
    """16-channel output sub-tiles per workgroup of the LDS-staged kernel (the op's tile_n): 64 channels when the
    layer has them, else 32 / 16 (the matching encoder's 128 -> 16 conv)."""
    return select([(None, _conv_shape(16, 3))], cout, 1, 1, 1).lds_subtiles


# Small grids (one frame, low-resolution levels): halve the workgroup's channel tile (64 -> 32) when even 4-row tiles
# leave fewer than this many workgroups, to shorten each workgroup's MFMA phase and spread it over more CUs.
# Measured (tools/perf_levels.py <B> <threshold>, conv stage of the hot path): B=1 3.31 -> 3.04 ms, B=2 5.06 -> 4.88 ms,
# B=4 and B=8 unchanged with 400; 800 / 1600 cost 1-1.5 % at B=4.
NARROW_TILE_BELOW = 400
NARROWEST_TILE_BELOW = 0  # below this many 64-channel workgroups use 16-channel tiles (0 = never)


SPLIT_MIN_CHUNKS = 6
SPLIT_MAX = 16
# decoder in_conv blocks: projection of the upsampled concat slices at low resolution (Plan.basic_block_upcat, pointwise_up_k).  Built, parity-tested,
# and OFF: at B = 32 the conv plan takes 28.80 against 28.53 ms with it.  Per 192x256 block the F(4x4) projection phase it removes costs 338 us
# (783 -> 445 us for conv2: that phase already runs at ~80 % of the matrix rate), pointwise_up_k + the low-resolution 1x1 conv that replace it
# 270 + 68 us, both HBM-bound (profiles/r05/experiments.md 3b).
PROJ_LOWRES = False
PROJ_LOWRES_MIN_TILES = 1536
PROJ_CHUNK_WEIGHT = 0.5  # a 1x1 (projection) chunk in units of a 3x3 chunk when the split-K factor is chosen (1.0 / 0.5 / 0.25 measured: B=1 2.353 / 2.330 / 2.343 ms, B=4 5.135 / 5.099 / 5.110)


def choose_lds_tile(N: int, Ho: int, Wo: int, cout: int, chunks: int):
    """(tile code, split): 8-row tiles (code 8) when they already give one full round of
    256 CUs x 3 resident workgroups, else 4-row tiles (code 9); split K only when the grid still
    cannot fill the chip AND every split keeps >= 6 chunks of 16 channels (measured on MI355X,
    tools/perf_conv_layers.py)."""
    ch = select([(None, _conv_shape(16 * chunks, 3))], cout, N, Ho, Wo)
    return ch.lds_tile_m, ch.lds_split_k


def choose_tiles(M: int, cout: int, steps: int):
    ch = select([(None, _conv_shape(16 * steps, 1))], cout, 1, 1, M)
    return ch.direct_tile_m, ch.direct_tile_n, ch.direct_split_k


# --- the one kernel-selection rule: idh_conv_select (csrc/plan_select.hip), which the C++ plan builder calls too --------------------
W_DIRECT, W_WINO, W_WINO4, W_SPLIT = 0, 1, 2, 3  # IDH_W_* of include/idh_ops.h
FAMILY_WINO, FAMILY_WINO4, FAMILY_SPLIT, FAMILY_LDS, FAMILY_S2_FIRST = 1, 2, 4, 8, 16  # IDH_FAMILY_*
SCHED_MERGE_LEVELS, SCHED_WINO_GROUP = 1, 2  # IDH_SCHED_*


def _conv_shape(cin: int, ks: int, stride: int = 1):
    """What ``select`` reads of an nn.Conv2d, for the choosers that are asked about a bare shape."""
    import types

    return types.SimpleNamespace(in_channels=cin, kernel_size=(ks, ks), stride=(stride, stride))


def conv_tuning() -> "_lib.ConvTuning":
    """``idh_conv_tuning`` from the module globals as they are NOW (tests and tools assign them and expect the next plan to see them)."""
    return _lib.ConvTuning(WINOGRAD, WINOGRAD4, WINOGRAD4_PROJ, S2_FIRST, WINO_MIN_TILES, WINO4_MIN_TILES, SPLIT_MIN_BLOCKS, NARROW_TILE_BELOW,
                           NARROWEST_TILE_BELOW, SPLIT_MIN_CHUNKS, SPLIT_MAX, S2_FIRST_MIN_BLOCKS, FUSED_UP_ROWS, TARGET_WAVES, MIN_WAVES, 0,
                           WINO_MIN_FILL, WINO4_MIN_FILL, PROJ_CHUNK_WEIGHT)


def select(srcs, cout: int, N: int, Ho: int, Wo: int, pad_mode: int = PAD_ZEROS, act: int = ACT_NONE, slope: float = 0.2, out=None, res=None,
           norm: bool = False, any_size: bool = False, math: str = "fp32") -> "_lib.ConvChoice":
    """``idh_conv_select`` for a conv of ``srcs`` = [(view, nn.Conv2d), ...] under the current tuning.  Of a view only H, W, cs are read and of a
    conv only in_channels, kernel_size, stride - 0 where a shape-only stand-in has none."""
    d = _lib.ConvDesc(N, Ho, Wo, cout, pad_mode, act, slope, getattr(out, "cs", 0), getattr(res, "cs", 0), res is not None, norm, any_size,
                      SPLIT_CODE.get(math, 0), len(srcs))
    for s, (v, cv) in zip(d.src, srcs):
        s.H, s.W, s.cs, s.is_cat = getattr(v, "H", 0), getattr(v, "W", 0), getattr(v, "cs", 0), isinstance(v, CatView)
        s.Cin, s.ks, s.stride = getattr(cv, "in_channels", 0), cv.kernel_size[0], cv.stride[0]
    ch = _lib.ConvChoice()
    _lib.check(_bind().idh_conv_select(C.byref(d), C.byref(conv_tuning()), C.byref(ch)), "idh_conv_select")
    return ch


class Plan:
    """Ordered op list + owned buffers.  ``run()`` = one C-ABI call."""

    def __init__(self, device, math: Optional[str] = None):
        self.device = device
        self.math = DEFAULT_MATH if math is None else math
        if self.math not in MATH_MODES:
            raise _lib.IdhError(f"unknown conv math mode {self.math!r} (expected one of {MATH_MODES})")
        self.ops: List[Op] = []
        self.meta: List[dict] = []  # per op: regions read / written, for the level scheduler
        self.keep: List[torch.Tensor] = []  # buffers / packed weights referenced by raw pointer
        self._free: Dict[tuple, List[torch.Tensor]] = {}  # released buffers by shape (``release``)
        self.recycled_candidates = 0  # buffers handed to the pool by ``release``
        self.recycled = 0  # ... and how many of them a later ``buffer()`` took over (tests assert that aliasing really happened)
        self._arr = None
        self._pos: Optional[List[int]] = None  # op index at build time -> index after schedule()
        self.flops = 0  # 2*MAC of the conv ops (algorithmic, no padding)

    # buffers -------------------------------------------------------------------------
    def buffer(self, N, H, W, Cch) -> View:
        """Dense NHWC buffer.  The conv kernel reads whole 16-channel blocks, so channel counts
        that are not a multiple of 16 get zero-filled padding channels (written by nobody)."""
        cs = ceil16(Cch)
        pool = self._free.get((N, H, W, cs)) if cs == Cch else None
        if pool:
            self.recycled += 1
            return View(pool.pop(), 0, Cch)
        alloc = torch.zeros if cs != Cch else torch.empty
        t = alloc(N, H, W, cs, device=self.device, dtype=torch.float32)
        self.keep.append(t)
        return View(t, 0, Cch)

    def release(self, v: View):
        """Liveness reuse of activation memory: the caller will record no further op that touches ``v`` (a whole buffer of this plan), so a
        later ``buffer()`` of the same shape may alias it.  Safe under the level scheduler by construction — the op regions are keyed by
        the tensor, so the new writer gets a write-after-read dependency on the last reader — but that dependency also serialises blocks
        that used to share a dependency level, which small grids need for their grouped launches: only buffers of at least
        ``REUSE_MIN_BYTES`` (ops that fill the chip on their own) are pooled."""
        t = v.buf
        if (BUFFER_REUSE and v.c0 == 0 and v.C == t.shape[-1] and t.dim() == 4 and t.numel() * 4 >= REUSE_MIN_BYTES
                and any(t is k for k in self.keep)):
            pool = self._free.setdefault(tuple(t.shape), [])
            if any(t is f for f in pool):  # a second release of a buffer that is still in the pool would hand it to TWO later allocations
                raise _lib.IdhError("Plan.release: buffer released twice")
            pool.append(t)
            self.recycled_candidates += 1

    # recording -----------------------------------------------------------------------
    def _record(self, op: Op, reads, writes) -> int:
        """The one way an op enters the plan: the descriptor, the (buffer id, c0, c1) regions ``idh_schedule_ops`` orders it by, and the
        cached ctypes array dropped.  Returns the build index (what ``set_in`` / ``set_out`` take, stable across ``schedule()``)."""
        self.ops.append(op)
        self.meta.append({"reads": reads, "writes": writes})
        self._arr = None
        return len(self.ops) - 1

    @staticmethod
    def _fill_src(s: ConvSrc, v: View):
        s.in_, s.cs, s.H, s.W, s.Cin = v.ptr, v.cs, v.H, v.W, v.C

    def _keep_bias(self, op: Op, bias: Optional[torch.Tensor]):
        """``op.bias`` = a contiguous copy of ``bias`` that lives as long as the plan (None: the op has no bias)."""
        if bias is not None:
            bias = bias.detach().contiguous()
            self.keep.append(bias)
            op.bias = bias.data_ptr()

    # ops -----------------------------------------------------------------------------
    def conv(self, x: View, conv: nn.Conv2d, out: View, act=ACT_NONE, slope=0.2, res: Optional[View] = None,
             x2: Optional[View] = None, conv2: Optional[nn.Conv2d] = None, pad_mode=PAD_ZEROS, norm=None, wino4_any_size: bool = False):
        """``norm`` = (stats, act, slope): read ``x`` through act((x - mean) * rstd) with the (N, 2, C) statistics of
        ``instance_norm(x, None)`` (``norm_on_load_eligible`` layers only).  ``wino4_any_size``: an fp32 layer of the F(4x4) shape family runs on
        conv3x3_wino4_k whatever its tile count (results then do not depend on the batch size)."""
        op = Op(kind=OP_CONV, N=x.N)
        srcs = [(x, conv)] + ([(x2, conv2)] if x2 is not None else [])
        for v, cv in srcs:
            if v.C != cv.in_channels:
                raise _lib.IdhError(f"conv expects {cv.in_channels} input channels, view has {v.C}")
        ch = select(srcs, conv.out_channels, out.N, out.H, out.W, pad_mode, act, slope, out, res, norm is not None, wino4_any_size, self.math)
        pack = (packed_weight, packed_wino_weight, packed_wino4_weight)
        for i, (v, cv) in enumerate(srcs):
            ks, st = cv.kernel_size[0], cv.stride[0]
            cat = v if isinstance(v, CatView) else None
            if cat is not None:
                if ch.w_layout == W_SPLIT or not ch.families & FAMILY_LDS or st != 1:
                    raise _lib.IdhError("a fused-upsample concat can only feed the LDS-staged fp32 conv kernel")
                if cat.direct.C % 16 or any(u.C != cat.ups[0].C or u.C % 16 or (2 * u.H, 2 * u.W) != (cat.H, cat.W) for u in cat.ups) or not 1 <= len(cat.ups) <= 2:
                    raise _lib.IdhError("fused-upsample concat: channel counts must be multiples of 16 and the maps exactly half size")
                v = cat.direct
            elif v.C % 16 and (v.c0 != 0 or v.cs != ceil16(v.C)):
                raise _lib.IdhError("a conv input whose channel count is not a multiple of 16 must be a whole zero-padded buffer")
            if ch.w_layout == W_SPLIT:  # one blob: [3x3 panels][1x1 panels of the second source][scales]
                w = split_packed_weight(conv, self.math, conv2)
            else:
                w = pack[ch.w_layout if i == 0 else W_DIRECT](cv)
            self.keep.append(w)
            s = op.src[i]
            self._fill_src(s, v)
            s.w, s.ks, s.stride, s.pad_mode = w.data_ptr(), ks, st, pad_mode
            if cat is not None:
                s.Cin, s.up_c0, s.up_C = cat.C, cat.direct.C, cat.ups[0].C
                for ui, u in enumerate(cat.ups):
                    s.up_in[ui], s.up_cs[ui] = u.ptr, u.cs
            self.flops += 2 * out.N * out.H * out.W * cv.out_channels * cv.in_channels * ks * ks
        bias = conv.bias
        if conv2 is not None and conv2.bias is not None:
            bias = (conv.bias + conv2.bias).detach() if conv.bias is not None else conv2.bias
        self._keep_bias(op, bias)
        if res is not None:
            op.res, op.res_cs = res.ptr, res.cs
        op.out, op.out_cs = out.ptr, out.cs
        op.Ho, op.Wo, op.Cout = out.H, out.W, conv.out_channels
        op.act, op.slope = act, slope
        M = out.N * out.H * out.W
        op.tile_m, op.tile_n, op.split_k = tm, tn, split = ch.tile_m, ch.tile_n, ch.split_k
        if norm is not None:
            stats, n_act, n_slope = norm
            if tm not in (8, 9) or tn != 1 or x2 is not None or isinstance(x, CatView) or tuple(stats.shape) != (x.N, 2, x.C):
                raise _lib.IdhError("normalise-on-load needs the LDS-staged fp32 conv with 16-channel tiles and one source")
            op.src[0].norm, op.src[0].norm_act, op.src[0].norm_slope = stats.data_ptr(), n_act, n_slope
        if split > 1:
            ws = torch.empty(split * M * ceil16(conv.out_channels), device=self.device, dtype=torch.float32)
            self.keep.append(ws)
            op.ws = ws.data_ptr()
        reads = ([_region(res)] if res is not None else []) + ([(norm[0].data_ptr(), 0, 1)] if norm is not None else [])
        for v, _ in srcs:
            if isinstance(v, CatView):
                reads += [_region(v.direct)] + [_region(u) for u in v.ups]
            else:
                reads.append(_region(v, pad16=True))
        self._record(op, reads, [_region(out)])
        return out

    def upsample2(self, x: View, out: View, nearest: bool = False):
        op = Op(kind=OP_UPSAMPLE2_NEAREST if nearest else OP_UPSAMPLE2, N=x.N, out=out.ptr, out_cs=out.cs)
        self._fill_src(op.src[0], x)
        self._record(op, [_region(x)], [_region(out)])
        return out

    def pointwise_up(self, x: View, conv: nn.Conv2d, low: View, out: View):
        """out = conv1x1(x) + upsample2(low) (IDH_OP_POINTWISE_UP, csrc/conv.hip pointwise_up_k)."""
        if conv.kernel_size[0] != 1 or conv.in_channels != x.C or conv.out_channels != out.C or low.C != out.C or (2 * low.H, 2 * low.W) != (x.H, x.W):
            raise _lib.IdhError("pointwise_up: a 1x1 conv of x plus the x2 upsampling of a half-resolution map with the output's channels")
        op = Op(kind=OP_POINTWISE_UP, N=x.N, out=out.ptr, out_cs=out.cs, Ho=out.H, Wo=out.W, Cout=out.C)
        w = packed_weight(conv)
        self.keep.append(w)
        s = op.src[0]
        self._fill_src(s, x)
        s.w, s.ks, s.stride = w.data_ptr(), 1, 1
        self._fill_src(op.src[1], low)
        self._keep_bias(op, conv.bias)
        self.flops += 2 * x.N * x.H * x.W * conv.out_channels * conv.in_channels
        self._record(op, [_region(x), _region(low)], [_region(out)])
        return out

    def instance_norm(self, x: View, out: Optional[View], act=ACT_NONE, slope=0.2):
        """nn.InstanceNorm2d(C) (no affine, eps 1e-5) optionally followed by LeakyReLU.  ``out=None``: statistics only —
        returns the (N, 2, C) mean / rstd tensor for a consumer conv that normalises on load (``conv(..., norm=...)``)."""
        if x.C % 4 or 256 % (x.C // 4):
            raise _lib.IdhError(f"instance-norm kernel needs C/4 to divide 256 (C={x.C})")
        op = Op(kind=OP_INSTNORM, N=x.N, act=act, slope=slope)
        self._fill_src(op.src[0], x)
        if out is not None:
            op.out, op.out_cs = out.ptr, out.cs
        nchunks = -(-(x.H * x.W) // 1024)
        ws = torch.empty(x.N * (nchunks + 1) * 2 * x.C, device=self.device, dtype=torch.float32)
        self.keep.append(ws)
        op.ws = ws.data_ptr()
        stats = ws[x.N * nchunks * 2 * x.C:].view(x.N, 2, x.C)
        self._record(op, [_region(x)], [_region(out)] if out is not None else [(stats.data_ptr(), 0, 1)])
        return out if out is not None else stats

    def copy(self, x: View, out: View):
        """NHWC view -> NHWC view (e.g. an existing feature map into a slice of a concat buffer)."""
        if (x.N, x.H, x.W, x.C) != (out.N, out.H, out.W, out.C):
            raise _lib.IdhError("copy: shape mismatch")
        op = Op(kind=OP_COPY, N=x.N, out=out.ptr, out_cs=out.cs)
        self._fill_src(op.src[0], x)
        self._record(op, [_region(x)], [_region(out)])
        return out

    def import_nchw(self, shape_nchw, out: View) -> int:
        """(N,C,H,W) dense -> NHWC slice.  The source pointer is patched per call with
        ``set_in``; returns the op index."""
        N, Cc, H, W = [int(v) for v in shape_nchw]
        if (N, H, W, Cc) != (out.N, out.H, out.W, out.C):
            raise _lib.IdhError(f"import of {tuple(shape_nchw)} into a view of {(out.N, out.C, out.H, out.W)}")
        op = Op(kind=OP_IMPORT, N=N, out=out.ptr, out_cs=out.cs)
        s = op.src[0]
        s.H, s.W, s.Cin = H, W, Cc
        return self._record(op, [], [_region(out)])

    def input_nchw(self, shape_nchw):
        """A plan buffer for a dense (N,C,H,W) input and its layout import: (the NHWC view, the import's op index for ``set_in``)."""
        N, Cc, H, W = [int(v) for v in shape_nchw]
        v = self.buffer(N, H, W, Cc)
        return v, self.import_nchw(shape_nchw, v)

    @staticmethod
    def pointwise_nchw_eligible(conv: nn.Conv2d) -> bool:
        """Shape family of csrc/conv.hip pointwise_nchw_k: the matching head's nn.Conv2d(64, 128, 1)."""
        return (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.in_channels == 64 and conv.out_channels == 128
                and conv.groups == 1)

    def pointwise_nchw(self, shape_nchw, conv: nn.Conv2d, out: View) -> int:
        """1x1 conv read straight from a dense (N,C,H,W) tensor into an NHWC view (IDH_OP_POINTWISE_NCHW): layout
        import and convolution in one pass.  The source pointer is patched per call with ``set_in``; returns the op index."""
        N, Cc, H, W = [int(v) for v in shape_nchw]
        if (N, H, W) != (out.N, out.H, out.W) or Cc != conv.in_channels or out.C != conv.out_channels or not self.pointwise_nchw_eligible(conv):
            raise _lib.IdhError(f"pointwise_nchw: {tuple(shape_nchw)} with {conv} into a view of {(out.N, out.C, out.H, out.W)}")
        op = Op(kind=OP_POINTWISE_NCHW, N=N, out=out.ptr, out_cs=out.cs, Ho=H, Wo=W, Cout=conv.out_channels)
        s = op.src[0]
        w = packed_weight(conv)
        self.keep.append(w)
        s.w, s.H, s.W, s.Cin, s.ks, s.stride = w.data_ptr(), H, W, Cc, 1, 1
        self._keep_bias(op, conv.bias)
        self.flops += 2 * N * H * W * conv.out_channels * conv.in_channels
        return self._record(op, [], [_region(out)])

    def stem(self, shape, strides, blob: torch.Tensor, out: View) -> int:
        """conv1 + folded BatchNorm + ReLU + MaxPool2d(2, 1) + BlurPool of the ResNet18 stem (IDH_OP_STEM, csrc/stem.hip) from N fp32 NCHW
        images into an NHWC view of 64 channels.  ``shape`` = (N, 3, H, W); ``strides`` = (images per group, floats between the images of
        a group, floats between groups) - a (B, K+1, 3, H, W) tensor is B groups of K+1; ``blob`` = ``idh_pack_stem_weight`` output.  The
        image pointer is patched per call with ``set_in``; returns the op index."""
        N, Cc, H, W = [int(v) for v in shape]
        Ho, Wo = ((H + 1) // 2) // 2, ((W + 1) // 2) // 2
        if Cc != 3 or H < 8 or W < 8 or (out.N, out.H, out.W, out.C) != (N, Ho, Wo, 64):
            raise _lib.IdhError(f"stem: images {tuple(shape)} (3 channels, H, W >= 8) into a view of {(out.N, out.C, out.H, out.W)}")
        group, img_stride, grp_stride = [int(v) for v in strides]
        if max(img_stride, grp_stride) >= 1 << 31 or N % group:
            raise _lib.IdhError("stem: image strides must fit in 32 bits and the groups divide the batch")
        op = Op(kind=OP_STEM, N=N, out=out.ptr, out_cs=out.cs, Ho=Ho, Wo=Wo, Cout=64)
        s = op.src[0]
        s.w, s.H, s.W, s.Cin = blob.data_ptr(), H, W, 3
        s.up_C, s.up_cs[0], s.up_cs[1] = group, img_stride, grp_stride
        self.keep.append(blob)
        self.flops += 2 * N * ((H + 1) // 2) * ((W + 1) // 2) * 64 * 147
        return self._record(op, [], [_region(out)])

    def export_nchw(self, x: View, out_nchw: Optional[torch.Tensor] = None) -> int:
        op = Op(kind=OP_EXPORT, N=x.N)
        self._fill_src(op.src[0], x)
        if out_nchw is not None:
            op.out = out_nchw.data_ptr()
        return self._record(op, [_region(x)], [])

    def head(self, x: View, conv: nn.Conv2d, out: torch.Tensor):
        """1x1 conv to one channel (DepthDecoderPP heads, reference networks.py:158-161)."""
        if conv.out_channels != 1 or conv.kernel_size != (1, 1):
            raise _lib.IdhError("pointwise head kernel covers Conv2d(C,1,1) only")
        op = Op(kind=OP_HEAD, N=x.N, out=out.data_ptr())
        w = conv.weight.detach().reshape(-1).contiguous()
        b = conv.bias.detach().contiguous()
        self.keep += [w, b]
        self._fill_src(op.src[0], x)
        op.src[0].w, op.bias = w.data_ptr(), b.data_ptr()
        return self._record(op, [_region(x)], [])

    # composite: BasicBlock (reference layers.py:78-95) ---------------------------------
    def basic_block(self, x: View, blk, out: Optional[View] = None) -> View:
        st = blk.conv1.stride[0]
        Ho = (x.H + 2 - 3) // st + 1
        Wo = (x.W + 2 - 3) // st + 1
        planes = blk.conv1.out_channels
        h = self.buffer(x.N, Ho, Wo, planes)
        self.conv(x, blk.conv1, h, act=ACT_LRELU, slope=0.2)
        if out is None:
            out = self.buffer(x.N, Ho, Wo, planes)
        if blk.downsample is None:
            self.conv(h, blk.conv2, out, act=ACT_LRELU, slope=0.2, res=x)
        elif (self.math != "fp32" and blk.downsample[0].kernel_size[0] == 3
              and split_eligible([(h, blk.conv2)], planes, x.N, Ho, Wo, PAD_ZEROS)):
            # stride-2 block: the strided 3x3 projection (1/3 of the block's conv2-stage flops) runs on its own with
            # the fp32 direct kernel and enters the split-precision conv2 as the residual
            proj = self.buffer(x.N, Ho, Wo, planes)
            self.conv(x, blk.downsample[0], proj)
            self.conv(h, blk.conv2, out, act=ACT_LRELU, slope=0.2, res=proj)
        else:
            self.conv(h, blk.conv2, out, act=ACT_LRELU, slope=0.2, x2=x, conv2=blk.downsample[0])
        self.release(h)  # the block's intermediate dies with conv2
        return out

    def basic_block_upcat(self, cat: View, lows: List[View], blk) -> Optional[View]:
        """BasicBlock on cat = [right | up(lows[0]) | up(lows[1])...] (the UNet++ decoders' in_conv, networks.py:52-77) with the projection
        branch split by linearity: a 1x1 conv commutes with bilinear upsampling (its weights sum to one, so the bias may sit on either side),
        ``downsample(cat) = W_a right + up(W_b lo + W_c lo2 + b)``.  Two thirds of the projection run at a quarter of the pixels
        (one 1x1 conv on the low-resolution maps), ``pointwise_up_k`` adds the right slice's share, and conv2 takes the sum as an ordinary
        residual - the F(4x4) kernel's plain + residual instance instead of its projection phase over 3 x planes channels.  Same function as
        ``basic_block(cat, blk)`` up to fp32 rounding.  Returns None (caller falls back) where it does not apply: small grids (the extra
        launches cost more than the projection phase there), widths the pointwise kernel does not have."""
        ds = blk.downsample[0] if blk.downsample is not None else None
        planes = blk.conv1.out_channels
        c = planes
        if (not PROJ_LOWRES or self.math != "fp32" or ds is None or ds.kernel_size[0] != 1 or ds.stride[0] != 1 or planes not in (64, 128) or
                not 1 <= len(lows) <= 2 or cat.C != c * (1 + len(lows)) or any(l.C != c or (2 * l.H, 2 * l.W) != (cat.H, cat.W) for l in lows)):
            return None
        if cat.N * (-(-cat.H // 8)) * (-(-cat.W // 32)) * (planes // 64) < PROJ_LOWRES_MIN_TILES:
            return None
        key = (ds.weight.data_ptr(), _lib.param_version(ds.weight), None if ds.bias is None else _lib.param_version(ds.bias), str(ds.weight.device))
        parts = getattr(ds, "_idh_proj_parts", None)
        if parts is None or parts[0] != key:
            with torch.no_grad():
                mods = []
                for i in range(1 + len(lows)):
                    m = nn.Conv2d(c, planes, 1, bias=(i == 1 and ds.bias is not None)).to(ds.weight.device)
                    m.weight.copy_(ds.weight[:, i * c:(i + 1) * c])
                    if m.bias is not None:
                        m.bias.copy_(ds.bias)
                    m.requires_grad_(False)
                    mods.append(m)
            parts = (key, mods)
            ds._idh_proj_parts = parts
        wa, wb = parts[1][0], parts[1][1]
        wc = parts[1][2] if len(lows) == 2 else None
        plo = self.buffer(cat.N, lows[0].H, lows[0].W, planes)
        if wc is None:
            self.conv(lows[0], wb, plo)
        else:
            self.conv(lows[0], wb, plo, x2=lows[1], conv2=wc)
        r = self.buffer(cat.N, cat.H, cat.W, planes)
        self.pointwise_up(cat.slice(0, c), wa, plo, r)
        h = self.buffer(cat.N, cat.H, cat.W, planes)
        self.conv(cat, blk.conv1, h, act=ACT_LRELU, slope=0.2)
        out = self.buffer(cat.N, cat.H, cat.W, planes)
        self.conv(h, blk.conv2, out, act=ACT_LRELU, slope=0.2, res=r)
        self.release(h)
        self.release(r)
        self.release(plo)
        return out

    # scheduling ----------------------------------------------------------------------
    def schedule(self):
        """Re-order the ops by dependency level (longest path from the inputs) and mark the
        4-row-tile LDS convs of one level as a launch group: they are mutually independent, so
        ``idh_run_ops`` runs them as ONE grid.  This is how the many small low-resolution convs
        of the UNet++ grid (each filling only a fraction of 256 CUs) get to run side by side
        — the reference executes them strictly one after another."""
        self.schedule_segments(0)

    def schedule_segments(self, n_first: int) -> int:
        """``schedule()`` for a plan that is replayed in two pieces — ops [0, n_first) then the rest — because a
        kernel outside the plan (the fused cost volume) consumes the first piece's output and produces the second
        piece's input.  Each piece is levelled on its own; returns the length of the first piece."""
        n = len(self.ops)
        n_first = max(0, min(int(n_first), n))
        arr = (Op * n)(*self.ops)
        regions, offs = [], [0]  # idh_schedule_ops: flat (buffer id, c0, c1) triples; op k reads [offs[2k], offs[2k+1]) and writes [offs[2k+1], offs[2k+2])
        for m in self.meta:
            for rs in (m["reads"], m["writes"]):
                regions += [x for r in rs for x in r]
                offs.append(len(regions) // 3)
        order, levels = (C.c_int32 * n)(), (C.c_int32 * n)()
        flags = (SCHED_MERGE_LEVELS if MERGE_LEVELS else 0) | (SCHED_WINO_GROUP if WINO_GROUP else 0)
        _lib.check(_bind().idh_schedule_ops(arr, n, n_first, (C.c_uint64 * (len(regions) + 1))(*regions), (C.c_int32 * len(offs))(*offs), flags, order, levels),
                   "idh_schedule_ops")
        self.ops = list(arr)
        self.meta = [self.meta[k] for k in order]
        self.levels = list(levels)
        pos = [0] * n
        for new, old in enumerate(order):
            pos[old] = new
        self._pos = pos if self._pos is None else [pos[p] for p in self._pos]
        self._arr = None
        return n_first

    # execution -----------------------------------------------------------------------
    def _array(self):
        if self._arr is None:
            self._arr = (Op * len(self.ops))(*self.ops)
        return self._arr

    def _idx(self, idx: int) -> int:
        return idx if self._pos is None else self._pos[idx]

    def run(self, start: int = 0, end: Optional[int] = None):
        """Replay ops [start, end) (default: all) with one C-ABI call."""
        L = _bind()
        arr = self._array()
        end = len(self.ops) if end is None else end
        if end <= start:
            return
        base = C.addressof(arr) + start * C.sizeof(Op)
        _lib.check(L.idh_run_ops(C.c_void_p(base), end - start, _lib.stream_ptr()), "idh_run_ops")

    def count_launches(self, start: int = 0, end: Optional[int] = None) -> int:
        """Kernel launches ``run(start, end)`` issues (``idh_count_launches``: same decisions, nothing launched)."""
        L = _bind()
        arr = self._array()
        end = len(self.ops) if end is None else end
        if end <= start:
            return 0
        n = L.idh_count_launches(C.c_void_p(C.addressof(arr) + start * C.sizeof(Op)), end - start)
        if n < 0:
            _lib.check(n, "idh_count_launches")
        return n

    def set_in(self, idx: int, t: torch.Tensor):
        """idx = op index returned at build time (stable across schedule())."""
        self._array()[self._idx(idx)].src[0].in_ = t.data_ptr()

    def set_out(self, idx: int, t: torch.Tensor, exp_out: Optional[torch.Tensor] = None):
        """Patch an op's output pointer; ``exp_out``: the head op's optional exp(output) tensor."""
        op = self._array()[self._idx(idx)]
        op.out = t.data_ptr()
        if exp_out is not None:
            op.ws = exp_out.data_ptr()

    def run_with(self, ins=(), outs=()):
        """``run()`` on this call's tensors: (build index, tensor) pairs patched in with ``set_in`` / ``set_out`` first."""
        for i, t in ins:
            self.set_in(i, t)
        for i, t in outs:
            self.set_out(i, t)
        self.run()


def math_of(module: nn.Module) -> str:
    """Conv arithmetic of a drop-in module: its ``conv_math`` attribute (set by ``dropin.convert(model,
    math=...)``) or the process-wide DEFAULT_MATH."""
    return getattr(module, "conv_math", None) or DEFAULT_MATH


PLAN_CACHE_ENTRIES = 4


class ParamKey(tuple):
    """The part of a plan-cache key that names parameter versions / build-time switches (as opposed to input shapes)."""

    def __add__(self, other):  # (tuple.__add__ would hand back a plain tuple, which PlanCache.put's stale-twin eviction does not recognise)
        return ParamKey(tuple.__add__(self, other))


class PlanCache:
    """Small LRU of execution plans (one entry = ops + all activation buffers of one input shape): an evaluation loop whose last
    batch is ragged, or a caller alternating two layouts / batch sizes, replays instead of rebuilding; the oldest entry (and its
    buffers) goes when a fifth shape arrives.  The LRU is for SHAPES only: an entry that differs from a new key just in its ParamKey
    parts (weights reloaded or updated in place, a build switch toggled) can never be hit again, so it is dropped at once — a
    checkpoint load after a warm-up forward does not double the resident activation memory."""

    def __init__(self, entries: int = PLAN_CACHE_ENTRIES):
        import collections

        self.entries = entries
        self.d = collections.OrderedDict()

    def get(self, key):
        ent = self.d.get(key)
        if ent is not None:
            self.d.move_to_end(key)
        return ent

    @staticmethod
    def _same_shapes(a, b) -> bool:
        return (isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b) and
                all(x == y or (isinstance(x, ParamKey) and isinstance(y, ParamKey)) for x, y in zip(a, b)))

    def put(self, key, ent):
        for k in [k for k in self.d if k != key and self._same_shapes(k, key)]:
            del self.d[k]  # same shapes, stale parameters / switches
        self.d[key] = ent
        self.d.move_to_end(key)
        while len(self.d) > self.entries:
            self.d.popitem(last=False)
        return ent

    def values(self):
        return self.d.values()

    def __len__(self):
        return len(self.d)

    def clear(self):
        self.d.clear()


def build_flags() -> tuple:
    """Module-level switches that shape a plan at build time (part of every plan-cache key: toggling one takes effect on the
    next call instead of silently replaying a plan built under the old setting)."""
    return (WINO_GROUP, FUSE_UPSAMPLE, FUSED_UP_ROWS, MERGE_LEVELS, FUSE_HEAD_NORM, FUSE_HEAD_IMPORT, NARROW_TILE_BELOW, NARROWEST_TILE_BELOW, SPLIT_MIN_CHUNKS,
            SPLIT_MAX, SPLIT_MIN_BLOCKS, WINOGRAD, WINO_MIN_TILES, WINO_MIN_FILL, WINOGRAD4, WINOGRAD4_PROJ, WINO4_MIN_TILES, WINO4_MIN_FILL, BUFFER_REUSE, REUSE_MIN_BYTES, DEFAULT_MATH,
            S2_FIRST, S2_FIRST_MIN_BLOCKS, PROJ_CHUNK_WEIGHT, PROJ_LOWRES, PROJ_LOWRES_MIN_TILES)


def _plan_cache(module: nn.Module) -> PlanCache:
    c = module.__dict__.get("_idh_plans")
    if c is None:
        c = PlanCache()
        module.__dict__["_idh_plans"] = c
        _lib.watch_state_dict_loads(module)
    return c


def _param_key(module: nn.Module):
    return ParamKey((math_of(module), build_flags()) + tuple((p.data_ptr(), _lib.param_version(p)) for p in module.parameters()))


def cached_plan(module: nn.Module, key, device, build) -> tuple:
    """The drop-ins' cached replay: ``module``'s plan-cache entry (plan, *payload) under ``key``.  On a miss ``build(p)`` records the ops on
    a fresh ``Plan(device, math=math_of(module))`` and returns the payload (op indices, output views); the plan is scheduled, the entry kept."""
    cache = _plan_cache(module)
    ent = cache.get(key)
    if ent is None:
        p = Plan(device, math=math_of(module))
        payload = build(p)
        p.schedule()
        ent = cache.put(key, (p, *payload))
    return ent


def _check_in(*ts):
    for t in ts:
        _lib.require_cuda_f32(t)
        if t.dim() != 4:
            raise _lib.IdhError(f"expected NCHW tensors, got shape {tuple(t.shape)}")


# --- BasicBlock as a stand-alone drop-in ----------------------------------------------------
def block_forward_nchw(blk, x: torch.Tensor) -> torch.Tensor:
    _check_in(x)
    x = x.contiguous()

    def build(p: Plan):
        xin, i_in = p.input_nchw(x.shape)
        y = p.basic_block(xin, blk)
        return i_in, p.export_nchw(y), y

    p, i_in, i_out, y = cached_plan(blk, ("bb", tuple(x.shape), str(x.device), _param_key(blk)), x.device, build)
    out = torch.empty(y.N, y.C, y.H, y.W, device=x.device, dtype=torch.float32)
    p.run_with([(i_in, x)], [(i_out, out)])
    return out


# --- CVEncoder (reference networks.py:186-215) --------------------------------------------
def build_cv_encoder(p: Plan, enc, cost: View, img_feat_shapes: Sequence[Sequence[int]]):
    """Adds the encoder to plan ``p``.  Returns (outputs: List[View], import op indices for
    img_feats)."""
    outs, imports = [], []
    x = cost
    for i in range(enc.num_blocks):
        ds = enc.convs[f"ds_conv_{i}"]
        st = ds.conv1.stride[0]
        Ho, Wo = (x.H + 2 - 3) // st + 1, (x.W + 2 - 3) // st + 1
        cout = ds.conv1.out_channels
        cimg = img_feat_shapes[i][1]
        if tuple(img_feat_shapes[i][2:]) != (Ho, Wo):
            raise _lib.IdhError(f"img_feats[{i}] spatial size {tuple(img_feat_shapes[i][2:])} != {(Ho, Wo)}")
        cat = p.buffer(x.N, Ho, Wo, cout + cimg)
        p.basic_block(x, ds, out=cat.slice(0, cout))
        imports.append(p.import_nchw(img_feat_shapes[i], cat.slice(cout, cimg)))
        seq = enc.convs[f"conv_{i}"]
        y = p.basic_block(cat, seq[0])
        y = p.basic_block(y, seq[1])
        outs.append(y)
        x = y
    return outs, imports


def cv_encoder_forward_nchw(enc, x: torch.Tensor, img_feats: List[torch.Tensor]) -> List[torch.Tensor]:
    _check_in(x, *img_feats)
    x = x.contiguous()
    img_feats = [f.contiguous() for f in img_feats]
    key = ("cve", tuple(x.shape), tuple(tuple(f.shape) for f in img_feats), str(x.device), _param_key(enc))

    def build(p: Plan):
        xin, i_x = p.input_nchw(x.shape)
        outs, i_img = build_cv_encoder(p, enc, xin, [f.shape for f in img_feats])
        return [i_x] + i_img, [p.export_nchw(o) for o in outs], outs

    p, i_in, i_out, outs = cached_plan(enc, key, x.device, build)
    res = [torch.empty(o.N, o.C, o.H, o.W, device=x.device, dtype=torch.float32) for o in outs]
    p.run_with(zip(i_in, [x] + img_feats), zip(i_out, res))
    return res


# --- UNet++ decoders (reference networks.py:20-84, 118-183) ------------------------------
ALL_SCALES = 0b1111  # IDH_SCALES_ALL of include/idh_net.h: bit i = the caller reads the output_i result


def build_decoder(p: Plan, dec, feats: List[View], scales: int = ALL_SCALES):
    """Adds the UNet++ grid to ``p``; returns {scale i: View of the surviving output_i result
    (before the optional 1x1 depth head)} for the scales whose bit is set in ``scales``.  A scale that is not wanted gets no output_i
    block (two 3x3 convs and two buffers each); the grid node X(i, 4-i) under it is built either way, the next column reads it.  Scale 0
    (output_0[0] is nn.Identity: the grid's top-left node itself) is always returned."""
    prev = list(feats)
    outputs: List[View] = []
    final: Dict[int, View] = {}
    for j in range(1, 5):
        for i in range(4 - j, -1, -1):
            right = dec.convs[f"right_conv_{i}{j - 1}"]
            diag = dec.convs[f"diag_conv_{i + 1}{j - 1}"]
            cout = right.conv1.out_channels
            has_up = (i + j) != 4
            xi = prev[i]
            seq = dec.convs[f"in_conv_{i}{j}"]
            fuse = (FUSE_UPSAMPLE and p.math == "fp32" and cout % 16 == 0 and xi.W >= 16 and
                    lds_eligible([(xi, seq[0].conv1)], seq[0].conv1.out_channels, xi.W, PAD_ZEROS) and seq[0].downsample is not None and
                    seq[0].downsample[0].kernel_size[0] == 1)
            if fuse:  # torch.cat + F.interpolate live in the consumer's loader
                r = p.basic_block(xi, right)
                lo = p.basic_block(prev[i + 1], diag)
                if (lo.H * 2, lo.W * 2) != (xi.H, xi.W):
                    raise _lib.IdhError("decoder pyramid levels must differ by exactly x2")
                ups = [lo] + ([p.basic_block(outputs[-1], dec.convs[f"up_conv_{i + 1}{j}"])] if has_up else [])
                cat = CatView(r, ups)
            else:
                cat = p.buffer(xi.N, xi.H, xi.W, cout * (3 if has_up else 2))
                p.basic_block(xi, right, out=cat.slice(0, cout))
                lo = p.basic_block(prev[i + 1], diag)
                if (lo.H * 2, lo.W * 2) != (xi.H, xi.W):
                    raise _lib.IdhError("decoder pyramid levels must differ by exactly x2")
                if j > 1 and not has_up:
                    # (liveness reuse) prev[i + 1] is X(i+1, 4-(i+1)), the last node of its row: up_conv and the output head read it in the
                    # column before, this diag_conv was its last reader
                    p.release(prev[i + 1])
                p.upsample2(lo, cat.slice(cout, cout))
                lows = [lo]
                # (liveness reuse) the half-resolution maps have no reader after their upsampling - unless the low-resolution projection
                # (basic_block_upcat, PROJ_LOWRES) is going to read them again in in_conv's first block
                hold_lows = PROJ_LOWRES
                if not hold_lows:
                    p.release(lo)
                if has_up:
                    lo2 = p.basic_block(outputs[-1], dec.convs[f"up_conv_{i + 1}{j}"])
                    p.upsample2(lo2, cat.slice(2 * cout, cout))
                    lows.append(lo2)
                    if not hold_lows:
                        p.release(lo2)
            y0 = p.basic_block_upcat(cat, lows, seq[0]) if isinstance(cat, View) else None
            if y0 is None:
                y0 = p.basic_block(cat, seq[0])
            if isinstance(cat, View):
                if hold_lows:
                    for l in lows:
                        p.release(l)
                p.release(cat)
            y = p.basic_block(y0, seq.conv_0)
            p.release(y0)
            outputs.append(y)
            if j == 4 - i:  # the only (i,j) whose output_i result survives in the dict
                head = dec.convs[f"output_{i}"]
                if isinstance(head[0], nn.Identity):
                    final[i] = y
                elif (scales >> i) & 1:
                    final[i] = p.basic_block(y, head[0])
        prev = outputs[::-1]
    return final


def decoder_forward_nchw(dec, input_features: List[torch.Tensor]) -> Dict[str, torch.Tensor]:
    _check_in(*input_features)
    feats = [f.contiguous() for f in input_features]
    dev, depth_head = feats[0].device, getattr(dec, "depth_head", False)

    def build(p: Plan):
        views, i_in = zip(*[p.input_nchw(f.shape) for f in feats])
        final = build_any_decoder(p, dec, list(views))
        if depth_head:
            i_out = {i: p.head(v, dec.convs[f"output_{i}"][1], torch.empty(1, device=dev)) for i, v in final.items()}
        else:
            i_out = {i: p.export_nchw(v) for i, v in final.items()}
        return i_in, i_out, final

    key = ("dec", tuple(tuple(f.shape) for f in feats), str(dev), _param_key(dec))
    p, i_in, i_out, final = cached_plan(dec, key, dev, build)
    res = {i: torch.empty(v.N, 1 if depth_head else v.C, v.H, v.W, device=dev, dtype=torch.float32) for i, v in final.items()}
    p.run_with(zip(i_in, feats), [(i_out[i], t) for i, t in res.items()])
    return {dec.out_key.format(i): t for i, t in res.items()}


def binary_mlp_forward(net, inputs, max_scale_only):
    from .mlp import binary_mlp_forward as f

    return f(net, inputs, max_scale_only)


# --- matching-encoder head (reference networks.py:279-283) ---------------------------------
def norm_on_load_eligible(p: Plan, x: View, conv: nn.Conv2d, pad_mode: int) -> bool:
    """Can ``conv`` read ``x`` through a fused InstanceNorm (idh_conv_src.norm)?  LDS-staged fp32 3x3 kernel, 16-channel
    output tiles, whole 16-channel input blocks."""
    return (p.math == "fp32" and x.C % 16 == 0 and lds_subtiles(conv.out_channels) == 1 and
            lds_eligible([(x, conv)], conv.out_channels, x.W, pad_mode))


def build_matching_head(p: Plan, enc, x: Optional[View], nchw_shape=None):
    """Head of ResnetMatchingEncoder (reference modules/networks.py:279-283) on an NHWC view ``x`` — or, with
    ``nchw_shape`` = (N, C, H, W) and ``x`` = None, directly on the backbone's dense NCHW tensor: the first 1x1 conv then
    reads it in place (``Plan.pointwise_nchw``) and the index of that op is returned next to the output view so the caller
    can patch the source pointer."""
    c1, c2 = enc.net[5], enc.net[8]
    if nchw_shape is not None:
        N, _, H, W = [int(v) for v in nchw_shape]
        h = p.buffer(N, H, W, c1.out_channels)
        i_in = p.pointwise_nchw(nchw_shape, c1, h)
        x = h  # dims only
    else:
        h = p.buffer(x.N, x.H, x.W, c1.out_channels)
        p.conv(x, c1, h)
    y = p.buffer(x.N, x.H, x.W, c2.out_channels)
    if FUSE_HEAD_NORM and norm_on_load_eligible(p, h, c2, PAD_REPLICATE):
        # InstanceNorm2d(128) + LeakyReLU: one statistics pass; the 3x3 conv normalises while staging its halo
        stats = p.instance_norm(h, None)
        p.conv(h, c2, y, pad_mode=PAD_REPLICATE, norm=(stats, ACT_LRELU, 0.2))
    else:
        hn = p.buffer(x.N, x.H, x.W, c1.out_channels)
        p.instance_norm(h, hn, act=ACT_LRELU, slope=0.2)
        p.conv(hn, c2, y, pad_mode=PAD_REPLICATE)
    out = p.buffer(x.N, x.H, x.W, c2.out_channels)
    p.instance_norm(y, out)
    return out if nchw_shape is None else (out, i_in)


def matching_head_forward(enc, feat_nchw: torch.Tensor, channels_last: bool = False) -> torch.Tensor:
    _check_in(feat_nchw)
    x = feat_nchw.contiguous()
    key = ("mh", tuple(x.shape), str(x.device), channels_last, _param_key(enc.net[5]) + _param_key(enc.net[8]))

    def build(p: Plan):
        if FUSE_HEAD_IMPORT and Plan.pointwise_nchw_eligible(enc.net[5]):
            y, i_in = build_matching_head(p, enc, None, nchw_shape=x.shape)
        else:
            xin, i_in = p.input_nchw(x.shape)
            y = build_matching_head(p, enc, xin)
        return i_in, None if channels_last else p.export_nchw(y), y

    return _run_encoder_plan(cached_plan(enc, key, x.device, build), x, channels_last)


def _run_encoder_plan(ent, x: torch.Tensor, channels_last: bool) -> torch.Tensor:
    """Replay a matching-encoder entry (plan, input op, export op or None, output view) on ``x``: NCHW, or a copy of the NHWC map."""
    p, i_in, i_out, y = ent
    if channels_last:
        p.run_with([(i_in, x)])
        return y.dense().clone()
    out = torch.empty(y.N, y.C, y.H, y.W, device=x.device, dtype=torch.float32)
    p.run_with([(i_in, x)], [(i_out, out)])
    return out


# --- the ResNet18 stem of the matching encoder (implicit-depth_amd/backbone.py) ---------------------------------------------------
class FoldedStem:
    """Eval-mode BatchNorms of the stem folded into its convolutions: ``blob`` (conv1 + bn1 for IDH_OP_STEM, idh_pack_stem_weight) and
    four bias-carrying ``nn.Conv2d`` (layer1[b].conv1 + bn1, conv2 + bn2), which ``Plan.conv`` packs and caches like any other conv.
    Folded on the device by ``idh_fold_conv_bn`` (the same arithmetic as the C entry idh_matching_stem_pack)."""

    def __init__(self, stem, device):
        L = _bind()
        sp = _lib.stream_ptr()
        conv1, bn1, layer1 = stem[0], stem[1], stem[4]
        f = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        bn_args = lambda bn: [f(bn.weight), f(bn.bias), f(bn.running_mean), f(bn.running_var)]
        self.blob = torch.empty(L.idh_stem_weight_floats(), device=device, dtype=torch.float32)
        a = [f(conv1.weight)] + bn_args(bn1)
        _lib.check(L.idh_pack_stem_weight(*[t.data_ptr() for t in a], float(bn1.eps), self.blob.data_ptr(), sp), "idh_pack_stem_weight")
        self.convs = []
        for blk in layer1:
            for conv, bn in ((blk.conv1, blk.bn1), (blk.conv2, blk.bn2)):
                c = nn.Conv2d(conv.in_channels, conv.out_channels, 3, padding=1, bias=True).to(device)
                c.requires_grad_(False)
                w, b = torch.empty_like(c.weight), torch.empty_like(c.bias)
                a = [f(conv.weight)] + bn_args(bn)
                _lib.check(L.idh_fold_conv_bn(a[0].data_ptr(), conv.out_channels, conv.in_channels * 9, *[t.data_ptr() for t in a[1:]], float(bn.eps),
                                              w.data_ptr(), b.data_ptr(), sp), "idh_fold_conv_bn")
                c.weight.data, c.bias.data = w, b
                self.convs.append(c)


def stem_param_key(stem) -> ParamKey:
    """Parameters AND buffers (BatchNorm running statistics) of the stem, with the BatchNorm eps values."""
    from .backbone import stem_bns

    mods = list(stem)
    ts = [t for m in mods for t in list(m.parameters()) + list(m.buffers())]
    return ParamKey(tuple((t.data_ptr(), _lib.param_version(t)) for t in ts) + tuple(float(bn.eps) for bn in stem_bns(mods)))


def folded_stem(enc, device) -> FoldedStem:
    """The encoder's FoldedStem, cached on it and rebuilt when a stem parameter or BatchNorm statistic changes (``load_state_dict``
    bumps the epoch of inference-mode tensors, ``_lib.watch_state_dict_loads``)."""
    stem = enc.net[:5]
    require_native_stem(enc)
    key = (stem_param_key(stem), str(device))
    c = enc.__dict__.get("_idh_folded_stem")
    if c is not None and c[0] == key:
        return c[1]
    fs = FoldedStem(stem, device)
    enc.__dict__["_idh_folded_stem"] = (key, fs)
    return fs


def require_native_stem(enc) -> None:
    from .backbone import stem_bns, stem_is_native_eligible

    stem = list(enc.net[:5])
    try:
        bns = stem_bns(stem)
    except (AttributeError, IndexError, TypeError):
        bns = []
    if any(isinstance(bn, nn.BatchNorm2d) and bn.training for bn in bns):
        raise _lib.IdhError("the native matching stem is inference-only: a stem BatchNorm is in training mode (call .eval(); there is no CPU fallback)")
    if not stem_is_native_eligible(stem):
        raise _lib.IdhError("the matching encoder's net[:5] is not the resnet18(filter_size=4, pool_only=True) stem the native kernels compute "
                            "(implicit-depth_amd/backbone.py: stem_is_native_eligible)")


def image_strides(images: torch.Tensor):
    """(images, (N, 3, H, W), (group, image stride, group stride)) for an (N, 3, H, W) or (B, K+1, 3, H, W) fp32 tensor whose images are
    dense; any other layout is made contiguous first."""
    if images.dim() not in (4, 5) or images.shape[-3] != 3:
        raise _lib.IdhError(f"expected (N, 3, H, W) or (B, K+1, 3, H, W) images, got {tuple(images.shape)}")
    H, W = images.shape[-2:]
    if tuple(images.stride()[-3:]) != (H * W, W, 1):
        images = images.contiguous()
    if images.dim() == 4:
        N = images.shape[0]
        return images, (N, 3, H, W), (N, images.stride(0), N * images.stride(0))
    B, K1 = images.shape[:2]
    if B > 1 and K1 > 1 and images.stride(0) < K1 * images.stride(1):
        images = images.contiguous()  # overlapping groups: not an addressing the kernel is meant for
    return images, (B * K1, 3, H, W), (K1, images.stride(1), images.stride(0))


def build_matching_stem(p: Plan, enc, images: torch.Tensor, out: Optional[View] = None):
    """conv1 .. layer1 of the encoder's ResNet18 stem (backbone.py) on raw images: the fused IDH_OP_STEM pass, then layer1's two
    BasicBlocks as four ``Plan.conv`` ops with the BatchNorms folded in (ReLU = LeakyReLU with slope 0; conv2 adds the block input in its
    epilogue) - on conv3x3_wino4_k at every batch size (fp32 plans), so one image's layer1 map is bit-identical to the same image's in any batch.  ``images``: a tensor of the call's shape and strides (N, 3, H, W) or
    (B, K+1, 3, H, W) (only its geometry is recorded; the pointer is patched per call with ``set_in``).  Returns (the layer1 map as an
    NHWC view of 64 channels, the stem op's index)."""
    fs = folded_stem(enc, p.device)
    _, shape, strides = image_strides(images)
    N, _, H, W = shape
    Ho, Wo = ((H + 1) // 2) // 2, ((W + 1) // 2) // 2
    x = p.buffer(N, Ho, Wo, 64)
    i_img = p.stem(shape, strides, fs.blob, x)
    for b in range(2):
        c1, c2 = fs.convs[2 * b], fs.convs[2 * b + 1]
        h = p.buffer(N, Ho, Wo, 64)
        p.conv(x, c1, h, act=ACT_LRELU, slope=0.0, wino4_any_size=True)
        y = out if (b == 1 and out is not None) else p.buffer(N, Ho, Wo, 64)
        p.conv(h, c2, y, act=ACT_LRELU, slope=0.0, res=x, wino4_any_size=True)
        p.release(h)
        if b == 0:
            p.release(x)
        x = y
    return x, i_img


def matching_encoder_forward(enc, images: torch.Tensor, channels_last: bool = False, head: bool = True) -> torch.Tensor:
    """ResnetMatchingEncoder.forward with a native stem: raw (N, 3, H, W) images -> stem -> layer1 -> head (``head=False``: the layer1
    map) in one plan, NHWC throughout.  Returns NCHW, or with ``channels_last`` the (N, H, W, C) map (as ``matching_head_forward``)."""
    require_native_stem(enc)
    _lib.require_cuda_f32(images)
    if images.dim() != 4:
        raise _lib.IdhError(f"expected NCHW images, got shape {tuple(images.shape)}")
    images, shape, strides = image_strides(images)
    pk = stem_param_key(enc.net[:5]) + ((_param_key(enc.net[5]) + _param_key(enc.net[8])) if head else ParamKey())
    key = ("stem", tuple(shape), strides, str(images.device), channels_last, head, pk)

    def build(p: Plan):
        y, i_in = build_matching_stem(p, enc, images)
        if head:
            y = build_matching_head(p, enc, y)
        return i_in, None if channels_last else p.export_nchw(y), y

    return _run_encoder_plan(cached_plan(enc, key, images.device, build), images, channels_last)


# --- SkipDecoder / SkipDecoderRegression (reference modules/networks_fast.py:10-145) ------------
def _conv_block(p: Plan, x: View, blk, out: Optional[View] = None) -> View:
    """ConvBlock: conv3x3 -> ELU -> conv3x3 -> ELU (networks_fast.py:10-28); ReLU (= LeakyReLU with slope 0) with use_elu=False."""
    act, slope = (ACT_LRELU, 0.0) if isinstance(blk.non_lin, nn.ReLU) else (ACT_ELU, 0.2)
    h = p.buffer(x.N, x.H, x.W, blk.conv1.out_channels)
    p.conv(x, blk.conv1, h, act=act, slope=slope)
    if out is None:
        out = p.buffer(x.N, x.H, x.W, blk.conv2.out_channels)
    p.conv(h, blk.conv2, out, act=act, slope=slope)
    p.release(h)
    return out


def build_skip_decoder(p: Plan, dec, feats: List[View]) -> Dict[int, View]:
    """features[-1] -> block1..block4, each: ConvBlock, nearest x2, concat skip, ConvBlock."""
    x = feats[-1]
    final: Dict[int, View] = {}
    for bi, blk in enumerate((dec.block1, dec.block2, dec.block3, dec.block4)):
        skip = feats[-2 - bi]
        cout = blk.pre_concat_conv.conv2.out_channels
        y = _conv_block(p, x, blk.pre_concat_conv)
        if (y.H * 2, y.W * 2) != (skip.H, skip.W):
            raise _lib.IdhError("decoder pyramid levels must differ by exactly x2")
        cat = p.buffer(skip.N, skip.H, skip.W, cout + skip.C)
        p.upsample2(y, cat.slice(0, cout), nearest=True)
        p.copy(skip, cat.slice(cout, skip.C))  # torch.cat([x, cat_feats], 1), networks_fast.py:44
        x = _conv_block(p, cat, blk.post_concat_conv)
        final[3 - bi] = x
    return final


def build_any_decoder(p: Plan, dec, feats: List[View], scales: int = ALL_SCALES) -> Dict[int, View]:
    """UNet++ (BDDecoderPP / DepthDecoderPP) or skip decoder, by the structure of ``dec``.  ``scales``: see ``build_decoder`` (a skip
    decoder's scales feed one another: it always builds all of them)."""
    if hasattr(dec, "block1"):
        return build_skip_decoder(p, dec, feats)
    return build_decoder(p, dec, feats, scales)


def build_regression_heads(p: Plan, dec, final: Dict[int, View]) -> Dict[int, "tuple"]:
    """SkipDecoderRegression heads (networks_fast.py:106-145): 1x1 conv -> ELU -> 1x1 conv -> ELU ->
    1x1 conv to one channel, per scale.  Returns {scale: (View of the 128-ch penultimate map, last Conv2d)}."""
    heads = {}
    for i, seq in ((3, dec.out1), (2, dec.out2), (1, dec.out3), (0, dec.out4)):
        v = final[i]
        h1 = p.buffer(v.N, v.H, v.W, seq[0].out_channels)
        p.conv(v, seq[0], h1, act=ACT_ELU)
        h2 = p.buffer(v.N, v.H, v.W, seq[2].out_channels)
        p.conv(h1, seq[2], h2, act=ACT_ELU)
        heads[i] = (h2, seq[4])
    return heads


def skip_regression_forward_nchw(dec, input_features: List[torch.Tensor]) -> Dict[str, torch.Tensor]:
    """SkipDecoderRegression.forward (networks_fast.py:137-145): feature maps + log-depth heads."""
    _check_in(*input_features)
    feats = [f.contiguous() for f in input_features]
    dev = feats[0].device

    def build(p: Plan):
        views, i_in = zip(*[p.input_nchw(f.shape) for f in feats])
        final = build_skip_decoder(p, dec, list(views))
        heads = build_regression_heads(p, dec, final)
        i_feat = {i: p.export_nchw(v) for i, v in final.items()}
        i_head = {i: p.head(hv, last, torch.empty(1, device=dev)) for i, (hv, last) in heads.items()}
        return i_in, i_feat, i_head, final

    key = ("skipreg", tuple(tuple(f.shape) for f in feats), str(dev), _param_key(dec))
    p, i_in, i_feat, i_head, final = cached_plan(dec, key, dev, build)
    res, outs = {}, []
    for i, v in final.items():
        res[f"feature_s{i}_b1hw"] = t = torch.empty(v.N, v.C, v.H, v.W, device=dev)
        res[f"log_depth_pred_s{i}_b1hw"] = d = torch.empty(v.N, 1, v.H, v.W, device=dev)
        outs += [(i_feat[i], t), (i_head[i], d)]
    p.run_with(zip(i_in, feats), outs)
    return res
