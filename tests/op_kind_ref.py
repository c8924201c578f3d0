"""Hand-built ``idh_op`` descriptors for every op kind of include/idh_ops.h other than IDH_OP_CONV / IDH_OP_STEM, and their references.

``nhwc.Plan`` reaches the layout imports / exports, the two upsamplings, the concat copy, the 1-channel head, the two fused pointwise kernels
and InstanceNorm only at the shapes a network produces.  test_op_kinds_cpu.py / test_op_kinds_gpu.py build the descriptors themselves
(csrc/conv.hip: one run_<kind> function per op kind): the smallest shapes that still have a tail, strided inputs and outputs, the grouped import
grid, and one "large" case per kernel whose grid is capped - the only way its grid-stride / persistent loop takes a second trip.

Buffers follow the hostile convention of tests/conv_op_ref.py: an NHWC output is channels [OUT_C0, OUT_C0 + C) of a wider buffer prefilled
with the PREFILL bit pattern, a dense NCHW output (export, head, head-exp) is images [1, N + 1) of an (N + 2)-image prefilled tensor, and
every strided input carries NaN in its channel padding.  "clean" = every element outside the written range still holds the pattern.
"""
import os
import re
import zlib

import torch
import torch.nn.functional as F

import conv_op_ref as R
from conv_op_ref import EINVAL, EUNSUPPORTED, OK, OUT_C0, PREFILL, U, _padded, fake_ptr, op_array, prefill, read_output  # noqa: F401

ACT_LRELU, SLOPE = R.ACT_LRELU, R.SLOPE

# kind name -> (IDH_OP_* code, the name of the code in include/idh_ops.h)
KINDS = {
    "import": (3, "NCHW_TO_NHWC"), "export": (4, "NHWC_TO_NCHW"), "copy": (9, "COPY"), "nearest": (8, "UPSAMPLE2_NEAREST"),
    "up2": (2, "UPSAMPLE2"), "head": (6, "POINTWISE_HEAD"), "pw_nchw": (10, "POINTWISE_NCHW"), "pw_up": (11, "POINTWISE_UP"),
    "instnorm": (7, "INSTNORM"),
}
NOT_HERE = {"CONV": 1, "STEM": 12}  # tests/conv_op_ref.py, tests/test_stem_*.py
RESERVED = {"SPLITK_REDUCE": 5}     # never accepted (test_conv_op_matrix_cpu.py::test_kind_5_is_reserved)
BIT_EXACT = ("import", "export", "copy", "nearest")  # pure data movement
DENSE_OUT = ("export", "head")                       # the output is a dense (N, C, H, W) tensor

# The grid caps of csrc/conv.hip (named constants there, each used by the run_<kind> function of its op kind), in workgroups of 256 threads,
# and what one workgroup takes (natural_grid below).  test_op_kinds_cpu.py::test_mirrored_caps_are_the_sources holds them against the source.
CAP_COPY = 8192      # kCopyMaxBlocks  (IDH_OP_COPY, one thread per channel quad of a pixel)
CAP_NEAREST = 8192   # kNearestMaxBlocks  (IDH_OP_UPSAMPLE2_NEAREST, one thread per OUTPUT channel quad)
CAP_HEAD = 8192      # kHeadMaxBlocks  (IDH_OP_POINTWISE_HEAD, one thread per pixel)
CAP_UP2 = 32768      # kUpsampleMaxBlocks  (lone IDH_OP_UPSAMPLE2, one thread per INPUT channel quad)
CAP_PW_NCHW = 4096   # kPwNchwMaxBlocks = 256 * 4 * 4  (IDH_OP_POINTWISE_NCHW, one workgroup per tile of 64 pixels)
CAP_PW_UP = 2048     # kPwUpMaxBlocks = 256 * 8  (IDH_OP_POINTWISE_UP, one workgroup per tile of 64 pixels)
CAPS = {"copy": CAP_COPY, "nearest": CAP_NEAREST, "head": CAP_HEAD, "up2": CAP_UP2, "pw_nchw": CAP_PW_NCHW, "pw_up": CAP_PW_UP}
K_MAX_IMPORT = 8               # kMaxImport
IMPORT_GROUP_MAX_BLOCKS = 4096  # kImportGroupMaxBlocks = 8 * kLevelMaxBlocks: a larger import keeps its own 3-D grid
PW_TILE = 64                   # kPwTile


class KSpec:
    """One op.  H, W, C = size and channels of source 0 (the 1-channel head: its input channels; pointwise_nchw: 64 -> 128)."""

    def __init__(self, kind, name, N, H, W, C, bias=True, exp=False, out=True, large=False):
        self.kind, self.name, self.N, self.H, self.W, self.C = kind, name, N, H, W, C
        self.bias, self.exp, self.out, self.large = bias, exp, out, large

    def with_n(self, n):
        s = KSpec(self.kind, self.name, n, self.H, self.W, self.C, self.bias, self.exp, self.out, self.large)
        return s

    # ---- geometry ------------------------------------------------------------------------------------------------
    @property
    def cout(self):  # channels written
        return {"head": 1, "pw_nchw": 128}.get(self.kind, self.C)

    @property
    def out_hw(self):
        return (2 * self.H, 2 * self.W) if self.kind in ("nearest", "up2") else (self.H, self.W)

    @property
    def in_cs(self):  # channel stride of source 0 (dense NCHW sources: unused)
        if self.kind == "export":
            return self.C + 5  # scalar loads: any stride >= C
        if self.kind == "pw_up":
            return 3 * self.C  # x = channels [C, 2C) of the decoder's concat buffer
        return self.C + 4

    @property
    def in_c0(self):
        return self.C if self.kind == "pw_up" else 0

    @property
    def low_cs(self):
        return self.C + 8

    @property
    def out_cs(self):
        return self.cout + 8

    @property
    def launches(self):
        if self.kind == "instnorm":
            return 3 if self.out else 2
        return 1

    def image_floats(self, name):
        """Floats between consecutive images of a buffer (the sub-range runs of the large cases advance every pointer by them)."""
        H, W = self.H, self.W
        if name == "x":
            return self.C * H * W if self.kind in ("import", "pw_nchw") else H * W * self.in_cs
        if name == "low":
            return (H // 2) * (W // 2) * self.low_cs
        Ho, Wo = self.out_hw
        if name == "out":
            return self.cout * Ho * Wo if self.kind in DENSE_OUT else Ho * Wo * self.out_cs
        if name == "exp":
            return Ho * Wo
        return 0  # weights, bias


def natural_grid(spec, n=None):
    """Workgroups the launch would have without its cap."""
    n = spec.N if n is None else n
    HW, cq = spec.H * spec.W, spec.C // 4
    cdiv = lambda a, b: -(-a // b)
    return {"copy": lambda: cdiv(n * HW * cq, 256), "nearest": lambda: cdiv(n * 4 * HW * cq, 256), "head": lambda: cdiv(n * HW, 256),
            "up2": lambda: cdiv(n * HW * cq, 256), "pw_nchw": lambda: n * cdiv(HW, PW_TILE), "pw_up": lambda: n * cdiv(HW, PW_TILE)}[spec.kind]()


def sub_ranges(spec):
    """Consecutive image ranges of a large case, each under the kernel's grid cap: a first one of two images (the one compared with the
    reference on the host), then as many images as the cap allows."""
    per = max(n for n in range(1, spec.N + 1) if natural_grid(spec, n) <= CAPS[spec.kind])
    edges = [0, 2]
    while edges[-1] < spec.N:
        edges.append(min(spec.N, edges[-1] + per))
    return list(zip(edges[:-1], edges[1:]))


# ------------------------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------------------------
def _cases():
    cs = []
    hw = lambda H, W: f"{H}x{W}"
    for Cc in (3, 24, 70):  # 32-channel x 64-pixel LDS tiles: channel tails 3 / 24 / 6, pixel tails 1 / 63 / 1 / 29
        for H, W in ((1, 1), (7, 9), (5, 13), (13, 17)):
            cs.append(KSpec("import", f"import-c{Cc}-{hw(H, W)}", 2, H, W, Cc))
    for Cc in (1, 32, 70):
        for H, W in ((1, 1), (8, 8), (5, 13), (13, 17)):
            cs.append(KSpec("export", f"export-c{Cc}-{hw(H, W)}", 2, H, W, Cc))
    for kind in ("copy", "nearest"):
        for Cc in (4, 68):
            for H, W in ((1, 1), (5, 7)):
                cs.append(KSpec(kind, f"{kind}-c{Cc}-{hw(H, W)}", 2, H, W, Cc))
    for Cc in (4, 64):  # 1 x 1, one row, one column: every clamp of the 3 x 3 neighbourhood active
        for H, W in ((1, 1), (1, 9), (9, 1), (5, 7)):
            cs.append(KSpec("up2", f"up2-c{Cc}-{hw(H, W)}", 2, H, W, Cc))
    for Cc in (4, 64, 68):
        for bias in (True, False):
            for exp in (False, True):
                cs.append(KSpec("head", f"head-c{Cc}-{'bias' if bias else 'nobias'}{'-exp' if exp else ''}", 2, 5, 7, Cc, bias=bias, exp=exp))
    for H, W in ((1, 1), (3, 5), (8, 8), (5, 13), (7, 10)):  # HW = 1, 15, 64, 65, 70 against tiles of 64 pixels / waves of 16
        for bias in (True, False):
            cs.append(KSpec("pw_nchw", f"pw_nchw-{hw(H, W)}-{'bias' if bias else 'nobias'}", 3, H, W, 64, bias=bias))
    for Cc in (64, 128):
        for H, W in ((2, 2), (2, 34), (6, 12)):  # 2 x 2: a 1 x 1 low map; 68 and 72 pixels: a second tile of 4 / 8 pixels
            for bias in (True, False):
                cs.append(KSpec("pw_up", f"pw_up-c{Cc}-{hw(H, W)}-{'bias' if bias else 'nobias'}", 2, H, W, Cc, bias=bias))
    for Cc in (4, 64):
        for H, W in ((25, 40), (32, 32), (25, 41)):  # HW = 1000, 1024, 1025 against chunks of 1024 pixels
            cs.append(KSpec("instnorm", f"instnorm-c{Cc}-{hw(H, W)}", 2, H, W, Cc))
    cs.append(KSpec("instnorm", "instnorm-c64-25x41-stats-only", 2, 25, 41, 64, out=False))
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = _cases()

# One per capped kernel: the natural grid exceeds the cap by less than a quarter, so that SOME workgroups take one more trip than the others
# (test_op_kinds_cpu.py::test_large_cases_cross_their_grid_cap_by_a_part holds these numbers against the caps above).
LARGE = [
    KSpec("copy", "copy-large", 272, 61, 67, 8, large=True),        # 1 111 664 pixels x 2 quads: 8685 workgroups
    KSpec("nearest", "nearest-large", 200, 31, 45, 8, large=True),  # 279 000 input pixels x 4 x 2 quads: 8719
    KSpec("head", "head-large", 516, 61, 67, 8, exp=True, large=True),  # 2 108 892 pixels: 8238
    KSpec("up2", "up2-large", 516, 61, 67, 16, large=True),         # 2 108 892 input pixels x 4 quads: 32 952; output 810 MB
    KSpec("pw_nchw", "pw_nchw-large", 6200, 7, 10, 64, large=True),  # 2 tiles per image (64 + 6 pixels): 12 400 = 3 x 4096 + 112
    KSpec("pw_up", "pw_up-large", 1100, 6, 12, 64, large=True),     # 2 tiles per image (64 + 8 pixels): 2200
]


def _imp(name, N, H, W, Cc):
    return KSpec("import", name, N, H, W, Cc)


# (name, members, group ids, launches)
IMPORT_GROUPS = [
    ("pyramid-of-five", [_imp(f"ig-pyr-{i}", 2, h, w, c) for i, (c, h, w) in enumerate(((24, 12, 16), (40, 6, 8), (64, 3, 4), (160, 2, 2), (256, 1, 1)))],
     [7] * 5, 1),
    ("nine-members", [_imp(f"ig-nine-{i}", 2, 3 + i, 5, 3 + 8 * i) for i in range(K_MAX_IMPORT + 1)], [7] * 9, 2),  # 8 + 1
    ("group-0", [_imp(f"ig-zero-{i}", 2, 3 + i, 5, 24) for i in range(3)], [0] * 3, 3),
    ("two-ids", [_imp(f"ig-ids-{i}", 2, 3 + i, 5, 24) for i in range(4)], [3, 3, 4, 4], 2),
    # 64 x 2 x 33 = 4224 blocks > 4096: the large member keeps its own grid, the small one in front of it runs alone
    ("large-member", [_imp("ig-large-a", 2, 5, 7, 24), _imp("ig-large-b", 33, 64, 64, 64)], [7, 7], 2),
]


# ------------------------------------------------------------------------------------------------------------------
# descriptors
# ------------------------------------------------------------------------------------------------------------------
def build_op(nhwc, spec, ptr, group=0, img0=0, n=None):
    """The idh_op of a spec for images [img0, img0 + n); ptr(name) -> device address of "x", "low", "w", "bias", "out", "exp", "ws"."""
    n = spec.N if n is None else n
    at = lambda name, c0=0: ptr(name) + 4 * (img0 * spec.image_floats(name) + c0)
    dense_at = lambda name: ptr(name) + 4 * (img0 + 1) * spec.image_floats(name)  # image 0 of the buffer stays prefilled
    k = spec.kind
    op = nhwc.Op()
    op.kind, op.N, op.group = KINDS[k][0], n, group
    s = op.src[0]
    s.in_, s.H, s.W, s.Cin = at("x", spec.in_c0), spec.H, spec.W, spec.C
    if k not in ("import", "pw_nchw"):
        s.cs = spec.in_cs
    Ho, Wo = spec.out_hw
    if k in DENSE_OUT:
        op.out = dense_at("out")
    elif spec.out:
        op.out, op.out_cs = at("out", OUT_C0), spec.out_cs
    if k in ("head", "pw_nchw", "pw_up"):
        s.w = ptr("w")
        op.bias = ptr("bias") if spec.bias else None
    if k == "head" and spec.exp:
        op.ws = dense_at("exp")
    if k in ("pw_nchw", "pw_up"):
        s.ks, s.stride = 1, 1
        op.Ho, op.Wo, op.Cout = Ho, Wo, spec.cout
    if k == "pw_up":
        lo = op.src[1]
        lo.in_, lo.cs, lo.H, lo.W, lo.Cin = at("low"), spec.low_cs, spec.H // 2, spec.W // 2, spec.C
    if k == "instnorm":
        op.ws, op.act, op.slope = ptr("ws"), ACT_LRELU, SLOPE
    return op


# ------------------------------------------------------------------------------------------------------------------
# tensors
# ------------------------------------------------------------------------------------------------------------------
def logical_tensors(spec, device="cpu"):
    """Seeded fp32 values of a case: "x" (NCHW for import / pointwise_nchw, NHWC otherwise), "low", OIHW-like "w" scaled for O(1) outputs, "bias"."""
    g = torch.Generator(device=device).manual_seed(zlib.crc32(spec.name.encode()))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32, device=device)
    N, H, W, Cc, k = spec.N, spec.H, spec.W, spec.C, spec.kind
    t = {"x": rn(N, Cc, H, W) if k in ("import", "pw_nchw") else rn(N, H, W, Cc)}
    if k == "instnorm":  # channels of different spread and offset (the statistics kernel's pivot has something to do)
        t["x"] = t["x"] * torch.linspace(0.5, 3.0, Cc) + torch.linspace(-2.0, 2.0, Cc)
    if k == "head":
        t["w"] = rn(Cc) / Cc ** 0.5
        t["bias"] = rn(1)
    if k in ("pw_nchw", "pw_up"):
        t["w"] = rn(spec.cout, Cc) / Cc ** 0.5
        t["bias"] = rn(spec.cout)
    if k == "pw_up":
        t["low"] = rn(N, H // 2, W // 2, Cc)
    if not spec.bias:
        t.pop("bias", None)
    return t


def _pad(x, cs, c0=0):
    """x as channels [c0, c0 + C) of a NaN-filled buffer of channel stride cs, on x's device."""
    if x.device.type == "cpu" and c0 == 0:
        return _padded(x, cs, float("nan"))
    buf = torch.full(x.shape[:3] + (cs,), float("nan"), dtype=torch.float32, device=x.device)
    buf[..., c0: c0 + x.shape[3]] = x
    return buf


def make_case(spec, device, group=0):
    """Device buffers + the nhwc.Op of a spec.  Large cases draw their values on the device (nothing large crosses to the host)."""
    from implicit_depth_amd import nhwc

    c = R.Case()
    c.spec, c.dev, c.cout = spec, {}, spec.cout
    c.t = t = logical_tensors(spec, device if spec.large else "cpu")
    dev, k = c.dev, spec.kind
    dev["x"] = (t["x"] if k in ("import", "pw_nchw") else _pad(t["x"], spec.in_cs, spec.in_c0)).to(device)
    if k == "pw_up":
        dev["low"] = _pad(t["low"], spec.low_cs).to(device)
    if k == "head":
        dev["w"] = t["w"].to(device)
    if k in ("pw_nchw", "pw_up"):
        conv = torch.nn.Conv2d(spec.C, spec.cout, 1, bias=False)
        conv.weight.data = t["w"].reshape(spec.cout, spec.C, 1, 1).clone()
        dev["w"] = nhwc.packed_weight(conv.to(device))
        torch.cuda.synchronize()
    if "bias" in t:
        dev["bias"] = t["bias"].to(device)
    Ho, Wo = spec.out_hw
    shape = (spec.N + 2, spec.cout, Ho, Wo) if k in DENSE_OUT else (spec.N, Ho, Wo, spec.out_cs)
    dev["out"] = torch.empty(shape, dtype=torch.int32, device=device)
    if spec.exp:
        dev["exp"] = torch.empty((spec.N + 2, 1, Ho, Wo), dtype=torch.int32, device=device)
    if k == "instnorm":  # as the header states: N * (ceil(HW / 1024) + 1) * 2 * C floats
        c.nchunks = -(-(spec.H * spec.W) // 1024)
        dev["ws"] = torch.empty(spec.N * (c.nchunks + 1) * 2 * spec.C, dtype=torch.float32, device=device)
    fill(c)
    c.op = build_op(nhwc, spec, lambda name: dev[name].data_ptr(), group)
    return c


def fill(case):
    prefill(case)  # "out" <- PREFILL, "ws" <- NaN
    if "exp" in case.dev:
        case.dev["exp"].fill_(PREFILL)


def split_output(case, key="out"):
    """(the written range as an int32 tensor ON THE BUFFER'S DEVICE, True when everything outside it still holds the prefill pattern)."""
    raw, spec = case.dev[key], case.spec
    if key == "exp" or spec.kind in DENSE_OUT:
        inside = raw[1: spec.N + 1]
        clean = bool((raw[0] == PREFILL).all()) and bool((raw[spec.N + 1] == PREFILL).all())
    else:
        inside = raw[..., OUT_C0: OUT_C0 + spec.cout]
        clean = bool((raw[..., :OUT_C0] == PREFILL).all()) and bool((raw[..., OUT_C0 + spec.cout:] == PREFILL).all())
    return inside, clean


def statistics(case):
    """(N, 2, C) mean / rstd an IDH_OP_INSTNORM left behind its chunk partials."""
    spec = case.spec
    return case.dev["ws"][spec.N * case.nchunks * 2 * spec.C:].view(spec.N, 2, spec.C)


# ------------------------------------------------------------------------------------------------------------------
# references and bounds
# ------------------------------------------------------------------------------------------------------------------
def _up2(x_nhwc):
    return F.interpolate(x_nhwc.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


def reference(spec, t):
    """(ref, B): the op's result in the output's layout - fp32 bits for the data-movement kinds, fp64 otherwise - and the magnitude the bound
    is relative to (None where unused).  pointwise_up: B = (B of the whole expression, up2(|low|))."""
    k, x = spec.kind, t["x"]
    if k == "import":
        return x.permute(0, 2, 3, 1).contiguous(), None
    if k == "export":
        return x.permute(0, 3, 1, 2).contiguous(), None
    if k == "copy":
        return x, None
    if k == "nearest":
        return x.repeat_interleave(2, 1).repeat_interleave(2, 2), None
    if k == "up2":
        ref, _, B = R.reference(R.UpSpec(spec.name, spec.N, spec.H, spec.W, spec.C), {"x0": x})
        return ref, B
    x = x.double()
    b = t["bias"].double() if "bias" in t else None
    if k == "head":
        w = t["w"].double()
        ref, B = (x * w).sum(-1), (x.abs() * w.abs()).sum(-1)
        if b is not None:
            ref, B = ref + b, B + b.abs()
        return ref[:, None], B[:, None]  # (N, 1, H, W)
    if k == "pw_nchw":
        w = t["w"].double()
        ref, B = torch.einsum("nchw,oc->nhwo", x, w), torch.einsum("nchw,oc->nhwo", x.abs(), w.abs())
        if b is not None:
            ref, B = ref + b, B + b.abs()
        return ref, B
    if k == "pw_up":
        w, low = t["w"].double(), t["low"].double()
        ref, B = torch.einsum("nhwc,oc->nhwo", x, w) + _up2(low), torch.einsum("nhwc,oc->nhwo", x.abs(), w.abs()) + _up2(low.abs())
        if b is not None:
            ref, B = ref + b, B + b.abs()
        return ref, (B, _up2(low.abs()))
    if k == "instnorm":
        return F.leaky_relu(F.instance_norm(x.permute(0, 3, 1, 2)), SLOPE).permute(0, 2, 3, 1), None
    raise KeyError(k)


INSTNORM_BAR = 1e-5  # of the output scale: the bar of tests/test_conv_gpu.py::test_instance_norm_every_accepted_width_and_block_size


def tolerance(spec, ref, B):
    """Elementwise bound of the arithmetic kinds (conv_op_ref.tolerance's model: K fused multiply-adds and S further additions err by at most
    (K + S + 4) u B in any order, twice that allowed, + u |ref| for the result's own rounding).
      up2:      8 u B + u |ref| - conv_op_ref.tolerance of an "up" spec
      head:     K = C, bias as the one further addition (folded into the + 4): 2 (C + 4) u B + u |ref|, B = sum |x| |w| + |bias|
      pw_nchw:  the direct family's formula with K = 64, S = 1: 2 (64 + 1 + 4) u B + u |ref|
      pw_up:    the same with K = C, B including up2(|low|), + 8 u up2(|low|) for the blend's own roundings"""
    k = spec.kind
    if k == "up2":
        return R.tolerance(R.UpSpec(spec.name, spec.N, spec.H, spec.W, spec.C), ref, B)
    if k == "head":
        return 2 * (spec.C + 4) * U * B + U * ref.abs()
    if k == "pw_nchw":
        return 2 * (64 + 1 + 4) * U * B + U * ref.abs()
    if k == "pw_up":
        B, Blow = B
        return 2 * (spec.C + 1 + 4) * U * B + U * ref.abs() + 8 * U * Blow
    raise KeyError(k)


def compose_fp32(spec, t):
    """head / pw_nchw / pw_up composed from fp32 torch ops (the reference's self-check), in the output's layout."""
    k, x = spec.kind, t["x"]
    if k == "head":
        y = F.conv2d(x.permute(0, 3, 1, 2), t["w"].reshape(1, spec.C, 1, 1), t.get("bias"))
        return y
    w = t["w"].reshape(spec.cout, spec.C, 1, 1)
    if k == "pw_nchw":
        return F.conv2d(x, w, t.get("bias")).permute(0, 2, 3, 1)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, t.get("bias")).permute(0, 2, 3, 1)
    return y + _up2(t["low"])


# ------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------
def _s(i, **kw):
    def f(op):
        for key, v in kw.items():
            setattr(op.src[i], key, v)
    return f


def _o(**kw):
    def f(op):
        for key, v in kw.items():
            setattr(op, key, v)
    return f


def _shift(get, set_, nbytes=4):
    """Moves a pointer off its 16-byte alignment."""
    return lambda op: set_(op, get(op) + nbytes)


def _both(*fs):
    def f(op):
        for g in fs:
            g(op)
    return f


def _refusals():
    """(name, spec, mutation of the built op, expected code): one mutation per validation rule of each case label of idh_run_ops; "NEW" in the
    name marks the rules this table was written together with (N / H / W / Cin > 0 and cs, out_cs >= channels for COPY, UPSAMPLE2_NEAREST,
    NHWC_TO_NCHW and POINTWISE_HEAD, H / W > 0 for INSTNORM).  The unmutated descriptor of every row is an accepted one."""
    base = {k: [c for c in CASES if c.kind == k and (k != "head" or c.exp) and c.bias and c.out and c.H * c.W > 1][-1] for k in KINDS}  # the widest of each kind
    rs = []
    add = lambda k, what, mut, code=EINVAL: rs.append((f"{k}-{what}", base[k], mut, code))
    bias_ptr = (lambda op: op.bias, lambda op, v: setattr(op, "bias", v))
    out_ptr = (lambda op: op.out, lambda op, v: setattr(op, "out", v))
    src_ptr = lambda i, f: (lambda op: getattr(op.src[i], f), lambda op, v: setattr(op.src[i], f, v))
    for k in KINDS:  # what every kind checks
        add(k, "null-in", _s(0, in_=None))
        if k != "instnorm":  # (out == NULL there: statistics only)
            add(k, "null-out", _o(out=None))
        new = "NEW-" if k in ("copy", "nearest", "export", "head", "instnorm") else ""
        add(k, ("NEW-" if k == "head" else "") + "n-zero", _o(N=0))
        add(k, ("NEW-" if k == "head" else "") + "n-negative", _o(N=-1))
        add(k, f"{new}h-zero", _both(_s(0, H=0), _s(1, H=0)))
        add(k, f"{new}w-zero", _both(_s(0, W=0), _s(1, W=0)))
    for k in ("import", "export", "instnorm"):  # the image index is blockIdx.z / .y
        add(k, "n-65536", _o(N=65536))
    for k in ("import", "export", "copy", "nearest", "up2", "head"):
        add(k, ("NEW-" if k not in ("import", "up2") else "") + "cin-zero", _s(0, Cin=0))
    for k in ("copy", "nearest", "up2", "head"):  # float4 accesses
        add(k, "cin-not-multiple-of-4", _s(0, Cin=base[k].C - 2))
        add(k, "cs-not-multiple-of-4", _s(0, cs=base[k].in_cs + 2))
    for k in ("copy", "nearest", "up2"):
        add(k, "out-cs-not-multiple-of-4", _o(out_cs=base[k].out_cs + 2))
    for k in ("copy", "nearest", "export", "head"):
        add(k, "NEW-cs-below-cin", _s(0, cs=base[k].C - 4))
    for k in ("copy", "nearest"):
        add(k, "NEW-out-cs-below-cin", _o(out_cs=base[k].C - 4))
    add("up2", "2^31-quads", _both(_o(N=1 << 15), _s(0, H=512, W=512)), EUNSUPPORTED)
    add("head", "null-w", _s(0, w=None))
    # IDH_OP_POINTWISE_NCHW
    k = "pw_nchw"
    add(k, "null-w", _s(0, w=None))
    add(k, "out-cs-not-multiple-of-4", _o(out_cs=138))
    add(k, "out-not-16-byte-aligned", _shift(*out_ptr))
    add(k, "bias-not-16-byte-aligned", _shift(*bias_ptr))
    add(k, "cin-32", _s(0, Cin=32), EUNSUPPORTED)
    add(k, "cout-64", _o(Cout=64), EUNSUPPORTED)
    add(k, "out-cs-below-cout", _o(out_cs=124), EUNSUPPORTED)
    add(k, "image-of-2^31-bytes", _s(0, H=2048, W=4096), EUNSUPPORTED)  # 2^23 pixels x 64 channels x 4 bytes
    # IDH_OP_POINTWISE_UP
    k, Cc = "pw_up", base["pw_up"].C
    add(k, "null-w", _s(0, w=None))
    add(k, "null-low", _s(1, in_=None))
    add(k, "h-odd", _s(0, H=base[k].H + 1))
    add(k, "w-odd", _s(0, W=base[k].W + 1))
    add(k, "cs-not-multiple-of-4", _s(0, cs=base[k].in_cs + 2))
    add(k, "low-cs-not-multiple-of-4", _s(1, cs=base[k].low_cs + 2))
    add(k, "out-cs-not-multiple-of-4", _o(out_cs=base[k].out_cs + 2))
    add(k, "cs-below-cin", _s(0, cs=Cc - 4))
    add(k, "low-cs-below-cout", _s(1, cs=Cc - 4))
    add(k, "out-cs-below-cout", _o(out_cs=Cc - 4))
    add(k, "in-not-16-byte-aligned", _shift(*src_ptr(0, "in_")))
    add(k, "low-not-16-byte-aligned", _shift(*src_ptr(1, "in_")))
    add(k, "w-not-16-byte-aligned", _shift(*src_ptr(0, "w")))
    add(k, "out-not-16-byte-aligned", _shift(*out_ptr))
    add(k, "bias-not-16-byte-aligned", _shift(*bias_ptr))
    add(k, "low-h-is-not-half", _s(1, H=base[k].H // 2 + 1))
    add(k, "low-w-is-not-half", _s(1, W=base[k].W // 2 + 1))
    add(k, "cin-differs-from-cout", _both(_s(0, Cin=128 if Cc == 64 else 64, cs=3 * 128)), EUNSUPPORTED)
    add(k, "cin-32", _both(_s(0, Cin=32), _o(Cout=32)), EUNSUPPORTED)
    add(k, "2^31-pixels", _both(_s(0, H=1 << 16, W=1 << 15), _s(1, H=1 << 15, W=1 << 14)), EUNSUPPORTED)
    # IDH_OP_INSTNORM
    k = "instnorm"
    add(k, "null-ws", _o(ws=None))
    add(k, "cin-zero", _s(0, Cin=0))
    add(k, "cin-not-multiple-of-4", _s(0, Cin=base[k].C - 2))
    add(k, "cin-quads-do-not-divide-256", _s(0, Cin=20, cs=24))  # 256 % 5
    add(k, "cs-not-multiple-of-4", _s(0, cs=base[k].in_cs + 2))
    add(k, "out-cs-not-multiple-of-4", _o(out_cs=base[k].out_cs + 2))
    assert len({r[0] for r in rs}) == len(rs)
    return rs


REFUSALS = _refusals()


def declared_kinds():
    """{name: code} of the IDH_OP_* enumerators of include/idh_ops.h."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "idh_ops.h")
    with open(path) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*IDH_OP_(\w+)\s*=\s*(\d+)", f.read(), re.M)}
