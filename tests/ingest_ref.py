"""numpy restatement of the frame loader the native ingest replaces (implicit_depth_amd/ingest.py, csrc/ingest.hip): Pillow's 8-bit
``Image.resize`` for BILINEAR / BICUBIC, ``to_tensor`` + ImageNet normalisation, the NEAREST depth resize with its validity masks, and
the intrinsics pyramid.  Written from the rules, not from any source: tests/golden/gen_golden_ingest.py checks it against Pillow and
torch on the CPU and tests/test_ingest_cpu.py against the goldens.

Resize, per dimension (C doubles): ``scale = in / out``, ``filterscale = max(scale, 1)``, ``support = S * filterscale`` (S = 1 bilinear,
2 bicubic with a = -0.5), ``ksize = 2 * ceil(support) + 1``.  Output index ``i``: ``center = (i + 0.5) * scale``,
``xmin = max(int(center - support + 0.5), 0)``, ``n = min(int(center + support + 0.5), in) - xmin``, taps
``filter((k + xmin - center + 0.5) / filterscale)`` divided by their sum, then ``int(+-0.5 + tap * 2**22)``.  A pass accumulates in integers
from ``1 << 21``, shifts right by 22 and clips to 0..255; horizontal first, the intermediate image is uint8, a pass whose dimension does
not change is skipped."""
import math

import numpy as np

BILINEAR, BICUBIC = 0, 1
PRECISION_BITS = 22
MEAN = np.array((0.485, 0.456, 0.406), dtype=np.float32)
STD = np.array((0.229, 0.224, 0.225), dtype=np.float32)


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTERS = {BILINEAR: (_bilinear, 1.0), BICUBIC: (_bicubic, 2.0)}


def ksize(n_in, n_out, filt):
    scale = n_in / n_out
    return int(math.ceil(_FILTERS[filt][1] * max(scale, 1.0))) * 2 + 1


def coeffs(n_in, n_out, filt):
    """(bounds (n_out,2) int32 [first source index, tap count], taps (n_out,ksize) int32 fixed point, zero past the count)."""
    f, s = _FILTERS[filt]
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = s * filterscale
    ks = ksize(n_in, n_out, filt)
    bounds = np.zeros((n_out, 2), np.int32)
    taps = np.zeros((n_out, ks), np.int32)
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [f((k + xmin - center + 0.5) / filterscale) for k in range(n)]
        tot = 0.0
        for v in w:
            tot += v
        if tot != 0.0:
            w = [v / tot for v in w]
        bounds[i] = (xmin, n)
        for k, v in enumerate(w):
            taps[i, k] = int((-0.5 if v < 0 else 0.5) + v * (1 << PRECISION_BITS))
    return bounds, taps


def _pass(img, bounds, taps, axis, wide=False):
    """One pass over ``axis`` of an (H,W,C) image."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.int64)
    for i, (x0, n) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for k in range(n):
            acc = acc + src[x0 + k] * int(taps[i, k])
        out[i] = acc >> PRECISION_BITS
    if wide:
        return np.moveaxis(out, 0, axis)
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize_u8(img_hwc, size, filt):
    """Pillow's ``Image.resize((w, h), resample)`` of a uint8 (H,W,C) image."""
    h, w = size
    out = img_hwc
    if w != img_hwc.shape[1]:
        out = _pass(out, *coeffs(img_hwc.shape[1], w, filt), axis=1)
    if h != img_hwc.shape[0]:
        out = _pass(out, *coeffs(img_hwc.shape[0], h, filt), axis=0)
    return out


def resize_u8_wide_intermediate(img_hwc, size, filt):
    """What a resize would give if the first pass were NOT rounded and clipped to uint8 (its result kept as the shifted integer sum):
    the defect tests/test_ingest_gpu.py must be able to see."""
    h, w = size
    out = img_hwc
    if w != img_hwc.shape[1]:
        out = _pass(out, *coeffs(img_hwc.shape[1], w, filt), axis=1, wide=True)
    if h != img_hwc.shape[0]:
        out = _pass(out, *coeffs(img_hwc.shape[0], h, filt), axis=0)
    return np.clip(out, 0, 255).astype(np.uint8)


def to_tensor(img_hwc_u8):
    """(C,H,W) float32: ``u8.float().div(255)``."""
    return np.ascontiguousarray(np.moveaxis(img_hwc_u8, 2, 0)).astype(np.float32) / np.float32(255)


def normalize(t_chw):
    """``.sub_(mean).div_(std)`` with float32 ImageNet statistics."""
    return (t_chw - MEAN[:, None, None]) / STD[:, None, None]


def load_color(frames_bhwc, size, filt, normalise=True):
    """((B,3,h,w) float32, (B,h,w,3) uint8) of uint8 (B,H,W,3) frames."""
    u8 = np.stack([resize_u8(f, size, filt) for f in frames_bhwc])
    t = np.stack([normalize(to_tensor(f)) if normalise else to_tensor(f) for f in u8])
    return t, u8


def nearest_index(n_in, n_out):
    """Source index of every output index for NEAREST: ``int((i + 0.5) * step)`` with ``step = in / out`` rounded to a double FIRST
    (``(i + 0.5) * in / out`` differs from Pillow at some sizes, e.g. 2 -> 7)."""
    step = n_in / n_out
    return np.minimum(((np.arange(n_out) + 0.5) * step).astype(np.int32), n_in - 1)


def load_depth(depth_bhw_u16, size=None, value_scale=1e-3, min_valid=1e-3, max_valid=10.0):
    """(depth (B,1,h,w) float32 with NaN where invalid, float mask, bool mask) of uint16 (B,H,W) millimetres."""
    d = depth_bhw_u16
    if size is not None and tuple(size) != d.shape[1:]:
        d = d[:, nearest_index(d.shape[1], size[0])][:, :, nearest_index(d.shape[2], size[1])]
    depth = d.astype(np.float32)[:, None] * np.float32(value_scale)
    mask_b = (depth > np.float32(min_valid)) & (depth < np.float32(max_valid))
    depth = np.where(mask_b, depth, np.float32(np.nan)).astype(np.float32)
    return depth, mask_b.astype(np.float32), mask_b


def intrinsics_pyramid(K_b44, native_size, depth_size, include_full_depth_K=False):
    """dict of float32 (B,4,4): K scaled to the depth resolution, halved per level 0..4, and the inverses."""
    K = np.array(K_b44, dtype=np.float32, copy=True).reshape(-1, 4, 4)
    out = {}
    if include_full_depth_K:
        out["K_full_depth_b44"] = K.copy()
        out["invK_full_depth_b44"] = np.stack([np.linalg.inv(k) for k in K])
    (H, W), (dh, dw) = native_size, depth_size
    K[:, 0] *= np.float32(dw / float(W))
    K[:, 1] *= np.float32(dh / float(H))
    for i in range(5):
        Ks = K.copy()
        Ks[:, :2] /= np.float32(2 ** i)
        out[f"K_s{i}_b44"] = Ks
        out[f"invK_s{i}_b44"] = np.stack([np.linalg.inv(k) for k in Ks])
    return out


# ---- the cases of tests/golden/g_ingest.npz (tests/golden/gen_golden_ingest.py writes them, the CPU and GPU tests read them) ------------
COLOR_CASES = [  # (name, source (H,W), target (h,w)); B = 3 seeded frames each, both filters
    ("down", (37, 53), (24, 32)),
    ("up", (30, 41), (45, 50)),          # upscale both ways
    ("ratio57", (97, 131), (19, 23)),    # ratio about 5.7: 25 bicubic taps, fewer at the borders
    ("skip_v", (20, 20), (20, 31)),      # vertical pass skipped
    ("skip_h", (20, 31), (9, 31)),       # horizontal pass skipped
    ("same", (24, 32), (24, 32)),        # no resize
    ("ragged", (75, 100), (33, 65)),     # targets that are no multiple of a tile
    ("cap8", (64, 64), (8, 8)),          # ratio exactly 8
    ("checker", (37, 53), (24, 32)),     # 0/255 checkerboard: both clip ends after each pass
    ("stripes", (37, 53), (24, 32)),     # one-pixel stripes
]
FILTER_NAMES = {"bilinear": BILINEAR, "bicubic": BICUBIC}
DEPTH_CASES = [("d_down", (37, 53), (24, 32)), ("d_half", (48, 64), (24, 32)), ("d_full", (37, 53), None)]
DEPTH_SPECIALS = (0, 1, 9999, 10000, 65535)
# the case whose result changes when the first pass is kept wider than uint8 (checked on the CPU in tests/test_ingest_cpu.py)
WIDE_INTERMEDIATE_CASE = ("checker", "bicubic")


def color_input(name, shape, seed):
    """(3,H,W,3) uint8: three different frames."""
    H, W = shape
    rng = np.random.default_rng(seed)
    if name == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        base = (((yy + xx) & 1) * 255).astype(np.uint8)
        f = np.stack([base, 255 - base, np.where(rng.random((H, W)) < 0.1, 255 - base, base)])
        return np.ascontiguousarray(np.stack([f, np.roll(f, 1, axis=2), 255 - f], axis=-1))
    if name == "stripes":
        xx = np.broadcast_to(np.arange(W)[None, :], (H, W))
        yy = np.broadcast_to(np.arange(H)[:, None], (H, W))
        # lines one pixel wide on a flat ground (and, as 255 - f, the inverse): the bicubic lobes undershoot beside a bright line
        f = np.stack([((xx % 7) == 3) * 255, ((yy % 7) == 3) * 255, (((xx % 7) == 3) | ((yy % 5) == 2)) * 255]).astype(np.uint8)
        return np.ascontiguousarray(np.stack([f, 255 - f, np.roll(f, 1, axis=1)], axis=-1))
    return rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)


def depth_input(shape, seed):
    """(2,H,W) uint16 millimetres with the special values planted."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 12000, (2,) + tuple(shape)).astype(np.uint16)
    flat = d.reshape(2, -1)
    pos = rng.permutation(flat.shape[1])[: 12 * len(DEPTH_SPECIALS)]
    for i, p in enumerate(pos):
        flat[:, p] = DEPTH_SPECIALS[i % len(DEPTH_SPECIALS)]
    return d
