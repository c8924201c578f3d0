"""CPU restatement of the AR compositing path (include/idh_composite.h) in numpy, written from its stated semantics:
the hole filling and nearest resize of the asset's depth render, and the resize / get_mask / valid-pixel / fade / blend / truncate
chain, with numpy's dtypes statement by statement.  The GPU tests compare the kernels against it on seeds the golden file does not
hold; tests/test_composite_cpu.py checks it against the reference's own code (tests/golden/g16_composite.npz).

Nothing here calls torch's interpolate or pooling: the resize is the half-pixel-centre arithmetic written out in float32, with the
FMAs of torch's CPU kernel emulated in extended precision."""
import numpy as np

BAND = 0.2           # DEPTH_ALPHA_BAND_SIZE, metres
FADE_IN_FRAMES = 45
COLOUR = (0.30, 0.9, 0.78)

f32 = np.float32


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def nearest_index(out: int, size: int) -> np.ndarray:
    """src = min(floor(dst * in / out), in - 1) with the float32 scale of PyTorch's legacy "nearest"."""
    scale = f32(size) / f32(out)
    return np.minimum(np.floor(np.arange(out, dtype=f32) * scale).astype(np.int64), size - 1)


def prepare_rendered_depth(render_b1HW, size):
    """Pixels that are exactly 0 take the maximum of the in-bounds part of their 7x7 neighbourhood; then nearest resize to ``size``."""
    x = _np(render_b1HW).astype(f32)
    B, _, Hr, Wr = x.shape
    pad = np.full((B, 1, Hr + 6, Wr + 6), -np.inf, f32)
    pad[:, :, 3:-3, 3:-3] = x
    pooled = np.full_like(x, -np.inf)
    for dy in range(7):
        for dx in range(7):
            pooled = np.maximum(pooled, pad[:, :, dy: dy + Hr, dx: dx + Wr])
    filled = np.where(x == 0, pooled, x)
    iy, ix = nearest_index(size[0], Hr), nearest_index(size[1], Wr)
    return filled[:, :, iy[:, None], ix[None, :]]


LD = np.longdouble  # 64-bit mantissa: a float32 product is exact in it, so rounding a * b + c once more to float32 is an FMA
assert np.finfo(LD).nmant >= 63, "composite_ref emulates float32 FMAs in x87 extended precision; this host's longdouble is narrower"


def _fma(a, b, c):
    return (np.asarray(a, f32).astype(LD) * np.asarray(b, f32).astype(LD) + np.asarray(c, f32).astype(LD)).astype(f32)


def _linear(out: int, size: int):
    scale = f32(size) / f32(out)
    src = np.maximum(_fma(scale, np.arange(out, dtype=f32) + f32(0.5), f32(-0.5)), f32(0))  # one FMA, as torch's CPU kernel
    i0 = np.minimum(np.floor(src).astype(np.int64), size - 1)
    l1 = np.clip(src - i0.astype(f32), f32(0), f32(1)).astype(f32)
    i1 = i0 + (i0 < size - 1)
    return i0, i1, f32(1) - l1, l1


def resize_bilinear(m_bhw, H: int, W: int) -> np.ndarray:
    """Bilinear, half-pixel centres, align_corners=False, no antialiasing, float32, rounded as torch's CPU upsample_bilinear2d rounds a contiguous
    one-channel map.  torch picks between two CPU kernels by the output size: H + W <= 128 takes the vectorised one (the
    four weight products, v01 first and the other taps accumulated by FMA), anything larger the generic one (row-wise, fma(ly0, top,
    ly1 * bot) with top / bot = fma(lx0, v0, lx1 * v1)).  tests/test_composite_cpu.py checks this function against F.interpolate on shapes
    either side of the rule.  A map of size (H, W) is returned as it is."""
    m = _np(m_bhw).astype(f32)
    if m.shape[-2:] == (H, W):
        return m
    y0, y1, ly0, ly1 = _linear(H, m.shape[-2])
    x0, x1, lx0, lx1 = _linear(W, m.shape[-1])
    Y0, Y1, X0, X1 = y0[:, None], y1[:, None], x0[None, :], x1[None, :]
    LY0, LY1, LX0, LX1 = ly0[:, None], ly1[:, None], lx0[None, :], lx1[None, :]
    v00, v01, v10, v11 = m[..., Y0, X0], m[..., Y0, X1], m[..., Y1, X0], m[..., Y1, X1]
    if H + W <= 128:
        acc = ((LY0 * LX1).astype(f32) * v01).astype(f32)
        acc = _fma((LY0 * LX0).astype(f32), v00, acc)
        acc = _fma((LY1 * LX0).astype(f32), v10, acc)
        return _fma((LY1 * LX1).astype(f32), v11, acc)
    top = _fma(LX0, v00, (LX1 * v01).astype(f32))
    bot = _fma(LX0, v10, (LX1 * v11).astype(f32))
    return _fma(LY0, top, (LY1 * bot).astype(f32))


def sigmoid_custom(x, multiplier=1.0):
    """1 / (1 + exp(-m x)) in float32.  torch's exp, not numpy's: the two differ by an ulp on some inputs, and the golden frames were made
    with torch's (a 1-ulp change of a probability can move a blend across an integer)."""
    import torch

    x = torch.from_numpy(np.ascontiguousarray(_np(x), dtype=f32))
    return (1 / (1 + torch.exp(-multiplier * x))).numpy()


def get_mask(predicted, virtual, soft: bool):
    """Dtype follows the operands: float32 against a float32 map, float64 against a float64 plane."""
    if soft:
        half = (predicted - virtual) + (f32(BAND / 2) if virtual.dtype == f32 else BAND / 2)
        return np.clip((f32(1 / BAND) if half.dtype == f32 else 1 / BAND) * half, 0.0, 1.0)
    return (predicted > virtual).astype(f32)


def composite(image_u8, *, occlusion=None, logits=True, multiplier=1.0, depth=None, virtual_depth=None, soft=True, virtual_rgba=None,
              colour=COLOUR, fade=None, bgr=False, prob_shift=0.0):
    """(frame uint8 (B,H,W,3), matte float32 (B,H,W)).  ``occlusion`` (B,1,h,w) logits or probabilities, or ``depth`` (B,1,h,w) with
    ``virtual_depth`` a (B,H,W) map or a float plane distance.  ``fade`` None or one value per frame.  ``prob_shift`` is added to the
    resized probability (the ambiguity margin of the logits cases)."""
    if (occlusion is None) == (depth is None):
        raise ValueError("exactly one of occlusion and depth")
    im8 = _np(image_u8)
    B, H, W, _ = im8.shape
    im = im8 / 255.0  # float64
    fades = [None] * B if fade is None else [float(f) for f in _np(fade).reshape(-1)]
    frames, mattes = [], []
    for b in range(B):
        if virtual_rgba is not None:
            rgba = _np(virtual_rgba)[b].astype(f32) / f32(255.0)
            vrgb, valid = rgba[:, :, :3], rgba[:, :, 3]
        else:
            vrgb = np.zeros((H, W, 3)) + np.asarray(colour, np.float64)
            valid = np.ones((H, W))
        if fades[b] is not None:
            valid = valid * (f32(fades[b]) if valid.dtype == f32 else fades[b])
        if occlusion is not None:
            p = sigmoid_custom(_np(occlusion)[b, 0], multiplier) if logits else _np(occlusion)[b, 0].astype(f32)
            up = resize_bilinear(p, H, W)
            if prob_shift:
                up = (up + f32(prob_shift)).astype(f32)
            matte = f32(1) - up * valid.astype(f32)
        else:
            d = resize_bilinear(_np(depth)[b, 0], H, W)
            if isinstance(virtual_depth, (int, float)):
                matte = 1.0 - get_mask(d, np.ones((H, W)) * float(virtual_depth), soft)
            else:
                vd = _np(virtual_depth)[b].astype(f32)
                valid = (vd > 0).astype(f32)
                if fades[b] is not None:
                    valid = valid * f32(fades[b])
                matte = f32(1) - get_mask(d, vd, soft) * valid
        matte = matte[:, :, None].astype(f32)
        comp = matte * im[b] + (1 - matte) * vrgb  # float64 sum; the second product is float32 with a render
        out = (comp * 255.0).astype(np.uint8)
        frames.append(out[:, :, ::-1] if bgr else out)
        mattes.append(matte[:, :, 0])
    return np.stack(frames), np.stack(mattes)
