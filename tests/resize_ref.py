"""A NumPy restatement of the frame resize's value rule (include/sage_gs.h, sgs_resize): both filters, both formats.
It imports nothing of the product.  test_resize_ref.py holds it to PIL.Image.resize bit for bit (bicubic) before anything else uses it.

Bicubic is Pillow's separable convolution resampling: fp64 coefficients (Python floats: every multiply and add rounded on its own),
22-bit fixed-point weights and 8-bit levels between the passes for uint8, fp64 sums and an fp32 intermediate for float; a pass whose
in-size equals its out-size is skipped.  Linear is bilinear at half-pixel centres in exact integer arithmetic (uint8) or in fp32 /
fp64 lerps (float)."""
from __future__ import annotations

import numpy as np

BITS = 22


def levels(frame):
    """uint8 levels of an fp32 frame as sgs_pack_rgba8 writes them, unfused: clamp to [0, 1], (unsigned)(x * 255 + 0.5) in fp32."""
    c = np.clip(np.asarray(frame, np.float32), np.float32(0), np.float32(1))
    return (c * np.float32(255) + np.float32(0.5)).astype(np.uint32).astype(np.uint8)


def unlevel(k):
    """The fp32 nearest k / 255 of every level."""
    return np.asarray(k).astype(np.float32) / np.float32(255)


def clip(d, bounds):
    """x < lo ? lo : (x > hi ? hi : x): NaN stays NaN."""
    d = np.asarray(d, np.float32)
    if bounds is None:
        return d
    lo, hi = np.float32(bounds[0]), np.float32(bounds[1])
    return np.where(d < lo, lo, np.where(d > hi, hi, d)).astype(np.float32)


def cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def coeffs(in_size, out_size, normalise=True):
    """[(first tap, [weights])] per output sample of an axis."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    out = []
    for o in range(out_size):
        c = (o + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), in_size)
        k = [cubic((j + lo - c + 0.5) * ss) for j in range(hi - lo)]
        ww = 0.0
        for v in k:
            ww = ww + v
        if normalise and ww != 0.0:
            k = [v / ww for v in k]
        out.append((lo, k))
    return out


def fixed(k):
    return [int(v * (1 << BITS) + (0.5 if v >= 0 else -0.5)) for v in k]


def _pass_u8(a, out_size, axis):
    """(levels, unclamped values) of one pass along `axis`."""
    a = np.moveaxis(np.asarray(a), axis, 0).astype(np.int64)
    raw = np.empty((out_size,) + a.shape[1:], np.int64)
    for o, (lo, k) in enumerate(coeffs(a.shape[0], out_size)):
        s = np.full(a.shape[1:], 1 << (BITS - 1), np.int64)
        for j, w in enumerate(fixed(k)):
            s = s + a[lo + j] * w
        raw[o] = s >> BITS
    return np.moveaxis(np.clip(raw, 0, 255).astype(np.uint8), 0, axis), np.moveaxis(raw, 0, axis)


def _pass_f32(a, out_size, axis):
    a = np.moveaxis(np.asarray(a, np.float32), axis, 0).astype(np.float64)
    out = np.empty((out_size,) + a.shape[1:], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for o, (lo, k) in enumerate(coeffs(a.shape[0], out_size)):
            s = np.zeros(a.shape[1:], np.float64)
            for j, w in enumerate(k):
                s = s + a[lo + j] * w
            out[o] = s.astype(np.float32)
    return np.moveaxis(out, 0, axis)


def bicubic_u8(lv, w, h, with_range=False):
    """uint8 [H,W(,C)] levels -> [h,w(,C)]; with_range: also (least, greatest) value before the clamp over both passes."""
    lv = np.asarray(lv, np.uint8)
    lo, hi = 0, 255
    if lv.shape[1] != w:
        lv, raw = _pass_u8(lv, w, 1)
        lo, hi = min(lo, int(raw.min())), max(hi, int(raw.max()))
    if lv.shape[0] != h:
        lv, raw = _pass_u8(lv, h, 0)
        lo, hi = min(lo, int(raw.min())), max(hi, int(raw.max()))
    return (lv, (lo, hi)) if with_range else lv


def bicubic_f32(d, w, h, bounds=None):
    d = clip(d, bounds)
    if d.shape[1] != w:
        d = _pass_f32(d, w, 1)
    if d.shape[0] != h:
        d = _pass_f32(d, h, 0)
    return d


def linear_taps(in_size, out_size):
    """(first index, second index, numerator of the second's weight over 2 * out_size) per output sample."""
    o = np.arange(out_size, dtype=np.int64)
    s = np.maximum((2 * o + 1) * in_size - out_size, 0)
    i0, f = s // (2 * out_size), s % (2 * out_size)
    last = i0 >= in_size - 1
    i0 = np.where(last, in_size - 1, i0)
    f = np.where(last, 0, f)
    i1 = np.where(last, i0, i0 + 1)
    return i0, i1, f


def linear_u8(lv, w, h):
    lv = np.asarray(lv, np.uint8).astype(np.int64)
    H, W = lv.shape[:2]
    x0, x1, fx = linear_taps(W, w)
    y0, y1, fy = linear_taps(H, h)
    tail = (1,) * (lv.ndim - 2)
    fx = fx.reshape((1, w) + tail); fy = fy.reshape((h, 1) + tail)
    a, b, c, d = lv[y0][:, x0], lv[y0][:, x1], lv[y1][:, x0], lv[y1][:, x1]
    s = a * (2 * w - fx) * (2 * h - fy) + b * fx * (2 * h - fy) + c * (2 * w - fx) * fy + d * fx * fy
    return ((s + 2 * w * h) // (4 * w * h)).astype(np.uint8)


def linear_f(d, w, h, bounds=None, dtype=np.float32):
    """Horizontal lerps a + (b - a) fx / 2w on both rows, then the vertical one, in `dtype` (fp64: the value the fp32 result is held to)."""
    d = clip(d, bounds).astype(dtype)
    H, W = d.shape
    x0, x1, fx = linear_taps(W, w)
    y0, y1, fy = linear_taps(H, h)
    tx = (fx.astype(dtype) / dtype(2 * w))[None, :]
    ty = (fy.astype(dtype) / dtype(2 * h))[:, None]
    with np.errstate(invalid="ignore"):
        a, b, c, e = d[y0][:, x0], d[y0][:, x1], d[y1][:, x0], d[y1][:, x1]
        top = a + (b - a) * tx
        bot = c + (e - c) * tx
        return (top + (bot - top) * ty).astype(dtype)


def resize_rgb8(frame, w, h, filter="bicubic", lv=None):
    """(fp32 [h,w,3] frame on k / 255, its uint8 levels) of an fp32 [H,W,3] frame; lv: the frame's levels where the build's differ."""
    lv = levels(frame) if lv is None else lv
    out = bicubic_u8(lv, w, h) if filter == "bicubic" else linear_u8(lv, w, h)
    return unlevel(out), out


def resize_f32(d, w, h, filter="bicubic", bounds=None):
    return bicubic_f32(d, w, h, bounds) if filter == "bicubic" else linear_f(d, w, h, bounds)
