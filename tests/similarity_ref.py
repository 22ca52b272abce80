"""NumPy restatement of the image similarity (sgs_image_similarity, include/sage_gs.h): int64 moments by shifted slices, the four
int64 terms, one fp64 quotient per window, floor to 30 fractional bits.  Held to a Python-integer loop written from the definition by
test_similarity_ref.py; the kernels (csrc/sgs_similarity.h) are held to it, every field exactly."""
from __future__ import annotations

import math

import numpy as np

TAPS = (2, 16, 74, 224, 436, 544, 436, 224, 74, 16, 2)
WINDOW = len(TAPS)
T_BITS = 22
T = 1 << T_BITS
C1, C2 = 114393189753815, 1029538707784335
Q_BITS = 30
ONE = 1 << Q_BITS
ROW_DTYPE = np.dtype([("ssim_q", "<i8", (3,)), ("sse", "<u8", (3,)), ("n_windows", "<u8"), ("n_pixels", "<u8")])
FIELDS = ("ssim_q", "sse", "n_windows", "n_pixels")
assert sum(TAPS) == 2048 and sum(TAPS) ** 2 == T and ROW_DTYPE.itemsize == 64
assert C1 == round((0.01 * 255) ** 2 * 2 ** 44) and C2 == round((0.03 * 255) ** 2 * 2 ** 44)


def levels(rgb_f32):
    """The 8-bit levels k_pack_rgba8 makes of an fp32 frame, every step in fp32, unfused."""
    x = np.clip(np.asarray(rgb_f32, np.float32), np.float32(0), np.float32(1))
    return (x * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def _window_sums(v):
    """int64 [H,W] -> [H-10,W-10]: sum over the 11 x 11 window at every origin of w[j] w[i] v."""
    H, W = v.shape
    h = np.zeros((H, W - WINDOW + 1), np.int64)
    for i, w in enumerate(TAPS):
        h += w * v[:, i:i + W - WINDOW + 1]
    out = np.zeros((H - WINDOW + 1, W - WINDOW + 1), np.int64)
    for j, w in enumerate(TAPS):
        out += w * h[j:j + H - WINDOW + 1]
    return out


def window_q(x, y):
    """q of every window of one channel: x, y integer levels [H,W] -> int64 [H-10,W-10]."""
    x, y = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    A, B = _window_sums(x), _window_sums(y)
    Cxx, Cyy, Cxy = _window_sums(x * x), _window_sums(y * y), _window_sums(x * y)
    n1 = 2 * A * B + C1
    d1 = A * A + B * B + C1
    n2 = 2 * (T * Cxy - A * B) + C2
    d2 = (T * Cxx - A * A) + (T * Cyy - B * B) + C2
    assert (d1 > 0).all() and (d2 > 0).all() and int(np.abs(n2).max()) < 2 ** 62 and int(d2.max()) < 2 ** 62
    s = (n1.astype(np.float64) * n2.astype(np.float64)) / (d1.astype(np.float64) * d2.astype(np.float64))
    return np.floor(s * float(ONE) + 0.5).astype(np.int64)


def row(x_levels, y_levels):
    """One frame's sgs_similarity_row: x_levels, y_levels uint8 [H,W,3]."""
    x, y = np.asarray(x_levels), np.asarray(y_levels)
    assert x.shape == y.shape and x.ndim == 3 and x.shape[2] == 3 and min(x.shape[:2]) >= WINDOW
    H, W = x.shape[:2]
    r = np.zeros((), ROW_DTYPE)
    for c in range(3):
        r["ssim_q"][c] = window_q(x[..., c], y[..., c]).sum()
        d = x[..., c].astype(np.int64) - y[..., c].astype(np.int64)
        r["sse"][c] = (d * d).sum()
    r["n_windows"] = (H - WINDOW + 1) * (W - WINDOW + 1)
    r["n_pixels"] = H * W
    return r


def score(r):
    """sum_c ssim_q[c] / (3 n_windows 2^30)."""
    return float(int(np.asarray(r["ssim_q"]).sum())) / (3.0 * float(r["n_windows"]) * ONE)


def first_difference(got, want):
    """(field, got, want) of the first field in which two rows differ, or None."""
    for n in FIELDS:
        if not np.array_equal(got[n], want[n]):
            return n, np.asarray(got[n]).tolist(), np.asarray(want[n]).tolist()
    return None


# ---- the definition once more, window by window, in Python integers (small frames only) --------------------------------------------------
def q_loop(x, y):
    """[H,W] levels -> list of rows of q, from the definition's text alone."""
    H, W = len(x), len(x[0])
    out = []
    for oy in range(H - 10):
        line = []
        for ox in range(W - 10):
            A = B = Cxx = Cyy = Cxy = 0
            for j in range(11):
                for i in range(11):
                    w = TAPS[j] * TAPS[i]
                    a, b = int(x[oy + j][ox + i]), int(y[oy + j][ox + i])
                    A += w * a; B += w * b; Cxx += w * a * a; Cyy += w * b * b; Cxy += w * a * b
            n1 = 2 * A * B + C1
            d1 = A * A + B * B + C1
            n2 = 2 * (T * Cxy - A * B) + C2
            d2 = (T * Cxx - A * A) + (T * Cyy - B * B) + C2
            assert 0 < d1 < 2 ** 63 and 0 < d2 < 2 ** 63 and abs(n1) < 2 ** 63 and abs(n2) < 2 ** 63
            s = (float(n1) * float(n2)) / (float(d1) * float(d2))
            line.append(math.floor(s * 1073741824.0 + 0.5))
        out.append(line)
    return out


# ---- Wang et al.'s SSIM with the float Gaussian, fp64 (the one tolerance of this feature is measured against it) -----------------------
def ssim_float(x_levels, y_levels):
    """Mean SSIM over the valid 11 x 11 windows and the three channels: Gaussian of sigma 1.5 normalised to 1, K1 = 0.01, K2 = 0.03,
    L = 255, weighted (biased) variances — Wang, Bovik, Sheikh, Simoncelli 2004."""
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2

    def blur(v):
        H, W = v.shape
        h = sum(g[i] * v[:, i:i + W - 10] for i in range(11))
        return sum(g[j] * h[j:j + H - 10] for j in range(11))

    total = 0.0
    for c in range(3):
        x, y = np.asarray(x_levels)[..., c].astype(np.float64), np.asarray(y_levels)[..., c].astype(np.float64)
        mx, my = blur(x), blur(y)
        vx, vy, cxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
        total += (((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))).mean()
    return total / 3.0
