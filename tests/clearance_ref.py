"""A NumPy restatement of the clearance map (sgs_clearance_map, sgs_clearance_query; include/sage_gs.h): the exact squared Euclidean
distance transform in cells^2, its four counters, and the position / path lookup in Python floats with round().  It never reads the
library; tests/test_clearance_ref.py holds it to a Python loop and to SciPy."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np

NONE = 0xFFFFFFFF
SRC_MASK8, SRC_TOPDOWN = 0, 1
UNSEEN_BLOCKS = 1
NEGATE, FLIP_X, FLIP_Y = 1, 2, 4
MAX_N = 32768


def obstacles(src, kind=None, min_hits=1, unseen_blocks=False):
    """bool [ny, nx]: a mask's non-zero bytes, or a seen map's cells with occupied >= min_hits (and, with unseen_blocks, those with
    occupied < min_hits and free < min_hits)."""
    src = np.asarray(src)
    if kind is None:
        kind = SRC_TOPDOWN if src.ndim == 3 else SRC_MASK8
    if kind == SRC_MASK8:
        assert src.ndim == 2
        return src != 0
    assert src.ndim == 3 and src.shape[2] == 2 and min_hits >= 1
    free, occ = src[..., 0].astype(np.int64), src[..., 1].astype(np.int64)
    ob = occ >= min_hits
    if unseen_blocks:
        ob = ob | ((occ < min_hits) & (free < min_hits))
    return ob


def d2_brute(ob):
    """uint32 [ny, nx]: per cell the minimum over the obstacle cells of (i - i')^2 + (j - j')^2; NONE everywhere without one."""
    ob = np.asarray(ob, bool)
    ny, nx = ob.shape
    js, is_ = np.nonzero(ob)
    if len(js) == 0:
        return np.full((ny, nx), NONE, np.uint32)
    jj, ii = np.mgrid[0:ny, 0:nx].astype(np.int64)
    best = np.full((ny, nx), np.iinfo(np.int64).max, np.int64)
    for a in range(0, len(js), 256):                                           # (blocks of obstacles bound the memory)
        d = (jj[..., None] - js[a:a + 256]) ** 2 + (ii[..., None] - is_[a:a + 256]) ** 2
        best = np.minimum(best, d.min(-1))
    return best.astype(np.uint32)


def row_distance(ob):
    """int64 [ny, nx]: the distance along x to the nearest obstacle of the same row; -1 where the row has none."""
    ob = np.asarray(ob, bool)
    ny, nx = ob.shape
    idx = np.arange(nx, dtype=np.int64)
    far = 4 * MAX_N
    left = np.maximum.accumulate(np.where(ob, idx, -far), axis=1)              # the last obstacle at or before i
    right = np.minimum.accumulate(np.where(ob, idx, far)[:, ::-1], axis=1)[:, ::-1]
    g = np.minimum(idx - left, right - idx)
    return np.where(ob.any(1)[:, None], g, -1)


def d2_two_pass(ob):
    """The same map as d2_brute by the separable integer form: rows, then for every row j the minimum over rows j' of
    g[j']^2 + (j - j')^2."""
    ob = np.asarray(ob, bool)
    ny, nx = ob.shape
    g = row_distance(ob)
    big = np.int64(1) << 40
    g2 = np.where(g >= 0, g * g, big)
    best = np.full((ny, nx), big, np.int64)
    rows = np.arange(ny, dtype=np.int64)
    for jp in np.nonzero((g >= 0).any(1))[0]:
        best = np.minimum(best, g2[jp][None, :] + ((rows - jp) ** 2)[:, None])
    return np.where(best >= big, NONE, best).astype(np.uint32)


def counts(d2, max_d2):
    """[obstacle cells, cells with 0 < d2 <= max_d2, cells with max_d2 < d2 < NONE, cells equal to NONE]."""
    d = np.asarray(d2).astype(np.int64)
    return [int((d == 0).sum()), int(((d > 0) & (d <= max_d2)).sum()), int(((d > max_d2) & (d < NONE)).sum()), int((d == NONE).sum())]


def clearance(src, kind=None, min_hits=1, unseen_blocks=False, max_d2=0):
    """(d2 uint32 [ny, nx], counts) of one map."""
    d2 = d2_two_pass(obstacles(src, kind, min_hits, unseen_blocks))
    return d2, counts(d2, max_d2)


@dataclass(frozen=True)
class Frame:
    """sgs_clearance_frame: where pixel (0, 0) lies, the sums the flips use, the scale, and what a query applies."""
    min_x: float = 0.0
    min_y: float = 0.0
    sum_x: float = 0.0
    sum_y: float = 0.0
    scale: float = 0.05
    flags: int = NEGATE | FLIP_X | FLIP_Y
    margin: int = 2
    max_d2: int = 0
    n_samples: int = 10
    reserved: int = 0

    def but(self, **kw):
        return replace(self, **kw)


def _pixel(v, lo, scale, n, margin):
    """The pixel of one coordinate, or None when it is outside beyond the margin (NaN and +-inf are)."""
    q = (v - lo) / scale
    if not math.isfinite(q):
        return None
    p = round(q)                                                               # ties to even, an exact Python int
    if not (-margin <= p < n + margin):
        return None
    return max(0, min(n - 1, p))


def sample(d2, f: Frame, x, y):
    """(the d2 under the point, NONE when it is outside beyond the margin; whether the point collides)."""
    x, y = float(x), float(y)
    ny, nx = d2.shape
    if f.flags & NEGATE:
        x, y = -x, -y
    if f.flags & FLIP_X:
        x = f.sum_x - x
    if f.flags & FLIP_Y:
        y = f.sum_y - y
    px, py = _pixel(x, f.min_x, f.scale, nx, f.margin), _pixel(y, f.min_y, f.scale, ny, f.margin)
    if px is None or py is None:
        return NONE, True
    v = int(d2[py, px])
    return v, v <= f.max_d2


def query(d2, f: Frame, segs):
    """int64 [n, 2]: the first colliding sample (from 1) or 0; the d2 under the last sample or NONE.  Python floats throughout."""
    d2 = np.asarray(d2)
    out = np.zeros((len(segs), 2), np.int64)
    for k, (x0, y0, x1, y1) in enumerate(np.asarray(segs, np.float64).tolist()):
        if f.n_samples <= 1:
            v, hit = sample(d2, f, x1, y1)
            out[k] = (1 if hit else 0, v)
            continue
        first, v = 0, NONE
        for s in range(1, f.n_samples + 1):
            t = s / float(f.n_samples)
            v, hit = sample(d2, f, x0 * (1 - t) + x1 * t, y0 * (1 - t) + y1 * t)
            if hit and not first:
                first = s
        out[k] = (first, v)
    return out


def query_vectorised(d2, f: Frame, segs):
    """query() in NumPy fp64 (np.rint rounds ties to even): the form the benchmark's host path and the 10^5-segment test use; held to
    query() by test_clearance_ref.py."""
    d2 = np.asarray(d2)
    ny, nx = d2.shape
    segs = np.asarray(segs, np.float64)
    n = len(segs)
    first = np.zeros(n, np.int64)
    last = np.full(n, NONE, np.int64)
    steps = [None] if f.n_samples <= 1 else range(1, f.n_samples + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in steps:
            if s is None:
                x, y = segs[:, 2].copy(), segs[:, 3].copy()
            else:
                t = s / float(f.n_samples)
                x, y = segs[:, 0] * (1 - t) + segs[:, 2] * t, segs[:, 1] * (1 - t) + segs[:, 3] * t
            if f.flags & NEGATE:
                x, y = -x, -y
            if f.flags & FLIP_X:
                x = f.sum_x - x
            if f.flags & FLIP_Y:
                y = f.sum_y - y
            qx, qy = np.rint((x - f.min_x) / f.scale), np.rint((y - f.min_y) / f.scale)
            ok = (qx >= -f.margin) & (qx < nx + f.margin) & (qy >= -f.margin) & (qy < ny + f.margin)
            px = np.clip(np.where(ok, qx, 0), 0, nx - 1).astype(np.int64)
            py = np.clip(np.where(ok, qy, 0), 0, ny - 1).astype(np.int64)
            v = np.where(ok, d2[py, px].astype(np.int64), NONE)
            hit = ~ok | (v <= f.max_d2)
            idx = 1 if s is None else s
            first = np.where((first == 0) & hit, idx, first)
            last = v
    return np.stack([first, last], 1)


def inflation_limit(radius_m, scale, reach=None):
    """The restatement of sage_gs.clearance.inflation_limit: the largest L such that sqrt((scale a)^2 + (scale b)^2) <= radius_m — in
    float64, as SciPy's sampling= evaluates it — holds for every offset with a^2 + b^2 <= L; raises when one value of a^2 + b^2
    passes for one offset and fails for another.  -1: not even the obstacle itself (radius < 0)."""
    r, s = float(radius_m), float(scale)
    reach = int(r / s) + 2 if reach is None else reach
    verdict = {}
    for a in range(reach + 1):
        for b in range(a + 1):
            ok = math.sqrt((s * a) * (s * a) + (s * b) * (s * b)) <= r
            k = a * a + b * b
            if verdict.setdefault(k, ok) != ok:
                raise ValueError(f"offsets with a^2 + b^2 = {k} disagree at radius {r}, scale {s}")
    L = -1
    for k in sorted(verdict):
        if not verdict[k]:
            break
        L = k
    assert all(not v for k, v in verdict.items() if k > L), "the predicate is not monotone in a^2 + b^2"
    return L
