"""The definition of the item endpoints (include/sage_gs.h sgs_endpoints) restated in NumPy and Python integers, for the tests.

An item is a list of raster indices y * nx + x, duplicates allowed.  B is the set of its distinct cells with a 4-neighbour outside the
item (outside the grid is outside the item); d(c) the L1 distance from c to B; a candidate is a free cell with d <= max_dist that,
when a target is given, satisfies (n x - Sx)(n tx - Sx) + (n y - Sy)(n ty - Sy) >= 0 in exact integers (n the entries, S their sums).
The answer is (x, y, d*, n_at_d): the least d among the candidates, the candidate of least raster index at that d and how many there
are at that d; (-1, -1, -1, 0) when there is none."""
from __future__ import annotations

import numpy as np

SRC_MASK8, SRC_D2 = 0, 1
ITEM_EMPTY, ITEM_BAD_CELL, ITEM_TOO_LONG = 1, 2, 4
QUERY_TOWARDS = 1
MAX_ENTRIES = 1 << 19
MAX_DIST = 63
INT32_MAX = 0x7FFFFFFF
NONE = (-1, -1, -1, 0)
ITEM_DTYPE = np.dtype([("n", "<u4"), ("flags", "<u4"), ("x_min", "<i4"), ("y_min", "<i4"), ("x_end", "<i4"), ("y_end", "<i4"), ("cx", "<i4"), ("cy", "<i4"),
                       ("boundary", "<u4"), ("reserved", "<u4"), ("sum_x", "<u8"), ("sum_y", "<u8")])
QUERY_DTYPE = np.dtype([("item", "<i4"), ("tx", "<i4"), ("ty", "<i4"), ("flags", "<u4")])
ANSWER_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("d", "<i4"), ("n_at_d", "<i4")])
assert ITEM_DTYPE.itemsize == 56 and QUERY_DTYPE.itemsize == 16 and ANSWER_DTYPE.itemsize == 16


def round_half_even(s: int, n: int) -> int:
    """The exact quotient s / n rounded half to even, in integers: what int(round(mean)) gives."""
    q, r = divmod(int(s), int(n))
    if 2 * r > n or (2 * r == n and q % 2 == 1):
        return q + 1
    return q


def boundary(cells, nx, ny) -> set:
    """B as a set of (y, x), from a Python set of the item's cells."""
    s = {(int(c) // nx, int(c) % nx) for c in cells}
    return {(y, x) for (y, x) in s if any(n not in s for n in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)))}


def field(b: set, nx, ny) -> np.ndarray:
    """int64 [ny, nx]: the L1 distance to B, by a min-plus sweep along x (all rows at once, there and back) and one along y."""
    big = 4 * (nx + ny)
    d = np.full((ny, nx), big, np.int64)
    for (y, x) in b:
        d[y, x] = 0
    for i in range(1, nx):
        d[:, i] = np.minimum(d[:, i], d[:, i - 1] + 1)
    for i in range(nx - 2, -1, -1):
        d[:, i] = np.minimum(d[:, i], d[:, i + 1] + 1)
    for j in range(1, ny):
        d[j] = np.minimum(d[j], d[j - 1] + 1)
    for j in range(ny - 2, -1, -1):
        d[j] = np.minimum(d[j], d[j + 1] + 1)
    return d


def item_flags(cells, nx, ny) -> int:
    c = np.asarray(cells, np.int64).reshape(-1)
    if len(c) == 0:
        return ITEM_EMPTY
    if len(c) > MAX_ENTRIES:
        return ITEM_TOO_LONG                                                        # the list is not looked at
    return ITEM_BAD_CELL if ((c < 0) | (c >= nx * ny)).any() else 0


def item_row(cells, nx, ny) -> np.ndarray:
    """The item's row (ITEM_DTYPE, one record)."""
    r = np.zeros(1, ITEM_DTYPE)
    c = np.asarray(cells, np.int64).reshape(-1)
    flags = item_flags(c, nx, ny)
    r["n"], r["flags"] = len(c), flags
    if flags:
        r["x_min"], r["y_min"], r["cx"], r["cy"] = INT32_MAX, INT32_MAX, -1, -1
        return r[0]
    ys, xs = c // nx, c % nx
    sx, sy = int(xs.sum()), int(ys.sum())
    r["x_min"], r["y_min"], r["x_end"], r["y_end"] = xs.min(), ys.min(), xs.max() + 1, ys.max() + 1
    r["cx"], r["cy"] = round_half_even(sx, len(c)), round_half_even(sy, len(c))
    r["boundary"], r["sum_x"], r["sum_y"] = len(boundary(c, nx, ny)), sx, sy
    return r[0]


def window(row, nx, ny, max_dist):
    """(x0, y0, w, h) of the item's window: its box grown by max_dist, clipped; empty for a flagged item."""
    if int(row["flags"]):
        return 0, 0, 0, 0
    x0, y0 = max(int(row["x_min"]) - max_dist, 0), max(int(row["y_min"]) - max_dist, 0)
    return x0, y0, min(int(row["x_end"]) + max_dist, nx) - x0, min(int(row["y_end"]) + max_dist, ny) - y0


def work_needed(rows, nx, ny, max_dist) -> int:
    total = sum(w * h for _, _, w, h in (window(r, nx, ny, max_dist) for r in rows))
    return 8 * len(rows) + ((total + 7) & ~7)


def free_of(src, source=SRC_MASK8, max_d2=0) -> np.ndarray:
    src = np.asarray(src)
    return src == 0 if source == SRC_MASK8 else src.astype(np.uint32) > np.uint32(max_d2)


def query(free, cells, max_dist=50, target=None, d=None):
    """((x, y, d*, n_at_d), the candidates at d* as a set of (x, y)) of one item on the grid free bool [ny, nx]; target (tx, ty) or
    None.  d: the item's field, when the caller has it."""
    ny, nx = free.shape
    c = np.asarray(cells, np.int64).reshape(-1)
    if item_flags(c, nx, ny) or (target is not None and not (0 <= target[0] < nx and 0 <= target[1] < ny)):
        return NONE, set()
    if d is None:
        d = field(boundary(c, nx, ny), nx, ny)
    n, sx, sy = len(c), int((c % nx).sum()), int((c // nx).sum())
    for level in range(0, max_dist + 1):
        ys, xs = np.nonzero((d == level) & free)                                    # raster order
        cand = [(int(x), int(y)) for y, x in zip(ys, xs)
                if target is None or (n * int(x) - sx) * (n * int(target[0]) - sx) + (n * int(y) - sy) * (n * int(target[1]) - sy) >= 0]
        if cand:
            return (cand[0][0], cand[0][1], level, len(cand)), set(cand)
    return NONE, set()


def endpoints(src, items, queries, max_dist=50, source=SRC_MASK8, max_d2=0):
    """(rows ITEM_DTYPE [n_items], answers ANSWER_DTYPE [n_queries], counts [answered, none, flagged, work bytes needed], the candidate
    sets) of items (a list of index lists) and queries (rows of item, tx, ty, flags)."""
    free = free_of(src, source, max_d2)
    ny, nx = free.shape
    rows = np.array([item_row(c, nx, ny) for c in items], ITEM_DTYPE)
    fields = {}
    answers, cands = np.zeros(len(queries), ANSWER_DTYPE), []
    for k, (item, tx, ty, flags) in enumerate(np.asarray(queries, np.int64).reshape(-1, 4).tolist()):
        a, cs = NONE, set()
        if 0 <= item < len(items) and (flags & ~QUERY_TOWARDS) == 0 and not int(rows["flags"][item]):
            if item not in fields:
                fields[item] = field(boundary(items[item], nx, ny), nx, ny)
            a, cs = query(free, items[item], max_dist, (tx, ty) if flags & QUERY_TOWARDS else None, fields[item])
        answers[k] = a
        cands.append(cs)
    answered = int((answers["d"] >= 0).sum())
    counts = [answered, len(queries) - answered, int((rows["flags"] != 0).sum()), work_needed(rows, nx, ny, max_dist)]
    return rows, answers, counts, cands
