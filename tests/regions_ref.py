"""The connected regions of a grid (sgs_regions_label; csrc/sgs_regions.h), restated on the host: NumPy only.

The definition is this project's own (include/sage_gs.h): the regions are the classes of the set under 4- or 8-connectivity, and a
region's label is 1 + the number of regions whose least raster index j * nx + i is smaller than its own.  label() is a two-pass
union-find over RUNS (maximal pieces of a row inside the set): runs are numbered in raster order, so a run's number orders as its
first cell does; runs of neighbouring rows are united when they touch (their column ranges overlap; under 8-connectivity, when grown
by one), always linking the larger root to the smaller; a root is then the first run of its region, and the roots in run order are
the labels 1, 2, ....  test_regions_ref.py holds it to a brute-force flood fill, to scipy.ndimage.label and to the reference's
recorded semantic-map items."""
from __future__ import annotations

import numpy as np

SRC_MASK8, SRC_D2 = 0, 1
NO_FIRST = 0xFFFFFFFF
INT32_MAX = 0x7FFFFFFF
ROW_DTYPE = np.dtype([("area", "<u4"), ("x_min", "<i4"), ("y_min", "<i4"), ("x_end", "<i4"), ("y_end", "<i4"), ("first", "<u4"),
                      ("sum_x", "<u8"), ("sum_y", "<u8")])


def in_set(src, lo, hi):
    """bool [ny, nx]: lo <= v <= hi on a uint8 mask or a uint32 d2 map (int32 views of one are read as uint32)."""
    v = np.asarray(src)
    v = v.view(np.uint32) if v.dtype == np.int32 else v.astype(np.uint32)
    return (v >= np.uint32(lo)) & (v <= np.uint32(hi))


def label(cells, connectivity=8):
    """cells bool [ny, nx] -> (labels int32 [ny, nx], n)."""
    assert connectivity in (4, 8)
    a = np.asarray(cells, bool)
    ny, nx = a.shape
    pad = np.zeros((ny, nx + 2), np.int8)
    pad[:, 1:-1] = a
    d = np.diff(pad, axis=1)
    rows, start = np.nonzero(d == 1)                                               # runs in raster order: row, first column
    _, end = np.nonzero(d == -1)                                                   # one past the last column
    n_runs = len(start)
    parent = list(range(n_runs))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    first_of_row = np.searchsorted(rows, np.arange(ny + 1))
    grow = 1 if connectivity == 8 else 0
    s, e = start.tolist(), end.tolist()
    for j in range(1, ny):
        p, p_end, q, q_end = int(first_of_row[j - 1]), int(first_of_row[j]), int(first_of_row[j]), int(first_of_row[j + 1])
        while p < p_end and q < q_end:
            if s[p] < e[q] + grow and s[q] < e[p] + grow:
                rp, rq = find(p), find(q)
                if rp != rq:
                    parent[max(rp, rq)] = min(rp, rq)
            if e[p] < e[q]:
                p += 1
            else:
                q += 1
    root = np.array([find(r) for r in range(n_runs)], np.int64)
    is_root = root == np.arange(n_runs)
    rank = np.cumsum(is_root)
    run_label = rank[root] if n_runs else np.zeros(0, np.int64)
    flat = np.zeros(ny * (nx + 1) + 1, np.int64)                                   # rows one cell wider: a run may end at nx
    at = rows * (nx + 1)
    np.add.at(flat, at + start, run_label)
    np.add.at(flat, at + end, -run_label)
    labels = np.cumsum(flat)[:-1].reshape(ny, nx + 1)[:, :nx]
    return np.ascontiguousarray(labels.astype(np.int32)), int(is_root.sum())


def flood_fill(cells, connectivity=8):
    """The definition, as a loop: the cells in raster order, each unlabelled one starting the next label and a stack."""
    a = np.asarray(cells, bool)
    ny, nx = a.shape
    labels = np.zeros((ny, nx), np.int32)
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    n = 0
    for j in range(ny):
        for i in range(nx):
            if not a[j, i] or labels[j, i]:
                continue
            n += 1
            labels[j, i] = n
            stack = [(j, i)]
            while stack:
                y, x = stack.pop()
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < ny and 0 <= xx < nx and a[yy, xx] and not labels[yy, xx]:
                        labels[yy, xx] = n
                        stack.append((yy, xx))
    return labels, n


def empty_rows(n):
    rows = np.zeros(n, ROW_DTYPE)
    rows["x_min"], rows["y_min"], rows["first"] = INT32_MAX, INT32_MAX, NO_FIRST
    return rows


def rows_of(labels, n, max_regions):
    """The sgs_region_row records [max_regions] of a label map with n regions: row r describes label r + 1."""
    labels = np.asarray(labels)
    ny, nx = labels.shape
    rows = empty_rows(max_regions)
    j, i = np.nonzero((labels > 0) & (labels <= max_regions))
    r = labels[j, i].astype(np.int64) - 1
    np.add.at(rows["area"], r, 1)
    np.minimum.at(rows["x_min"], r, i.astype(np.int32))
    np.minimum.at(rows["y_min"], r, j.astype(np.int32))
    np.maximum.at(rows["x_end"], r, (i + 1).astype(np.int32))
    np.maximum.at(rows["y_end"], r, (j + 1).astype(np.int32))
    np.minimum.at(rows["first"], r, (j * nx + i).astype(np.uint32))
    np.add.at(rows["sum_x"], r, i.astype(np.uint64))
    np.add.at(rows["sum_y"], r, j.astype(np.uint64))
    return rows


def counts_of(labels, n):
    """uint32 [4]: regions, cells in the set, the largest area, the least label that has it."""
    area = np.bincount(np.asarray(labels).reshape(-1), minlength=n + 1)[1:]
    if n == 0:
        return np.array([0, 0, 0, 0], np.uint32)
    return np.array([n, int(area.sum()), int(area.max()), int(np.argmax(area)) + 1], np.uint32)


def regions(cells, connectivity=8, max_regions=None):
    """(labels, rows, counts) of one map; max_regions defaults to the number of regions."""
    labels, n = label(cells, connectivity)
    return labels, rows_of(labels, n, n if max_regions is None else max_regions), counts_of(labels, n)
