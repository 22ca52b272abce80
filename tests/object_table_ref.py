"""A NumPy restatement of the visible-object table (sgs_object_table, include/sage_gs.h): per label the pixel count, the tight box, the
sums of x and y and the least depth pattern, and the two counters.  Written with np.bincount, np.minimum.at / np.maximum.at and masks;
test_object_table_ref.py holds it to a plain Python loop over the pixels on small frames, so it is not only checked against itself.

The table is this project's own definition (the reference reads no such observation): the header's rule is what is restated here.
"""
from __future__ import annotations

import numpy as np

ID_NONE = -1
Z_INF = np.uint32(0x7F800000)                   # +inf: an empty row's z_min, and the largest fp32 pattern that enters the minimum
ROW_DTYPE = np.dtype([("n_pixels", "<u4"), ("x_min", "<i4"), ("y_min", "<i4"), ("x_end", "<i4"), ("y_end", "<i4"), ("z_min", "<f4"),
                      ("sum_x", "<u8"), ("sum_y", "<u8")])
FIELDS = ROW_DTYPE.names
INT32_MAX = 2 ** 31 - 1


def empty_rows(n_labels):
    rows = np.zeros(int(n_labels), ROW_DTYPE)
    rows["x_min"] = rows["y_min"] = INT32_MAX
    rows["z_min"] = np.float32(np.inf)
    return rows


def z_bits(rows):
    """z_min as the uint32 patterns it is compared by."""
    return np.ascontiguousarray(rows["z_min"]).view(np.uint32)


def table(ids, depth, n_labels):
    """(rows ROW_DTYPE [n_labels], counts uint32 [2]) of one frame: ids int32 [H,W], depth fp32 [H,W] or None."""
    ids = np.asarray(ids)
    assert ids.dtype == np.int32 and ids.ndim == 2
    H, W = ids.shape
    flat = ids.reshape(-1).astype(np.int64)
    in_label = (flat >= 0) & (flat < n_labels)
    lab = flat[in_label]
    ys, xs = np.divmod(np.flatnonzero(in_label), W)
    rows = empty_rows(n_labels)
    rows["n_pixels"] = np.bincount(lab, minlength=n_labels)
    assert H * W * max(H, W) < 2 ** 53                       # bincount sums its weights in fp64: exact below 2^53
    rows["sum_x"] = np.bincount(lab, weights=xs, minlength=n_labels).astype(np.uint64)
    rows["sum_y"] = np.bincount(lab, weights=ys, minlength=n_labels).astype(np.uint64)
    lo = np.full((2, n_labels), INT32_MAX, np.int64)
    hi = np.zeros((2, n_labels), np.int64)
    np.minimum.at(lo[0], lab, xs); np.minimum.at(lo[1], lab, ys)
    np.maximum.at(hi[0], lab, xs + 1); np.maximum.at(hi[1], lab, ys + 1)
    rows["x_min"], rows["y_min"], rows["x_end"], rows["y_end"] = lo[0], lo[1], hi[0], hi[1]
    if depth is not None:
        bits = np.ascontiguousarray(depth, np.float32).reshape(-1).view(np.uint32)[in_label]
        enters = bits <= Z_INF                               # +0, denormals, positive finite, +inf; not negatives, -0, NaNs
        z = np.full(n_labels, Z_INF, np.uint32)
        np.minimum.at(z, lab[enters], bits[enters])
        rows["z_min"] = z.view(np.float32)
    counts = np.array([(flat == ID_NONE).sum(), (~in_label & (flat != ID_NONE)).sum()], np.uint32)
    return rows, counts


def table_by_loop(ids, depth, n_labels):
    """The same table by the rule read aloud, pixel by pixel (small frames only)."""
    H, W = ids.shape
    rows, counts = empty_rows(n_labels), np.zeros(2, np.uint32)
    z = np.full(n_labels, Z_INF, np.uint32)
    for y in range(H):
        for x in range(W):
            k = int(ids[y, x])
            if not 0 <= k < n_labels:
                counts[0 if k == ID_NONE else 1] += 1
                continue
            r = rows[k]
            r["n_pixels"] += 1; r["sum_x"] += np.uint64(x); r["sum_y"] += np.uint64(y)
            r["x_min"], r["y_min"], r["x_end"], r["y_end"] = min(r["x_min"], x), min(r["y_min"], y), max(r["x_end"], x + 1), max(r["y_end"], y + 1)
            b = np.float32(depth[y, x]).view(np.uint32) if depth is not None else Z_INF
            if b <= Z_INF:
                z[k] = min(z[k], b)
    rows["z_min"] = z.view(np.float32)
    return rows, counts


def first_difference(got, want):
    """None when the two tables are equal in every field (z_min by bits), else (label, field, got, want) of the first difference in
    label order, fields in the struct's order."""
    assert got.shape == want.shape
    for k in range(len(want)):
        for f in FIELDS:
            g, w = (z_bits(got)[k], z_bits(want)[k]) if f == "z_min" else (got[f][k], want[f][k])
            if g != w:
                return (k, f, (hex(int(g)) if f == "z_min" else int(g)), (hex(int(w)) if f == "z_min" else int(w)))
    return None
