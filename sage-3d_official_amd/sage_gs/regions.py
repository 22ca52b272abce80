"""Which cells belong together: the connected regions of a grid on the GPU (include/sage_gs.h sgs_regions_label), numbered as
scipy.ndimage.label numbers them, behind the interface of the reference's 2-D semantic-map builder.

The reference (semantic_map_builder.py) cuts the wall pixels of a scene's occupancy.png into wall items and its zero pixels into
"Unable Area" items with two scipy.ndimage.label calls on a 3x3 structure; every item carries an area, a box in metres and its cells'
centres.  Regions keeps the label map on the device; semantic_map_items writes the items exactly as the reference writes them.  On a
clearance map the regions of the free cells are reachability: the reference's planner cuts corners, so two free cells have a path
exactly when they lie in one 8-connected region (ClearanceMap.free_regions, same_region).
"""
from __future__ import annotations

import numpy as np

from . import _capi

PREDEFINED_CLASSES = ("door", "window", "chair", "table", "sofa", "bed", "wardrobe", "plant", "floor", "wall", "ceiling")
WALL_CATEGORY_ID = PREDEFINED_CLASSES.index("wall") + 1
MIN_UNABLE_AREA = 5                                # an "Unable Area" below this many cells is dropped; the numbering of the rest goes on


class Regions:
    """The regions of one map.  `labels` is the int32 [ny, nx] tensor on the device; `table` a NumPy record array
    (_capi.REGION_ROW_DTYPE) with one row per region, row r for label r + 1; `counts` four Python ints: regions, cells in the set,
    the largest area, the least label that has it."""

    def __init__(self, renderer, labels, table, counts):
        self._r, self.labels, self.table = renderer, labels, table
        self.counts = tuple(int(v) for v in counts)
        self.n = self.counts[0]
        self.ny, self.nx = int(labels.shape[0]), int(labels.shape[1])
        self._order = None

    @classmethod
    def of(cls, src, *, renderer=None, first_guess: int = 1024, **kw):
        """The regions of one map `src` — a tensor on the device, or anything np.asarray takes (uploaded as a mask) — with
        Renderer.label_regions' keywords.  The table is complete: when the map has more regions than first_guess rows, the call is
        made again with as many rows as there are regions."""
        import torch
        from .renderer import default_renderer
        r = default_renderer() if renderer is None else renderer
        if not isinstance(src, torch.Tensor):
            src = torch.from_numpy(np.ascontiguousarray(np.asarray(src)).astype(np.uint8, copy=False)).to(r.device)
        if src.dim() != 2:
            raise ValueError("src must be one map [ny, nx]")
        labels, rows, counts = r.label_regions(src, max_regions=max(1, int(first_guess)), **kw)
        n = int(counts[0].item()) & 0xFFFFFFFF
        if n > rows.shape[0]:
            labels, rows, counts = r.label_regions(src, max_regions=n, **kw)
        table = rows[:n].cpu().numpy().reshape(-1).view(_capi.REGION_ROW_DTYPE).copy()
        return cls(r, labels, table, counts.cpu().numpy().view(np.uint32))

    def labels_host(self) -> np.ndarray:
        return self.labels.cpu().numpy()

    def largest(self) -> int:
        """The least label among the regions of the largest area; 0 when there is no region."""
        return self.counts[3]

    def cells(self, k: int):
        """(ys, xs) of label k in raster order, as np.nonzero(labels == k) gives them: from ONE stable device sort of the cells in
        the set by label, made at the first call and kept."""
        import torch
        k = int(k)
        if not 1 <= k <= self.n:
            raise ValueError(f"label {k} outside 1 .. {self.n}")
        if self._order is None:
            flat = self.labels.reshape(-1)
            at = torch.nonzero(flat, as_tuple=False).reshape(-1)                  # raster order
            _, perm = torch.sort(flat[at], stable=True)
            self._order = at[perm].cpu().numpy()
            self._begin = np.concatenate([[0], np.cumsum(self.table["area"].astype(np.int64))])
        idx = self._order[self._begin[k - 1]:self._begin[k]]
        return idx // self.nx, idx % self.nx

    def label_at(self, cells) -> np.ndarray:
        """int64 [n]: the label under every (i, j) of cells; 0 outside the set and outside the map.  One gather on the device."""
        import torch
        c = np.asarray(cells, np.int64).reshape(-1, 2)
        inside = (c[:, 0] >= 0) & (c[:, 0] < self.nx) & (c[:, 1] >= 0) & (c[:, 1] < self.ny)
        at = np.where(inside, c[:, 1] * self.nx + c[:, 0], 0)
        got = self.labels.reshape(-1)[torch.from_numpy(at).to(self.labels.device)].cpu().numpy().astype(np.int64)
        return np.where(inside, got, 0)

    def same(self, a_cells, b_cells) -> np.ndarray:
        """bool [n]: whether cells a[k] and b[k], (i, j) each, lie in one region (both in the set)."""
        a = np.asarray(a_cells, np.int64).reshape(-1, 2)
        both = self.label_at(np.concatenate([a, np.asarray(b_cells, np.int64).reshape(-1, 2)]))
        la, lb = both[:len(a)], both[len(a):]
        return (la != 0) & (la == lb)


def label(mask, connectivity: int = 8, renderer=None):
    """scipy.ndimage.label(mask, structure) for the 3x3 structure (connectivity 8) or the cross (4), on the GPU: (int32 array of the
    mask's shape, n).  mask: anything np.asarray takes (non-zero is in the set) or a uint8 / bool tensor on the device."""
    import torch
    from .renderer import default_renderer
    r = default_renderer() if renderer is None else renderer
    src = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0)).to(r.device)
    if src.dim() != 2:
        raise ValueError("mask must be [ny, nx]")
    labels, _, counts = r.label_regions(src, connectivity=connectivity, max_regions=0)
    return labels.cpu().numpy(), int(counts[0].item()) & 0xFFFFFFFF


def wall_value(occupancy) -> int:
    """The grey value the reference takes for walls (semantic_map_builder.py:91-100): among the values in (0, 250) the most frequent
    one — the least of them on a tie, as np.argmax keeps the first —, and the least value of the image when there is none."""
    values, counts = np.unique(np.asarray(occupancy).reshape(-1), return_counts=True)
    cand = [(int(v), int(c)) for v, c in zip(values, counts) if 0 < v < 250]
    if not cand:
        return int(values[0])
    return cand[int(np.argmax([c for _, c in cand]))][0]


def _f2(v) -> str:
    return f"{float(v):.2f}"


def items_of_labels(n, cells_of, scale, x_min, y_min, kind: str) -> list:
    """The items of one label map (of the occupancy image turned upside down) as the reference writes them; kind 'wall' or 'unable'.
    cells_of(k) -> (ys, xs) of label k in raster order.  Host float64 in the reference's order of operations."""
    name = "wall" if kind == "wall" else "unable_area"
    z = 3.0 if kind == "wall" else 0.0
    out, kept = [], 0
    for idx in range(1, n + 1):
        ys, xs = cells_of(idx)
        if kind != "wall" and len(xs) < MIN_UNABLE_AREA:
            continue
        kept += 1
        x_left, x_right = x_min + xs.min() * scale, x_min + (xs.max() + 1) * scale
        y_bottom, y_top = y_min + ys.min() * scale, y_min + (ys.max() + 1) * scale
        out.append({"category_id": WALL_CATEGORY_ID if kind == "wall" else -1, "category_label": "wall" if kind == "wall" else "Unable Area",
                    "instance_id": f"{name}_{idx}", "item_id": f"{name}_{kept}",
                    "bbox_m": [_f2(x_left), _f2(y_bottom), _f2(x_right), _f2(y_top)],
                    "bbox_xywh_m": [_f2(x_left), _f2(y_bottom), _f2(x_right - x_left), _f2(y_top - y_bottom)],
                    "area": int(len(xs)), "height_m": _f2(z), "min_z_m": _f2(0.0), "max_z_m": _f2(z),
                    "mask_coords_m": [[_f2(y_min + (y + 0.5) * scale), _f2(x_min + (x + 0.5) * scale)] for y, x in zip(ys, xs)]})
    return out


def semantic_map_items(occupancy, scale, x_min, y_min, renderer=None, label_fn=None) -> list:
    """The wall and "Unable Area" items of a scene's occupancy image (uint8 [h, w], as PIL's "L" conversion gives it) exactly as the
    reference's build_semantic_maps writes them for a scene without object boxes: the image turned upside down, the pixels equal to
    wall_value(occupancy) labelled into walls and the zero pixels into unable areas under 8-connectivity, instance_id numbered by
    label, item_id by the items kept.  label_fn(cells bool [h, w]) -> (labels, n) replaces the device (a host restatement, in
    tests)."""
    occ = np.ascontiguousarray(np.flipud(np.asarray(occupancy)))
    if occ.ndim != 2 or occ.dtype != np.uint8:
        raise ValueError("occupancy must be a uint8 [h, w] image")
    out = []
    for kind, value in (("wall", wall_value(occ)), ("unable", 0)):
        if label_fn is not None:
            labels, n = label_fn(occ == value)
            cells_of = lambda k, labels=labels: np.nonzero(labels == k)          # noqa: E731
        else:
            import torch
            from .renderer import default_renderer
            r = default_renderer() if renderer is None else renderer
            reg = Regions.of(torch.from_numpy(occ).to(r.device), renderer=r, lo=value, hi=value)
            n, cells_of = reg.n, reg.cells
        out += items_of_labels(n, cells_of, scale, x_min, y_min, kind)
    return out
