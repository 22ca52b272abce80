"""From two items of a scene to a trajectory between them: the free cell beside each item on the side that faces the other
(include/sage_gs.h sgs_endpoints), then the planner of sage_gs.geodesic — behind the interface of the reference's trajectory generator.

The reference (vln_trajectory_generator.py) finds each endpoint with get_nearest_free_pixel_on_side, a breadth-first search over Python
sets, twice per candidate pair and once per item in build_connectivity_map.  Here an ItemSet holds the items of a scene on the device;
nearest_free answers any number of (item, target) queries in one call; plan_pairs goes from pairs of item names to trajectory points.

DEPARTURES from the reference, both stated in include/sage_gs.h: among several free cells at the least distance the one of least raster
index y * nx + x is returned (the reference returns whichever its hash table iterates first; `n_at_d == 1` says when there is no choice),
and the half-plane towards the target is evaluated exactly in integers (the reference's float dot has the same sign except within
rounding of zero).  max_search_dist is at most 63.  Paths: see sage_gs.geodesic.astar_pixel.
"""
from __future__ import annotations

import numpy as np

from . import _capi

TOWARDS = _capi.ENDPOINTS_QUERY_TOWARDS
FIELDS_PER_CALL = 64                               # goal cells whose fields are computed and walked in one pair of calls
# what the reference's generate_trajectory_points writes into every point besides its number, position and rotation
POINT_CAMERA = {"action": [], "camera_images": [], "focal_length": 7.0, "horizontal_aperture": 20.954999923706055,
                "vertical_aperture": 20.954999923706055, "focus_distance": 0.0, "clipping_range": [1.0, 1000000.0]}


def _renderer(renderer):
    from .renderer import default_renderer
    return default_renderer() if renderer is None else renderer


def _map_of(where, renderer=None):
    """(renderer, src tensor, max_d2) of a ClearanceMap, a tensor on the device (a mask: free iff 0) or a host grid (free iff 0)."""
    import torch
    from .clearance import ClearanceMap
    if isinstance(where, ClearanceMap):
        return where._r, where.d2, int(where.frame.max_d2)
    r = _renderer(renderer)
    if isinstance(where, torch.Tensor):
        return r, where, 0
    return r, torch.from_numpy(np.ascontiguousarray(np.asarray(where) != 0)).to(r.device), 0


class ItemSet:
    """The items of one scene on the device, in compressed sparse rows.  `names` in the order given; `rows` a NumPy record array
    (_capi.ENDPOINTS_ITEM_DTYPE), one per item: entries, flags, the tight box, the centroid pixel (cx, cy) — the reference's
    instance_centroid_px —, the boundary count and the sums.  An item without pixels is kept (flagged empty), so that indices and
    names stay in step."""

    def __init__(self, names, pixel_lists, nx: int, ny: int, renderer=None):
        import torch
        self._r = _renderer(renderer)
        self.names, self.nx, self.ny = list(names), int(nx), int(ny)
        self.index = {n: k for k, n in enumerate(self.names)}
        if not 1 <= len(self.names) <= _capi.ENDPOINTS_MAX_ITEMS:
            raise ValueError(f"1 .. {_capi.ENDPOINTS_MAX_ITEMS} items")
        lists = [np.asarray(p, np.int64).reshape(-1, 2) for p in pixel_lists]
        offsets = np.concatenate([[0], np.cumsum([len(p) for p in lists])])
        yx = np.concatenate(lists) if lists else np.zeros((0, 2), np.int64)
        inside = (yx[:, 0] >= 0) & (yx[:, 0] < self.ny) & (yx[:, 1] >= 0) & (yx[:, 1] < self.nx)
        cells = np.where(inside, yx[:, 0] * self.nx + yx[:, 1], -1)                  # a pixel outside the grid flags its item
        self.offsets = torch.from_numpy(offsets.astype(np.int32)).to(self._r.device)
        self.cells = torch.from_numpy(np.concatenate([cells, [0]]).astype(np.int32)).to(self._r.device)       # (never an empty tensor)
        blank = torch.zeros((self.ny, self.nx), dtype=torch.uint8, device=self._r.device)
        rows, _, _ = self._r.endpoints(blank, (self.offsets, self.cells), [], max_dist=0)
        self.rows = rows.cpu().numpy().reshape(-1).view(_capi.ENDPOINTS_ITEM_DTYPE).copy()

    @classmethod
    def from_instances(cls, itemid2inst, grid_shape, renderer=None):
        """From the reference's itemid2inst: {name: instance}, an instance's `mask_coords` its (y, x) pixels; grid_shape (ny, nx)."""
        names = list(itemid2inst)
        return cls(names, [(itemid2inst[n] or {}).get("mask_coords", []) or [] for n in names], grid_shape[1], grid_shape[0], renderer)

    def __len__(self):
        return len(self.names)

    def centroid(self, name):
        """(cx, cy) of an item, or None for a flagged one."""
        r = self.rows[self.index[name]]
        return None if int(r["flags"]) else (int(r["cx"]), int(r["cy"]))

    def queries(self, items=None, towards=None) -> np.ndarray:
        """int64 [n, 4] query rows for `items` (names or indices; default every item) with `towards` (None, or per query an (x, y) or
        None)."""
        which = range(len(self)) if items is None else [self.index[i] if not isinstance(i, (int, np.integer)) else int(i) for i in items]
        q = np.zeros((len(which), 4), np.int64)
        q[:, 0] = list(which)
        if towards is not None:
            if len(towards) != len(q):
                raise ValueError("one target (or None) per query")
            for k, t in enumerate(towards):
                if t is not None:
                    q[k, 1:] = (int(t[0]), int(t[1]), TOWARDS)
        return q


def nearest_free(item_set: ItemSet, where, towards=None, items=None, max_search_dist: int = 50) -> np.ndarray:
    """The batch form: for every query the nearest free cell on the side facing its target, as a record array
    (_capi.ENDPOINTS_ANSWER_DTYPE: x, y, d, n_at_d; -1, -1, -1, 0 for none).  where: a ClearanceMap (free where the agent can stand),
    a uint8 / bool tensor on the device or a host grid (free iff 0).  items: names or indices (default: every item once); towards:
    None, or per query an (x, y) or None.  One call, one copy back."""
    r, src, max_d2 = _map_of(where, item_set._r)
    if tuple(src.shape) != (item_set.ny, item_set.nx):
        raise ValueError(f"the map is {tuple(src.shape)}, the items were made for {(item_set.ny, item_set.nx)}")
    q = item_set.queries(items, towards)
    if len(q) == 0:
        return np.zeros(0, _capi.ENDPOINTS_ANSWER_DTYPE)
    _, answers, _ = r.endpoints(src, (item_set.offsets, item_set.cells), q, max_d2=max_d2, max_dist=int(max_search_dist))
    return answers.cpu().numpy().reshape(-1).view(_capi.ENDPOINTS_ANSWER_DTYPE).copy()


def nearest_free_pixel_on_side(instance_mask, base_map, towards_px=None, max_search_dist: int = 50, renderer=None):
    """The drop-in for the reference's get_nearest_free_pixel_on_side: instance_mask a list of (y, x), base_map [H, W] with 0 for a
    free cell, towards_px (x, y) or None; (x, y) or None.  See the module's departures; a target outside the grid answers None."""
    base = np.asarray(base_map)
    if len(instance_mask) == 0 or max_search_dist < 0:
        return None
    s = ItemSet(["item"], [instance_mask], base.shape[1], base.shape[0], renderer)
    a = nearest_free(s, base, None if towards_px is None else [towards_px], max_search_dist=max_search_dist)[0]
    return None if int(a["d"]) < 0 else (int(a["x"]), int(a["y"]))


def connectivity_map(grid_map, itemid2inst, renderer=None) -> dict:
    """The reference's build_connectivity_map: {component: set of item names}, an item belonging to the 4-connected component of free
    cells that holds its nearest free cell (no target); items without one are left out.  A component's key is its region label
    (Renderer.label_regions under connectivity 4), where the reference has a union-find root."""
    import torch
    r = _renderer(renderer)
    grid = np.asarray(grid_map)
    blocked = torch.from_numpy(np.ascontiguousarray(grid != 0)).to(r.device)
    have = {k: v for k, v in itemid2inst.items() if v and v.get("mask_coords")}
    if not have:
        return {}
    items = ItemSet.from_instances(have, grid.shape, r)
    answers = nearest_free(items, blocked)
    labels, _, _ = r.label_regions(~blocked, connectivity=4, max_regions=0)
    found = np.nonzero(answers["d"] >= 0)[0]
    at = torch.from_numpy(answers["y"][found].astype(np.int64) * grid.shape[1] + answers["x"][found]).to(r.device)
    of = labels.reshape(-1)[at].cpu().numpy()
    groups: dict = {}
    for k, label in zip(found.tolist(), of.tolist()):
        groups.setdefault(int(label), set()).add(items.names[k])
    return groups


def are_items_connected(item1, item2, connectivity) -> bool:
    return any(item1 in g and item2 in g for g in connectivity.values())


def _points(path, scale, min_x, min_y):
    from .geodesic import trajectory_points
    return [{"point": str(j), "position": p["position"], "rotation": p["rotation"], **{k: (list(v) if isinstance(v, list) else v) for k, v in POINT_CAMERA.items()}}
            for j, p in enumerate(trajectory_points(path, scale, min_x, min_y))]


def plan_pairs(pairs, itemid2inst, grid_map, scale, min_x, min_y, renderer=None, item_set=None) -> list:
    """validate_and_generate_path for every (start_item, end_item) of pairs: a list of {"start", "end", "points"} or None.  One
    endpoints call for all pairs (two queries each: the start item towards the end item's centroid and the other way round), one
    geodesic field per distinct goal cell and one path call per FIELDS_PER_CALL of them, then the points on the host."""
    import torch
    r = _renderer(renderer)
    grid = np.asarray(grid_map)
    known = {k: v for k, v in itemid2inst.items() if v}
    out = [None] * len(pairs)
    if not known or not len(pairs):
        return out
    items = ItemSet.from_instances(known, grid.shape, r) if item_set is None else item_set
    live = [k for k, (a, b) in enumerate(pairs) if a in items.index and b in items.index and items.centroid(a) is not None and items.centroid(b) is not None]
    if not live:
        return out
    blocked = torch.from_numpy(np.ascontiguousarray(grid != 0)).to(r.device)
    ends = nearest_free(items, blocked, items=[pairs[k][0] for k in live] + [pairs[k][1] for k in live],
                        towards=[items.centroid(pairs[k][1]) for k in live] + [items.centroid(pairs[k][0]) for k in live])
    starts, goals = ends[:len(live)], ends[len(live):]
    both = [n for n in range(len(live)) if starts["d"][n] >= 0 and goals["d"][n] >= 0]
    by_goal: dict = {}
    for n in both:
        by_goal.setdefault((int(goals["x"][n]), int(goals["y"][n])), []).append(n)
    cells = list(by_goal)
    for c0 in range(0, len(cells), FIELDS_PER_CALL):
        chunk = cells[c0:c0 + FIELDS_PER_CALL]
        seeds = [(f, x, y) for f, (x, y) in enumerate(chunk)]
        fmap = np.zeros(len(chunk), np.int64)
        steps, _ = r.geodesic_field(blocked, seeds, field_map=fmap)
        q = [(f, int(starts["x"][n]), int(starts["y"][n])) for f, c in enumerate(chunk) for n in by_goal[c]]
        owners = [n for c in chunk for n in by_goal[c]]
        host = steps.cpu().numpy().view(np.uint32)
        s = np.array([host[f, y, x] for f, x, y in q], np.int64)
        reach = s[:, 0] != _capi.GEODESIC_NONE
        max_len = int(np.where(reach, s[:, 0] + s[:, 1] + 1, 1).max())
        walked, info = r.geodesic_path(blocked, steps, q, field_map=fmap, max_len=max_len)
        walked, info = walked.cpu().numpy(), info.cpu().numpy()
        for n, w, (length, status) in zip(owners, walked, info):
            if status != _capi.GEODESIC_PATH_OK:
                continue
            a, b = pairs[live[n]]
            out[live[n]] = {"start": a, "end": b, "points": _points([(int(x), int(y)) for x, y in w[:length]], scale, min_x, min_y)}
    return out


def validate_and_generate_path(start_item, end_item, itemid2inst, grid_map, scale, min_x, min_y, renderer=None):
    """The drop-in for the reference's validate_and_generate_path: {"start", "end", "points"} or None."""
    return plan_pairs([(start_item, end_item)], itemid2inst, grid_map, scale, min_x, min_y, renderer)[0]
