"""Where an agent can stand: the clearance map (include/sage_gs.h sgs_clearance_map, sgs_clearance_query) behind the interface of the
reference's 2-D collision detector.

The reference (collision_detector.py) builds an obstacle grid from a semantic map, runs SciPy's Euclidean distance transform on it,
grows the obstacles by the robot radius (dist_m <= robot_radius_m) and looks positions and ten-sample path segments up in the grown
grid.  ClearanceMap keeps the grid on the GPU: the exact squared distance transform d2 (integers, cells^2) is computed there once,
the growth is the threshold d2 <= inflation_limit(radius, scale), and any number of positions or segments are answered by one launch.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass

import numpy as np

from . import _capi

OBSTACLE_LABELS = ("unable area", "wall")          # category_label, lower-cased (collision_detector.py:106-107)


def inflation_limit(radius_m: float, scale: float) -> int:
    """The largest integer L = a^2 + b^2 such that the reference's predicate sqrt((scale a)^2 + (scale b)^2) <= radius_m — evaluated
    in float64 exactly as SciPy's distance_transform_edt(sampling=scale) followed by `dist_m <= robot_radius_m` evaluates it — holds
    for every cell offset (a, b) with a^2 + b^2 <= L: a cell is inside the obstacles grown by radius_m iff its d2 <= L.  This is NOT
    floor((radius_m / scale)^2): at (0.15, 0.05) three cells square and root to 0.15000000000000002, so the reference does not grow
    an obstacle by a full three cells, and L is 8.  Raises ValueError if some value of a^2 + b^2 passes for one offset and fails for
    another (no threshold on d2 could then reproduce the reference), or if the scale is not positive and finite.  A radius below 0
    gives -1: not even the obstacle cell."""
    r, s = float(radius_m), float(scale)
    if not (math.isfinite(s) and s > 0.0) or math.isnan(r):
        raise ValueError("scale must be finite and > 0, radius_m a number")
    if r < 0.0:
        return -1
    if not r / s <= 4096.0:
        raise ValueError(f"radius {r} at scale {s} is more than 4096 cells")
    reach = int(r / s) + 2
    passes: dict = {}
    for a in range(reach + 1):
        da = s * a
        for b in range(a + 1):
            db = s * b
            ok = math.sqrt(da * da + db * db) <= r
            if passes.setdefault(a * a + b * b, ok) != ok:
                raise ValueError(f"radius {r} at scale {s}: offsets with a^2 + b^2 = {a * a + b * b} fall on both sides of the radius")
    limit, failed = -1, False
    for k in sorted(passes):
        if passes[k] and failed:
            raise ValueError(f"radius {r} at scale {s}: a^2 + b^2 = {k} is inside although a smaller value is outside")
        if passes[k]:
            limit = k
        else:
            failed = True
    return limit


@dataclass
class ClearanceFrame:
    """include/sage_gs.h sgs_clearance_frame: how a caller's (x, y) reaches a pixel of the map, and what a query applies.  The
    defaults of the three flags are those of the reference's forward_position_mapping."""
    min_x: float
    min_y: float
    max_x: float
    max_y: float
    scale: float = 0.05
    negate_xy: bool = True
    flip_x: bool = True
    flip_y: bool = True
    margin: int = 2
    max_d2: int = 0

    def c_frame(self, n_samples: int = 10) -> "_capi.SgsClearanceFrame":
        flags = (_capi.CLEARANCE_NEGATE if self.negate_xy else 0) | (_capi.CLEARANCE_FLIP_X if self.flip_x else 0) | \
                (_capi.CLEARANCE_FLIP_Y if self.flip_y else 0)
        return _capi.SgsClearanceFrame(float(self.min_x), float(self.min_y), float(self.min_x) + float(self.max_x),
                                       float(self.min_y) + float(self.max_y), float(self.scale), flags, int(self.margin),
                                       int(self.max_d2), int(n_samples), 0)


def load_semantic_map(path, scale: float = 0.05):
    """The one-off host load of a 2-D semantic map JSON (a list of instances with `category_label` and `mask_coords_m`, pairs of
    (y, x) in metres): (mask uint8 [height, width], (min_x, max_x, min_y, max_y)).  Bounds, size and pixels as the reference's
    _load_map_data / _build_obstacle_map compute them: the bounds over EVERY instance's coordinates, height and width
    int(ceil(extent / scale)) + 1, an obstacle pixel int(round((v - min) / scale)) for the instances labelled 'unable area' or
    'wall' (lower-cased).  Raises where the reference would go on without a map (a missing file, no coordinates)."""
    with open(path) as fh:
        instances = json.load(fh)
    coords = [np.asarray(inst.get("mask_coords_m", []), np.float64).reshape(-1, 2) for inst in instances]
    every = np.concatenate(coords) if coords else np.zeros((0, 2))
    if len(every) == 0:
        raise ValueError(f"{path}: no coordinates in the map")
    min_y, max_y, min_x, max_x = float(every[:, 0].min()), float(every[:, 0].max()), float(every[:, 1].min()), float(every[:, 1].max())
    scale = float(scale)
    height, width = int(np.ceil((max_y - min_y) / scale)) + 1, int(np.ceil((max_x - min_x) / scale)) + 1
    mask = np.zeros((height, width), np.uint8)
    for inst, yx in zip(instances, coords):
        if str(inst.get("category_label", "")).lower() not in OBSTACLE_LABELS or len(yx) == 0:
            continue
        py = np.rint((yx[:, 0] - min_y) / scale).astype(np.int64)              # np.rint: ties to even, as Python's round
        px = np.rint((yx[:, 1] - min_x) / scale).astype(np.int64)
        keep = (py >= 0) & (py < height) & (px >= 0) & (px < width)
        mask[py[keep], px[keep]] = 1
    return mask, (min_x, max_x, min_y, max_y)


class ClearanceMap:
    """The drop-in for the reference's SemanticMap2DCollisionDetector, on the GPU.  Holds d2 (int32 [ny, nx] on the device, uint32
    valued: -1 reads SGS_CLEARANCE_NONE), the frame that maps positions to pixels, and the limit d2 <= max_d2 that stands for the
    robot radius.  Single checks return a Python bool (one launch and eight bytes back each); check_positions / check_paths answer a
    batch in one launch."""

    def __init__(self, renderer, d2, frame: ClearanceFrame, counts, robot_radius_m: float, map_path=None):
        self._r, self.d2, self.frame, self.robot_radius_m, self.scale = renderer, d2, frame, float(robot_radius_m), float(frame.scale)
        self.map_path = map_path
        self.map_height, self.map_width = int(d2.shape[0]), int(d2.shape[1])
        self.min_x, self.max_x, self.min_y, self.max_y = frame.min_x, frame.max_x, frame.min_y, frame.max_y
        self._counts = [int(v) & 0xFFFFFFFF for v in counts.cpu().tolist()]

    @staticmethod
    def _limit(robot_radius_m, scale):
        return max(0, inflation_limit(robot_radius_m, scale))                    # the reference does not inflate at a radius <= 0

    @classmethod
    def from_semantic_map(cls, path, robot_radius_m: float = 0.1, scale: float = 0.05, renderer=None):
        """The detector of a semantic map JSON: the mask is made on the host (load_semantic_map), uploaded, and d2 computed once."""
        import torch
        from .renderer import default_renderer
        r = default_renderer() if renderer is None else renderer
        mask, (min_x, max_x, min_y, max_y) = load_semantic_map(path, scale)
        limit = cls._limit(robot_radius_m, scale)
        d2, counts = r.clearance_map(torch.from_numpy(mask).to(r.device), max_d2=limit)
        return cls(r, d2, ClearanceFrame(min_x, min_y, max_x, max_y, scale, max_d2=limit), counts, robot_radius_m, str(path))

    @classmethod
    def from_topdown(cls, grid, topdown_grid, robot_radius_m: float, min_hits: int = 1, unseen_blocks: bool = False, renderer=None):
        """The detector of a seen map: `grid` the TopdownGrid, `topdown_grid` the int32 [ny, nx, 2] tensor Renderer.topdown_map
        accumulated.  Positions are map coordinates as they are (no negation, no flips); pixel (0, 0) is the centre of cell (0, 0),
        so a position is looked up in the cell whose centre is nearest."""
        from .renderer import default_renderer
        r = default_renderer() if renderer is None else renderer
        s = float(grid.cell_size)
        limit = cls._limit(robot_radius_m, s)
        d2, counts = r.clearance_map(topdown_grid, min_hits=min_hits, unseen_blocks=unseen_blocks, max_d2=limit)
        min_x, min_y = float(grid.origin_x) + 0.5 * s, float(grid.origin_y) + 0.5 * s
        frame = ClearanceFrame(min_x, min_y, min_x + (int(grid.nx) - 1) * s, min_y + (int(grid.ny) - 1) * s, s,
                               negate_xy=False, flip_x=False, flip_y=False, max_d2=limit)
        return cls(r, d2, frame, counts, robot_radius_m)

    # -- the batch forms -----------------------------------------------------------------------------------------------------------
    def check_paths(self, starts, ends, num_samples: int = 10) -> np.ndarray:
        """bool [n]: whether a path from starts[k] to ends[k] ([n, 2] or [n, 3]; z is not looked at) collides, sampled as
        check_path_collision_3d samples it.  One launch."""
        a, b = np.asarray(starts, np.float64), np.asarray(ends, np.float64)
        if a.ndim != 2 or a.shape != b.shape or a.shape[1] < 2:
            raise ValueError("starts and ends must be [n, 2] or [n, 3] arrays of one shape")
        if len(a) == 0:
            return np.zeros(0, bool)
        out = self._r.clearance_query(self.d2, self.frame, np.concatenate([a[:, :2], b[:, :2]], 1), num_samples)
        return out[:, 0].cpu().numpy() != 0

    def check_positions(self, xy) -> np.ndarray:
        """bool [n]: check_collision_3d of every row of xy ([n, 2] or [n, 3]).  One launch."""
        p = np.asarray(xy, np.float64)
        return self.check_paths(p, p, 1)

    # -- the reference's interface ---------------------------------------------------------------------------------------------------
    def check_collision_3d(self, pos_3d) -> bool:
        return bool(self.check_positions(np.asarray(pos_3d, np.float64).reshape(1, -1))[0])

    def check_path_collision_3d(self, start_pos_3d, end_pos_3d, num_samples: int = 10) -> bool:
        return bool(self.check_paths(np.asarray(start_pos_3d, np.float64).reshape(1, -1), np.asarray(end_pos_3d, np.float64).reshape(1, -1),
                                     num_samples)[0])

    def check_collision_at_position(self, x: float, y: float) -> bool:
        return self.check_collision_3d([x, y, 0.0])

    def geodesic_field(self, goals_xy):
        """How far every cell is from the nearest of goals_xy ([n, 2] or [n, 3] positions as the checks above take them) when the
        grown obstacles have to be walked round: a sage_gs.geodesic.GeodesicField of this map."""
        from .geodesic import GeodesicField
        return GeodesicField.from_clearance(self, goals_xy=goals_xy)

    def free_regions(self):
        """The 8-connected regions of the cells an agent can stand on (d2 > the inflation limit): a sage_gs.regions.Regions of this
        map, computed on the device at the first call and kept.  Two free cells have a path exactly when they share a label."""
        if getattr(self, "_free_regions", None) is None:
            from .regions import Regions
            self._free_regions = Regions.of(self.d2, renderer=self._r, source="d2", lo=int(self.frame.max_d2) + 1)
        return self._free_regions

    def same_region(self, a_xy, b_xy) -> np.ndarray:
        """bool [n]: whether positions a_xy[k] and b_xy[k] ([n, 2] or [n, 3], mapped to pixels as the checks map them, not clamped)
        both lie on free cells of one region — whether a walk between them exists at all.  One gather on the device."""
        return self.free_regions().same(self.cells_of(a_xy), self.cells_of(b_xy))

    def nearest_free(self, item_set, towards=None, items=None, max_search_dist: int = 50) -> np.ndarray:
        """For items of a sage_gs.trajectory.ItemSet the nearest cell an agent can stand on, on the side that faces a target: a record
        array of (x, y, d, n_at_d), (-1, -1, -1, 0) for none — sage_gs.trajectory.nearest_free on this map's d2."""
        from .trajectory import nearest_free
        return nearest_free(item_set, self, towards, items, max_search_dist)

    def cells_of(self, xy) -> np.ndarray:
        """int64 [n, 2] = (i, j): the pixel of every position of xy, mapped and rounded as the queries map and round it (negation,
        flips, rint of a true division); not clamped — a position outside the map gives a cell outside 0 .. width - 1, 0 .. height - 1."""
        p = np.asarray(xy, np.float64).reshape(-1, np.asarray(xy).shape[-1])[:, :2].copy()
        f = self.frame
        if f.negate_xy:
            p = -p
        if f.flip_x:
            p[:, 0] = (float(f.min_x) + float(f.max_x)) - p[:, 0]
        if f.flip_y:
            p[:, 1] = (float(f.min_y) + float(f.max_y)) - p[:, 1]
        return np.stack([np.rint((p[:, 0] - f.min_x) / f.scale), np.rint((p[:, 1] - f.min_y) / f.scale)], 1).astype(np.int64)

    @property
    def obstacle_map(self) -> np.ndarray:
        """uint8 [height, width]: 1 where the grown obstacles are — the reference's obstacle_map after inflation."""
        d = self.d2.cpu().numpy().view(np.uint32)
        return (d <= np.uint32(self.frame.max_d2)).astype(np.uint8)

    def get_collision_info(self) -> dict:
        total = self.map_height * self.map_width
        grown = self._counts[0] + self._counts[1]
        return {"map_path": self.map_path, "robot_radius_m": self.robot_radius_m, "scale": self.scale,
                "map_bounds": {"x": [self.min_x, self.max_x], "y": [self.min_y, self.max_y]},
                "map_size": [self.map_height, self.map_width], "obstacle_pixels": grown, "total_pixels": total,
                "obstacle_ratio": float(grown) / total}
