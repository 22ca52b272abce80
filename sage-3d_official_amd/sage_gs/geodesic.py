"""How far one place is from another when walls have to be walked round: geodesic distance fields and shortest paths on the GPU
(include/sage_gs.h sgs_geodesic_field, sgs_geodesic_path) behind the interface of the reference's trajectory planner.

The reference (vln_trajectory_generator.py) plans every trajectory with a pure-Python A* over the grid the clearance map holds —
walls and 'Unable Area' cells grown by the robot radius —, one search per (start item, end item) pair.  A GeodesicField is computed
once per goal on the device and answers every start cell of the map: the pair (a, b) of straight and diagonal steps of the cheapest
8-connected walk, exact in integers, and the walk itself.
"""
from __future__ import annotations

import math

import numpy as np

from . import _capi

NONE = _capi.GEODESIC_NONE
SQRT2 = math.sqrt(2.0)


class GeodesicField:
    """The field of one set of goals on one map.  `steps` is uint32 [ny, nx, 2] on the host, (a, b) per cell, NONE in both words
    where a cell is blocked or cannot reach a goal; the device copy stays for the paths."""

    def __init__(self, renderer, src, max_d2, steps_dev, goals, blocked_goals, scale=None):
        self._r, self._src, self._max_d2, self._dev = renderer, src, max_d2, steps_dev
        self.goal_cells = [tuple(int(v) for v in g) for g in goals]
        self.blocked_goals = int(blocked_goals)
        self.scale = None if scale is None else float(scale)
        self.steps = steps_dev[0].cpu().numpy().view(np.uint32)
        self.ny, self.nx = self.steps.shape[:2]

    @classmethod
    def _make(cls, renderer, src, max_d2, goal_cells, scale):
        goals = np.asarray(goal_cells, np.int64).reshape(-1, 2)
        if len(goals) < 1:
            raise ValueError("at least one goal cell")
        seeds = np.concatenate([np.zeros((len(goals), 1), np.int64), goals], 1)
        steps, blocked = renderer.geodesic_field(src, seeds, max_d2=max_d2)
        return cls(renderer, src, max_d2, steps, goals, blocked[0], scale)

    @classmethod
    def from_clearance(cls, clearance_map, goals_xy=None, goal_cells=None):
        """The field on a sage_gs.clearance.ClearanceMap: blocked where d2 <= its inflation limit — the reference's grid_map.  Goals
        as positions (goals_xy, mapped to cells as the map's checks map them) or as cells (goal_cells, (i, j))."""
        if (goals_xy is None) == (goal_cells is None):
            raise ValueError("give goals_xy or goal_cells")
        cells = clearance_map.cells_of(goals_xy) if goal_cells is None else goal_cells
        return cls._make(clearance_map._r, clearance_map.d2, int(clearance_map.frame.max_d2), cells, clearance_map.scale)

    @classmethod
    def from_mask(cls, mask, goal_cells, renderer=None, scale=None):
        """The field on a mask (anything np.asarray takes, or a uint8 / bool tensor on the device): non-zero is blocked."""
        import torch
        from .renderer import default_renderer
        r = default_renderer() if renderer is None else renderer
        src = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0)).to(r.device)
        return cls._make(r, src, None, goal_cells, scale)

    def distance_cells(self) -> np.ndarray:
        """float64 [ny, nx]: a + b sqrt(2), inf where no goal can be reached."""
        s = self.steps.astype(np.float64)
        return np.where(self.steps[..., 0] == NONE, np.inf, s[..., 0] + s[..., 1] * SQRT2)

    def distance_m(self) -> np.ndarray:
        if self.scale is None:
            raise ValueError("this field has no scale")
        return self.distance_cells() * self.scale

    def paths(self, start_cells):
        """[path or None]: per start cell (i, j) the list of (i, j) cells to a goal, the start first; None where the start is
        blocked, outside the map or cannot reach a goal."""
        starts = np.asarray(start_cells, np.int64).reshape(-1, 2)
        if len(starts) == 0:
            return []
        inside = (starts[:, 0] >= 0) & (starts[:, 0] < self.nx) & (starts[:, 1] >= 0) & (starts[:, 1] < self.ny)
        s = self.steps[np.where(inside, starts[:, 1], 0), np.where(inside, starts[:, 0], 0)].astype(np.int64)
        length = np.where(inside & (s[:, 0] != NONE), s[:, 0] + s[:, 1] + 1, 1)
        q = np.concatenate([np.zeros((len(starts), 1), np.int64), np.where(inside[:, None], starts, -1)], 1)
        cells, info = self._r.geodesic_path(self._src, self._dev, q, max_d2=self._max_d2, max_len=int(length.max()))
        cells, info = cells.cpu().numpy(), info.cpu().numpy()
        if (info[:, 1] == _capi.GEODESIC_PATH_NOT_FINAL).any() or (info[:, 1] == _capi.GEODESIC_PATH_TRUNCATED).any():
            raise RuntimeError("geodesic_path: the field is not final")
        return [[(int(x), int(y)) for x, y in c[:n]] if st == _capi.GEODESIC_PATH_OK else None for c, (n, st) in zip(cells, info)]

    def path(self, start_cell):
        return self.paths([start_cell])[0]


def astar_pixel(grid, start, goal, renderer=None):
    """The drop-in for the reference's astar_pixel(grid, start, goal): grid [H, W] with 1 (non-zero) for a blocked cell, start and goal
    (x, y); a list of (x, y) from start to goal, or None.  One field seeded at `goal` plus one path from `start`, on the GPU.
    Among equal-cost paths it may return ANOTHER one than the reference does; the numbers of straight and diagonal steps are the
    same (the cheapest pair is unique).  DEPARTURES: a blocked or outside `start` returns None (the reference never looks at the
    start cell and would walk out of it), and so does a blocked `goal`."""
    f = GeodesicField.from_mask(grid, [goal], renderer=renderer)
    return f.path(start)


def trajectory_points(path, scale, min_x, min_y, fixed_z=0.5, sample_step=1):
    """The positions and rotations of the reference's generate_trajectory_points for a path of (x, y) cells: a list of
    {"position": [x, y, z], "rotation": [0, 0, qz, qw]} — the cell centre min + (p + 0.5) * scale of every sample_step-th cell, the
    yaw atan2 towards the next sample, the last sample facing itself (yaw 0).  Host arithmetic in float64, written from the formulae."""
    xs = [min_x + (x + 0.5) * scale for x, _ in path][::sample_step]
    ys = [min_y + (y + 0.5) * scale for _, y in path][::sample_step]
    out = []
    for k in range(len(xs)):
        n = k + 1 if k + 1 < len(xs) else k
        yaw = math.atan2(ys[n] - ys[k], xs[n] - xs[k])
        out.append({"position": [xs[k], ys[k], fixed_z], "rotation": [0.0, 0.0, math.sin(yaw / 2.0), math.cos(yaw / 2.0)]})
    return out
