#!/usr/bin/env python3
"""Writes tests/golden/geodesic_golden.json: what the reference's OWN astar_pixel and generate_trajectory_points
(Code/data_pipeline/trajectory_generation/vln_trajectory_generator.py) return on small synthetic grids of this project's making.

    python tests/golden/make_geodesic_golden.py /path/to/the/reference/checkout

It needs the reference's checkout and what its module imports (NumPy, SciPy, requests), and runs where they are; the tests read only the
JSON.  The grids (<= 96 x 72): the three rooms of clearance_golden.json as the reference's detector inflated them at two radii (read from
that file), a serpentine maze, a room with a sealed closet, and a wall pierced only by a diagonal gap — the maker asserts that the
reference walks through it, so corner cutting is pinned.  Per grid: five goals x thirty seeded free starts, the returned path (as the
start and one digit per step, the index of the step in the reference's own order of directions) or null, and for two paths the
trajectory points at sample_step 1 and 3.  Only DATA is written; no reference source text is copied."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))
RADII = ("0.1", "0.15")
N_GOALS, N_STARTS = 5, 30


def serpentine_maze(nx=40, ny=31):
    """Corridors two cells wide between walls one cell thick, open at alternating ends."""
    ob = np.zeros((ny, nx), np.uint8)
    ob[0], ob[-1], ob[:, 0], ob[:, -1] = 1, 1, 1, 1
    for k, j in enumerate(range(3, ny - 1, 3)):
        ob[j, :] = 1
        if k % 2 == 0:
            ob[j, nx - 3:nx - 1] = 0
        else:
            ob[j, 1:3] = 0
    return ob


def closet_room(nx=44, ny=30):
    """A room with a closet whose walls are closed: the cells inside are free and cannot be reached from the room."""
    ob = np.zeros((ny, nx), np.uint8)
    ob[0], ob[-1], ob[:, 0], ob[:, -1] = 1, 1, 1, 1
    ob[8:20, 28:40] = 1
    ob[9:19, 29:39] = 0
    ob[14, 5:20] = 1
    return ob


def diagonal_gap(nx=24, ny=16):
    """A wall in column 10 down to row 7 and in column 11 from row 8 on: the only way through is the diagonal step (10, 8) <-> (11, 7),
    whose two orthogonal cells (10, 7) and (11, 8) are wall."""
    ob = np.zeros((ny, nx), np.uint8)
    ob[:8, 10] = 1
    ob[8:, 11] = 1
    return ob


def grids():
    with open(os.path.join(HERE, "clearance_golden.json")) as fh:
        g = json.load(fh)
    out = []
    for e in g["maps"]:
        for radius in RADII:
            ob = np.array([[int(c) for c in row] for row in e["obstacle_map"][radius]], np.uint8)
            out.append((f"{e['name']}_r{radius}", ob, e["scale"], e["bounds"][0], e["bounds"][2]))
    out.append(("serpentine_maze", serpentine_maze(), 0.05, 0.0, 0.0))
    out.append(("closet_room", closet_room(), 0.05, -1.1, 0.35))
    out.append(("diagonal_gap", diagonal_gap(), 0.1, 0.25, -0.4))
    return out


def encode(path):
    return "".join(str(DIRS.index((b[0] - a[0], b[1] - a[1]))) for a, b in zip(path[:-1], path[1:]))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SAGE3D_REFERENCE", "")
    sys.path.insert(0, os.path.join(ref, "Code", "data_pipeline", "trajectory_generation"))
    from vln_trajectory_generator import astar_pixel, generate_trajectory_points
    out = {"grids": []}
    for seed, (name, ob, scale, min_x, min_y) in enumerate(grids()):
        ny, nx = ob.shape
        assert nx <= 96 and ny <= 72
        rs = np.random.RandomState(500 + seed)
        free = [(int(i), int(j)) for j, i in np.argwhere(ob == 0)]
        goals = [free[k] for k in rs.choice(len(free), N_GOALS, replace=False)]
        if name == "closet_room":
            goals[0], goals[1] = (33, 13), (2, 2)                               # one goal inside the closet, one in the room
        if name == "diagonal_gap":
            goals[0], goals[1] = (2, 12), (20, 3)                               # one goal on either side of the wall
        entry = {"name": name, "grid": ["".join(str(int(v)) for v in row) for row in ob], "scale": scale, "min_x": min_x, "min_y": min_y,
                 "goals": [], "trajectories": []}
        n_found = n_none = 0
        for goal in goals:
            starts = [free[k] for k in rs.choice(len(free), N_STARTS, replace=False)]
            starts[0] = goal                                                       # a path of one cell
            pairs = []
            for s in starts:
                p = astar_pixel(ob, s, goal)
                if p is None:
                    n_none += 1
                else:
                    n_found += 1
                    p = [(int(x), int(y)) for x, y in p]
                    assert p[0] == s and p[-1] == goal
                    if name == "diagonal_gap" and (s[0] <= 10) != (goal[0] <= 10) and not (s[0] == 10 and s[1] < 8) and not (goal[0] == 10 and goal[1] < 8):
                        k = p.index((10, 8))
                        assert (11, 7) in (p[k - 1] if k else None, p[k + 1] if k + 1 < len(p) else None), "the reference does not cut the corner"
                    if len(entry["trajectories"]) < 2 and 8 <= len(p) <= 30:
                        step = (1, 3)[len(entry["trajectories"])]
                        pts = generate_trajectory_points(p, scale, min_x, min_y, 0.5, step)
                        entry["trajectories"].append({"start": list(s), "path": encode(p), "fixed_z": 0.5, "sample_step": step,
                                                      "points": [{"position": q["position"], "rotation": q["rotation"]} for q in pts]})
                pairs.append({"start": list(s), "path": None if p is None else encode(p)})
            entry["goals"].append({"goal": list(goal), "pairs": pairs})
        assert n_found > 0 and len(entry["trajectories"]) == 2, name
        if name in ("closet_room",):
            assert n_none >= 20, (name, n_none)
        if name == "diagonal_gap":
            assert n_none == 0
        entry["found"], entry["none"] = n_found, n_none
        out["grids"].append(entry)
    dst = os.path.join(HERE, "geodesic_golden.json")
    with open(dst, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    assert os.path.getsize(dst) < 200 * 1024
    print(dst, os.path.getsize(dst), "bytes")
    for e in out["grids"]:
        print(e["name"], len(e["grid"][0]), "x", len(e["grid"]), "found", e["found"], "none", e["none"])


if __name__ == "__main__":
    main()
