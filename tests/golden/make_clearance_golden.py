#!/usr/bin/env python3
"""Writes tests/golden/clearance_golden.json: what the reference's OWN SemanticMap2DCollisionDetector
(Code/benchmark/environment_evaluation/collision_detector.py) answers on three small synthetic semantic maps of this project's making.

    python tests/golden/make_clearance_golden.py /path/to/the/reference/checkout

It needs the reference's checkout and SciPy (which the detector imports), and runs where both are; the tests read only the JSON.  Per
map the file holds the map itself (the JSON the detector loads), the bounds and size the detector derived, and for each robot radius
in RADII its obstacle_map after inflation (rows of '0' / '1'), its check_collision_3d answers at seeded positions — inside, on the
border pixel, within the 2-pixel margin, just beyond it, far outside — and its check_path_collision_3d answers on seeded segments with
num_samples 1, 2 and 10, some of them across the interior wall.  Non-finite inputs are left out: there sgs_clearance_query departs
from the reference on purpose (include/sage_gs.h).  Only DATA is written; no reference source text is copied."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RADII = (0.0, 0.1, 0.12, 0.15, 0.25)


def r3(v):
    return round(float(v), 4)


def room(nx, ny, scale, x0, y0, wall_col, gap, block, seed):
    """A walled room of nx x ny cells whose cell (0, 0) lies at (x0, y0): an interior wall in column wall_col with a gap of rows
    `gap`, an 'Unable Area' block, a floor of every third cell that is no obstacle — and reaches one cell beyond the east wall, so
    that the bounds are not the walls' —, and wall points that sit exactly half-way between two pixels."""
    at = lambda i, j: [r3(y0 + j * scale), r3(x0 + i * scale)]                  # (y, x), as mask_coords_m holds them   # noqa: E731
    border = [at(i, j) for j in range(ny) for i in range(nx) if i in (0, nx - 1) or j in (0, ny - 1)]
    inner = [at(wall_col, j) for j in range(1, ny - 1) if not gap[0] <= j < gap[1]]
    # half-way points: (v - min) / scale = k + 0.5 for an even and an odd k, on otherwise free rows
    half = [[r3(y0 + (ny // 2) * scale), x0 + 4.5 * scale], [r3(y0 + (ny // 2 + 3) * scale), x0 + 7.5 * scale],
            [y0 + 2.5 * scale, r3(x0 + 5 * scale)], [y0 + 5.5 * scale, r3(x0 + 9 * scale)]]
    bi, bj, bw, bh = block
    unable = [at(i, j) for j in range(bj, bj + bh) for i in range(bi, bi + bw)]
    floor = [at(i, j) for j in range(1, ny - 1, 3) for i in range(1, nx + 1, 3)]
    rs = np.random.RandomState(seed)
    chairs = [at(int(rs.randint(2, nx - 2)), int(rs.randint(2, ny - 2))) for _ in range(6)]
    return [{"category_label": "wall", "mask_coords_m": border}, {"category_label": "Wall", "mask_coords_m": inner + half},
            {"category_label": "Unable Area", "mask_coords_m": unable}, {"category_label": "floor", "mask_coords_m": floor},
            {"category_label": "chair", "mask_coords_m": chairs}]


MAPS = {
    "room_48x36": dict(scale=0.05, instances=room(48, 36, 0.05, 0.0, 0.0, 20, (14, 20), (30, 8, 5, 4), 1)),
    "room_60x40_offset": dict(scale=0.05, instances=room(59, 40, 0.05, -1.3, 2.15, 33, (5, 9), (6, 25, 7, 6), 2)),
    "room_23x17_coarse": dict(scale=0.1, instances=room(22, 17, 0.1, 0.5, -0.8, 9, (7, 10), (14, 3, 3, 3), 3)),
}


def probes(det, seed):
    """3-D positions and segments whose MAP coordinates are chosen (the detector negates and flips: x3d = x2d - (min + max))."""
    rs = np.random.RandomState(seed)
    s, h, w = det.scale, det.map_height, det.map_width
    sx, sy = det.min_x + det.max_x, det.min_y + det.max_y
    to3d = lambda x, y: [float(x - sx), float(y - sy), 0.5]                     # noqa: E731
    pix = lambda px, py: (det.min_x + px * s, det.min_y + py * s)               # noqa: E731
    pos = [to3d(*pix(rs.uniform(0, w - 1), rs.uniform(0, h - 1))) for _ in range(60)]
    for px, py in ((0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0), (w // 2, 0), (0, h // 2),                     # the border pixels
                   (-1, 3), (-2, 3), (3, -1.6), (w, 3), (w + 1, h + 1), (w + 1.4, 5), (5, h + 0.7), (-1.2, -2),   # within the margin
                   (-2.6, 3), (-3, 3), (3, -2.7), (w + 2, 3), (w + 1.6, 3), (3, h + 2), (-3, -3), (w + 2.2, h + 2.2),   # just beyond it
                   (-40, 3), (3, 500), (1e6, 1e6), (-1e9, 2),                                                      # far outside
                   (4.5, h // 2), (7.5, h // 2 + 3), (5, 2.5), (9, 5.5), (2.5, 3.5), (3.5, 2.5)):                  # half-way
        pos.append(to3d(*pix(px, py)))
    segs = []
    for k in range(48):
        a = pix(rs.uniform(1, w - 2), rs.uniform(1, h - 2))
        b = pix(rs.uniform(1, w - 2), rs.uniform(1, h - 2)) if k % 3 else pix(rs.uniform(-4, w + 4), rs.uniform(-4, h + 4))
        segs.append(to3d(*a) + to3d(*b) + [(1, 2, 10)[k % 3] if k < 24 else 10])
    return pos, segs


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SAGE3D_REFERENCE", "")
    os.environ["SILENT_LOGGING_MODE"] = "1"
    sys.path.insert(0, os.path.join(ref, "Code", "benchmark", "environment_evaluation"))
    from collision_detector import SemanticMap2DCollisionDetector as Detector
    out = {"radii": list(RADII), "maps": []}
    with tempfile.TemporaryDirectory() as tmp:
        for seed, (name, m) in enumerate(MAPS.items()):
            path = os.path.join(tmp, name + ".json")
            with open(path, "w") as fh:
                json.dump(m["instances"], fh)
            entry = {"name": name, "scale": m["scale"], "instances": m["instances"], "obstacle_map": {}, "position_hits": {},
                     "segment_hits": {}, "obstacle_pixels": {}}
            for radius in RADII:
                det = Detector(path, robot_radius_m=radius, scale=m["scale"])
                if "bounds" not in entry:
                    entry["bounds"] = [det.min_x, det.max_x, det.min_y, det.max_y]
                    entry["size"] = [det.map_height, det.map_width]
                    assert det.map_width <= 60 and det.map_height <= 40
                    entry["positions"], entry["segments"] = probes(det, 100 + seed)
                key = repr(radius)
                entry["obstacle_map"][key] = ["".join("1" if v else "0" for v in row) for row in det.obstacle_map]
                entry["obstacle_pixels"][key] = det.get_collision_info()["obstacle_pixels"]
                entry["position_hits"][key] = "".join("1" if det.check_collision_3d(np.array(p)) else "0" for p in entry["positions"])
                entry["segment_hits"][key] = "".join(
                    "1" if det.check_path_collision_3d(np.array(s[:3]), np.array(s[3:6]), num_samples=int(s[6])) else "0" for s in entry["segments"])
            out["maps"].append(entry)
    dst = os.path.join(HERE, "clearance_golden.json")
    with open(dst, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print(dst, os.path.getsize(dst), "bytes")
    for e in out["maps"]:
        print(e["name"], e["size"], {k: (v.count("1"), len(v)) for k, v in e["position_hits"].items()},
              {k: v.count("1") for k, v in e["segment_hits"].items()})


if __name__ == "__main__":
    main()
