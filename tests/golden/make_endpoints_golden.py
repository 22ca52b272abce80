#!/usr/bin/env python3
"""Writes tests/golden/endpoints_golden.json: what the reference's OWN trajectory generator
(Code/data_pipeline/trajectory_generation/vln_trajectory_generator.py) answers on two synthetic scenes of this project's making.

    python tests/golden/make_endpoints_golden.py /path/to/the/reference/checkout

It needs the reference's checkout and what its module imports, and runs where they are; the tests read only the JSON.  A scene is a
2-D semantic map (a list of instances with `category_label` and `mask_coords_m`) of at most 96 x 72 cells at 0.05 m.  Per scene the
maker calls build_2d_map (robot radius 0.2 m), and on the grid it returns instance_centroid_px and boundary_pixels per item,
get_nearest_free_pixel_on_side per query, build_connectivity_map, and validate_and_generate_path per recorded pair.  Recorded: the
instances, the grid (a hex string per row), per item its pixel list, centroid and boundary count, per query the reference's answer and
its L1 distance to the boundary (computed here by brute force), the connectivity groups, and the whole dict of the recorded pairs.

"rooms": two rooms joined by a door and a sealed closet; items in open floor, hugging a straight wall, in a corner, straddling a wall,
one with two pixels whose mean lands on .5 in both axes, a one-pixel item on each grid edge, a 5 x 3 item queried with targets exactly
perpendicular to it, one-pixel items in a row and on a diagonal (their endpoints are forced and the straight walk between two of them is
the only cheapest one, so the reference's whole trajectory is pinned), and two one-pixel items in the closet (forced endpoints, no path).
"walled": unable cells on a lattice that the radius grows into one block, everything but two far corners; six items in the middle are walled in farther than 50 cells, two lie
within reach of a corner.

The maker asserts what keeps the tests honest (see the asserts at the end of main).  Only DATA is written; no reference source text is
copied."""
import contextlib
import io
import json
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import endpoints_ref as ref  # noqa: E402

SCALE, RADIUS = 0.05, 0.2
W, H = 96, 72


def metres(pixels, min_x, min_y, nudge=0.0):
    """[[y, x]] in metres, as strings with two decimals, of (y, x) pixels."""
    return [[f"{min_y + y * SCALE + nudge:.2f}", f"{min_x + x * SCALE + nudge:.2f}"] for y, x in pixels]


def box(x0, y0, x1, y1):
    return [(y, x) for y in range(y0, y1) for x in range(x0, x1)]


def rooms():
    wall = box(0, 0, W, 1) + box(0, H - 1, W, H) + box(0, 0, 1, H) + box(W - 1, 0, W, H)
    wall += [(y, 48) for y in range(H) if not 14 <= y <= 26]                        # the wall between the rooms, with a door
    wall += [(y, 70) for y in range(44, H)] + [(44, x) for x in range(70, W)]       # the closet: no door
    items = {f"row_{k}": [(20, 10 + 5 * k)] for k in range(5)}
    items.update({f"diag_{k}": [(8 + 5 * k, 56 + 5 * k)] for k in range(3)})
    items.update({"closet_0": [(58, 82)], "closet_1": [(60, 80)], "open": box(20, 40, 26, 44), "hug": box(1, 50, 4, 56), "corner": box(1, 66, 4, 70),
                  "straddle": box(45, 34, 52, 37), "half": [(50, 30), (53, 31)], "edge_top": [(0, 40)], "edge_bottom": [(H - 1, 40)],
                  "edge_left": [(30, 0)], "edge_right": [(30, W - 1)], "perp": box(60, 30, 65, 33)})
    extra = [("perp", (72, 31)), ("perp", (52, 31)), ("perp", (62, 5)), ("perp", (62, 60)), ("open", (22, 60)), ("open", (80, 42))]
    return "rooms", [("wall", wall)], items, extra, (-2.4, 1.1)


def walled():
    # a lattice of unable cells 5 apart: grown by the radius (4 cells) it covers everything but the two pockets
    pockets = set(box(0, 0, 11, 11)) | set(box(W - 11, H - 11, W, H))
    unable = [(y, x) for (y, x) in box(0, 0, W, H) if x % 5 == 0 and (y % 5 == 0 or y == H - 1) and (y, x) not in pockets]
    items = {f"far_{k}": [c] for k, c in enumerate([(36, 40), (36, 44), (36, 48), (36, 52), (30, 46)])}
    items.update({"far_5": box(49, 39, 52, 42), "near_0": [(20, 20)], "near_1": [(50, 75)], "in_pocket": [(5, 6), (5, 6), (6, 6)]})
    return "walled", [("Unable Area", unable)], items, [], (0.35, -3.0)


def l1_field(boundary):
    """int64 [H, W]: min over B of |dx| + |dy|, by brute force."""
    ys, xs = np.mgrid[:H, :W]
    return np.min([np.abs(xs - bx) + np.abs(ys - by) for (by, bx) in boundary], axis=0)


def main(reference):
    sys.path.insert(0, os.path.join(reference, "Code", "data_pipeline", "trajectory_generation"))
    with contextlib.redirect_stdout(io.StringIO()):
        import vln_trajectory_generator as gen
    scenes = []
    n_forced_towards = n_none = n_path = n_no_path = 0
    for name, obstacles, items, extra, (min_x, min_y) in (rooms(), walled()):
        instances = [{"category_label": label, "instance_id": f"{label}_{k}", "mask_coords_m": metres(px, min_x, min_y)} for k, (label, px) in enumerate(obstacles)]
        for item, px in items.items():
            coords = metres(px, min_x, min_y)
            if item == "in_pocket":                                                  # two coordinates that round to one pixel
                coords[1] = metres(px[1:2], min_x, min_y, nudge=0.01)[0]
            instances.append({"category_label": "chair", "instance_id": item, "mask_coords_m": coords})
        sem = json.loads(json.dumps(instances))
        grid, scale, gx, gy = gen.build_2d_map(sem, SCALE, RADIUS)
        assert grid is not None and grid.shape == (H, W) and scale == SCALE
        inst = {i["instance_id"]: i for i in sem if i["category_label"] == "chair"}
        for item, px in items.items():
            assert inst[item]["mask_coords"] == px, item
        free = grid == 0
        out_items = {}
        for item, i in inst.items():
            b = gen.boundary_pixels(i["mask_coords"])
            out_items[item] = {"mask_coords": [list(c) for c in i["mask_coords"]], "centroid": list(gen.instance_centroid_px(i["mask_coords"])), "n_boundary": len(b)}
        cent = {item: tuple(v["centroid"]) for item, v in out_items.items()}
        queries = [(a, None) for a in inst] + [(a, cent[b]) for a in inst for b in inst if a != b] + extra
        out_queries, forced = [], {}
        for item, towards in queries:
            mc = inst[item]["mask_coords"]
            answer = gen.get_nearest_free_pixel_on_side(mc, grid, towards_px=towards)
            cells = [y * W + x for y, x in mc]
            mine, cands = ref.query(free, cells, 50, towards)
            rec = {"item": item, "towards": None if towards is None else list(towards), "answer": None if answer is None else [int(v) for v in answer]}
            if answer is None:
                assert mine == ref.NONE, (name, item, towards)
                n_none += 1
            else:
                b = gen.boundary_pixels(mc)
                dist = l1_field(b)
                rec["d"] = int(dist[answer[1], answer[0]])
                assert rec["d"] == mine[2] and tuple(answer) in cands, (name, item, towards, answer, mine)
                if towards is not None:
                    # No cell within d* has a float dot whose sign differs from the exact one.  Where the exact dot is beyond 1 in
                    # size, float64 cannot lose its sign; the others are put through the reference's own expression.
                    m = np.mean([(px, py) for (py, px) in mc], axis=0)
                    n, sx, sy = len(mc), sum(x for _, x in mc), sum(y for y, _ in mc)
                    ys, xs = np.nonzero(dist <= rec["d"])
                    exact = (n * xs - sx) * (n * towards[0] - sx) + (n * ys - sy) * (n * towards[1] - sy)
                    for x, y, e in zip(xs.tolist(), ys.tolist(), exact.tolist()):
                        if abs(e) > n * n:
                            continue
                        fl = np.dot(np.array([x - m[0], y - m[1]]), np.array([towards[0] - m[0], towards[1] - m[1]]))
                        ex = (Fraction(x) - Fraction(sx, n)) * (Fraction(towards[0]) - Fraction(sx, n)) + (Fraction(y) - Fraction(sy, n)) * (Fraction(towards[1]) - Fraction(sy, n))
                        assert ex * n * n == e and (fl >= 0) == (ex >= 0), (name, item, towards, x, y)
                    if len(cands) == 1:
                        n_forced_towards += 1
                        forced[(item, towards)] = tuple(answer)
            out_queries.append(rec)
        # connectivity: every item's candidates (no target) lie in one 4-connected component, so the groups do not hang on the tie
        groups = gen.build_connectivity_map(grid, inst)
        for item, i in inst.items():
            _, cands = ref.query(free, [y * W + x for y, x in i["mask_coords"]], 50, None)
            comps = set()
            for (x, y) in cands:
                seen, stack = {(x, y)}, [(x, y)]
                while stack:
                    cx, cy = stack.pop()
                    for nx_, ny_ in ((cx - 1, cy), (cx + 1, cy), (cx, cy - 1), (cx, cy + 1)):
                        if 0 <= nx_ < W and 0 <= ny_ < H and free[ny_, nx_] and (nx_, ny_) not in seen:
                            seen.add((nx_, ny_))
                            stack.append((nx_, ny_))
                comps.add(min(seen))
            assert len(comps) <= 1, (name, item, comps)
        # pairs: both endpoints forced; a path that is one straight walk (the only cheapest one), or none
        pairs = []
        for a in inst:
            for b in inst:
                if a == b or (a, cent[b]) not in forced or (b, cent[a]) not in forced:
                    continue
                with contextlib.redirect_stdout(io.StringIO()):
                    got = gen.validate_and_generate_path(a, b, inst, grid, scale, gx, gy)
                if got is None:
                    pairs.append({"start": a, "end": b, "result": None})
                    n_no_path += 1
                    continue
                pts = [p["position"] for p in got["points"]]
                steps = {(round((q[0] - p[0]) / scale), round((q[1] - p[1]) / scale)) for p, q in zip(pts[:-1], pts[1:])}
                if len(steps) == 1 and len(pts) <= 22:
                    pairs.append({"start": a, "end": b, "result": got})
                    n_path += 1
        scenes.append({"name": name, "scale": scale, "robot_radius_m": RADIUS, "min": [gx, gy], "width": W, "height": H, "instances": instances,
                       "grid": [bytes(row.tolist()).hex() for row in grid], "items": out_items, "queries": out_queries,
                       "connectivity": sorted(sorted(g) for g in groups.values()), "pairs": pairs})
    assert n_forced_towards >= 40, n_forced_towards
    assert n_none >= 20, n_none
    assert n_path >= 20 and n_no_path >= 5, (n_path, n_no_path)
    half = scenes[0]["items"]["half"]
    assert half["centroid"] == [30, 52], half["centroid"]                             # 30.5 and 51.5: half to even
    path = os.path.join(HERE, "endpoints_golden.json")
    with open(path, "w") as fh:
        json.dump({"scenes": scenes}, fh, separators=(",", ":"))
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print(f"{path}: {size} bytes; {n_forced_towards} forced answers with a target, {n_none} None, {n_path} forced pairs with a path, {n_no_path} without")


if __name__ == "__main__":
    main(sys.argv[1])
