#!/usr/bin/env python3
"""Writes tests/golden/regions_golden.json: what the reference's OWN build_semantic_maps
(Code/data_pipeline/interiorgs_processing/semantic_map_builder.py) writes for three small synthetic scenes of this project's making.

    python tests/golden/make_regions_golden.py /path/to/the/reference/checkout

It needs the reference's checkout and what its module imports (NumPy, SciPy, Pillow, Matplotlib), and runs where they are; the tests
read only the JSON.  A scene is an occupancy.png (<= 96 x 72), an occupancy.json (scale, min) and a labels.json holding [] — no object
boxes, so the reference's footprint loop never runs.  shapely is not needed for that and may be missing: stand-ins for `shapely` and
`shapely.geometry` are installed whose Point / Polygon raise when called; the maker asserts that they never were.  Recorded per scene:
the image (a hex string per row), scale and min, the wall value the reference printed, and every item it wrote, whole, mask_coords_m
included.  The maker asserts what the scenes are there to show: two grey values of which the rarer is not the wall value; a scene of
0 and 255 alone, whose walls and unable areas coincide; walls that touch only diagonally and form one item; a one-pixel wall; unable
areas of 1, 4 and 5 cells — the first two dropped, the numbering of the rest going on —; a region whose first cell lies further
right than the first cell of a later-numbered one.  Only DATA is written; no reference source text is copied."""
import contextlib
import io
import json
import os
import re
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CALLS = []


def _refuse(name):
    def make(*a, **kw):
        CALLS.append(name)
        raise RuntimeError(f"shapely.geometry.{name} was called: the scenes have no object boxes")
    return make


def install_shapely_stand_ins():
    shapely, geometry = types.ModuleType("shapely"), types.ModuleType("shapely.geometry")
    geometry.Point, geometry.Polygon = _refuse("Point"), _refuse("Polygon")
    shapely.geometry = geometry
    sys.modules["shapely"], sys.modules["shapely.geometry"] = shapely, geometry


# ---- the scenes, drawn as the reference LABELS them (the png is this turned upside down) ------------------------------------------------------
def two_greys():
    """64 x 48: walls of grey 100, three pixels of grey 180, unable areas of 1, 6, 4, 5 and 12 cells in raster order."""
    f = np.full((48, 64), 255, np.uint8)
    f[2, 40:45] = 100                                  # wall 1 starts at x = 40 ...
    f[3:9, 40] = 100
    f[3, 5:12] = 100                                   # ... wall 2 at x = 5, one row later
    f[10, 10:15] = 100                                 # two bars that touch only diagonally: (14, 10) and (15, 11)
    f[11, 15:20] = 100
    f[20, 30] = 100                                    # a one-pixel wall
    f[40, 2:62] = 100
    f[44, 20], f[44, 22], f[45, 21] = 180, 180, 180
    f[5, 50] = 0                                       # 1 cell
    f[15:17, 50:53] = 0                                # 6 cells
    f[25:27, 50:52] = 0                                # 4 cells
    f[30, 50:55] = 0                                   # 5 cells
    f[34:37, 8:12] = 0                                 # 12 cells
    return f, 0.05, [-1.6, 0.4, 0.0]


def binary():
    """40 x 30 of 0 and 255 alone: the wall value falls back to 0."""
    f = np.full((30, 40), 255, np.uint8)
    f[1, 1:39] = 0
    f[2:12, 1] = 0
    f[5, 10] = 0                                       # 1 cell
    f[8:10, 20:22] = 0                                 # 4 cells
    f[14, 5:10] = 0                                    # 5 cells
    f[18:21, 30:33] = 0                                # 9 cells
    for k in range(6):                                 # a staircase of single cells: one region under 8-connectivity
        f[22 + k, 10 + k] = 0
    return f, 0.1, [0.25, -0.75, 0.0]


def rooms():
    """96 x 72: rooms of grey 60 with doors, a few pixels of grey 249, MORE pixels of grey 250 than of 60 (250 is no candidate), and
    zero pixels outside the rooms."""
    f = np.full((72, 96), 255, np.uint8)
    f[4:68, 6:90] = 250
    f[6:66, 8:88] = 255
    f[8, 10:86], f[63, 10:86], f[8:64, 10], f[8:64, 85] = 60, 60, 60, 60
    f[8:64, 40] = 60
    f[35, 10:86] = 60
    f[35, 20:24], f[35, 60:64], f[18:22, 40], f[50:54, 40] = 255, 255, 255, 255      # doors: the walls fall into pieces
    f[20, 60:63] = 249
    f[0, 0:96:2] = 0                                   # single cells
    f[1, 3:9] = 0
    f[70, 30:60] = 0
    f[69, 29], f[71, 60] = 0, 0                        # joined to the bar diagonally
    f[45:48, 55:58] = 0
    return f, 0.05, [-2.4, -1.8, 0.0]


SCENES = (("a_two_greys", two_greys), ("b_binary", binary), ("c_rooms", rooms))


def first_cells(labels, n):
    flat = labels.reshape(-1)
    return [int(np.nonzero(flat == k)[0][0]) for k in range(1, n + 1)]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SAGE3D_REFERENCE", "")
    os.environ.setdefault("MPLBACKEND", "Agg")
    install_shapely_stand_ins()
    sys.path.insert(0, os.path.join(ref, "Code", "data_pipeline", "interiorgs_processing"))
    from PIL import Image
    from scipy.ndimage import label as nd_label
    from semantic_map_builder import build_semantic_maps
    out = {"scenes": []}
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = Path(tmp) / "in", Path(tmp) / "out"
        meta = {}
        for name, draw in SCENES:
            f, scale, lo = draw()
            assert f.shape[1] <= 96 and f.shape[0] <= 72
            png = np.ascontiguousarray(np.flipud(f))
            (src / name).mkdir(parents=True)
            Image.fromarray(png, "L").save(src / name / "occupancy.png")
            (src / name / "occupancy.json").write_text(json.dumps({"scale": scale, "min": lo}))
            (src / name / "labels.json").write_text("[]")
            meta[name] = (png, scale, lo)
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            build_semantic_maps(src, dst, True, None)
        assert not CALLS, CALLS
        for name, _ in SCENES:
            png, scale, lo = meta[name]
            with open(dst / f"2D_Semantic_Map_{name}_Complete.json") as fh:
                items = json.load(fh)
            wall = int(re.search(rf"\[{name}\] wall pixel value = (\d+)", log.getvalue()).group(1))
            out["scenes"].append({"name": name, "width": int(png.shape[1]), "height": int(png.shape[0]),
                                  "occupancy": [bytes(row).hex() for row in png], "scale": scale, "min": lo, "wall_value": wall, "items": items})
    # what the scenes are there to show
    by = {s["name"]: s for s in out["scenes"]}
    eight, four = np.ones((3, 3), int), None

    def flipped(s):
        return np.flipud(np.array([list(bytes.fromhex(r)) for r in s["occupancy"]], np.uint8))

    a, f = by["a_two_greys"], flipped(by["a_two_greys"])
    assert a["wall_value"] == 100 and 0 < (f == 180).sum() < (f == 100).sum()
    walls, n = nd_label(f == 100, structure=eight)
    assert n == nd_label(f == 100, structure=four)[1] - 1 and walls[10, 14] == walls[11, 15] != 0          # the diagonal pair is one item
    assert (np.bincount(walls.reshape(-1))[1:] == 1).sum() == 1                                          # a one-pixel wall
    first = first_cells(walls, n)
    assert first == sorted(first) and first[0] % 64 > first[1] % 64                                      # label 1 starts right of label 2
    un = [it for it in a["items"] if it["category_label"] == "Unable Area"]
    assert np.bincount(nd_label(f == 0, structure=eight)[0].reshape(-1))[1:].tolist() == [1, 6, 4, 5, 12]
    assert [(it["instance_id"], it["item_id"], it["area"]) for it in un] == [("unable_area_2", "unable_area_1", 6), ("unable_area_4", "unable_area_2", 5),
                                                                            ("unable_area_5", "unable_area_3", 12)]
    b, f = by["b_binary"], flipped(by["b_binary"])
    assert set(np.unique(f)) == {0, 255} and b["wall_value"] == 0
    wl = [it for it in b["items"] if it["category_label"] == "wall"]
    ul = [it for it in b["items"] if it["category_label"] == "Unable Area"]
    assert {it["instance_id"][len("unable_area_"):]: it["mask_coords_m"] for it in ul} == \
        {it["instance_id"][len("wall_"):]: it["mask_coords_m"] for it in wl if it["area"] >= 5} and len(wl) > len(ul) > 0
    c, f = by["c_rooms"], flipped(by["c_rooms"])
    assert c["wall_value"] == 60 and (f == 250).sum() > (f == 60).sum() > (f == 249).sum() > 0
    assert all(it["mask_coords_m"] and len(it["mask_coords_m"]) == it["area"] for s in out["scenes"] for it in s["items"])
    path = os.path.join(HERE, "regions_golden.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    assert os.path.getsize(path) < 200 * 1024
    print(path, os.path.getsize(path), "bytes")
    for s in out["scenes"]:
        print(s["name"], s["width"], "x", s["height"], "wall value", s["wall_value"], len(s["items"]), "items")


if __name__ == "__main__":
    main()
