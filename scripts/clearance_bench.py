"""Clearance map timing (sgs_clearance_map, sgs_clearance_query), in one run:
  - sgs_clearance_map on 256x256 x 1, 512x512 x 8 and x 64 room-like maps (walls, interior walls with gaps, furniture), on 1024x1024
    with one obstacle in a corner — the column walk's worst case — and on 512x512 with one obstacle in the middle;
  - sgs_clearance_query on 10, 10^4 and 10^6 segments of 10 samples against a 512x512 room-like map;
  - per case the ms per call by HIP events after a warm-up, in alternating rounds, with the spread between rounds;
  - beside each the host path it replaces, checked equal to the kernel's result before anything is timed: the grid copied to the
    host, SciPy's distance_transform_edt per map and a NumPy threshold at the robot radius (wall-clock; `host_edt`), and for the
    queries the restatement's vectorised NumPy lookup on the host (`host_lookup`);
  - the column walk's length per case — rows visited per cell, from the restatement of the walk — which is what bounds the column
    pass, and the call's algorithmic bytes over its time.
Writes profiles/clearance_bench.json and prints it as one JSON line.  Usage: python scripts/clearance_bench.py"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS = 5
HBM_PEAK_GBS = 8000.0          # MI355X: 8 TB/s
RADIUS_M, SCALE = 0.1, 0.05


def spread(xs):
    return {"median_ms": round(sorted(xs)[len(xs) // 2], 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def room_map(np, n, seed):
    rs = np.random.RandomState(seed)
    ob = np.zeros((n, n), bool)
    ob[0], ob[-1], ob[:, 0], ob[:, -1] = True, True, True, True
    for _ in range(4):                                             # interior walls with a gap
        a, lo, gap = rs.randint(n // 8, 7 * n // 8), rs.randint(0, n // 2), rs.randint(n // 4, 3 * n // 4)
        line = np.zeros(n, bool)
        line[lo:lo + n // 2] = True
        line[gap:gap + 16] = False
        if rs.rand() < 0.5:
            ob[a] |= line
        else:
            ob[:, a] |= line
    for _ in range(n // 8):                                        # furniture
        j, i = rs.randint(4, n - 20, 2)
        ob[j:j + rs.randint(3, 16), i:i + rs.randint(3, 16)] = True
    return ob


def walk_rows(np, d2, ob):
    """Rows a cell visits in k_clear_cols, summed over the map: it walks dy = 1, 2, ... while dy^2 < best (best only shrinks: at
    least up to ceil(sqrt(d2)) - 1, at most to the own row's start) and a row exists on either side.  The lower figure is returned:
    2 (ceil(sqrt(d2)) - 1) per cell, cut at the map's edges."""
    ny, nx = d2.shape
    if not ob.any():
        return 0
    reach = np.ceil(np.sqrt(d2.astype(np.float64))).astype(np.int64) - 1
    reach = np.maximum(reach, 0)
    j = np.arange(ny)[:, None]
    return int((np.minimum(reach, j) + np.minimum(reach, ny - 1 - j)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import clearance_ref as ref
    from sage_gs import Renderer
    from sage_gs.clearance import ClearanceFrame, inflation_limit
    try:
        from scipy.ndimage import distance_transform_edt
    except ImportError:
        distance_transform_edt = None
    r = Renderer("cuda:0")
    L = inflation_limit(RADIUS_M, SCALE)
    res = {"metric": "clearance_ms", "rounds": ROUNDS, "hbm_peak_GBs": HBM_PEAK_GBS, "device": torch.cuda.get_device_name(0),
           "robot_radius_m": RADIUS_M, "scale": SCALE, "max_d2": L, "scipy": distance_transform_edt is not None, "map_cases": {}, "query_cases": {}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    corner = np.zeros((1, 1024, 1024), bool)
    corner[0, 0, 0] = True
    middle = np.zeros((1, 512, 512), bool)
    middle[0, 256, 256] = True
    jobs = [("256x256x1_rooms", np.stack([room_map(np, 256, 1)])), ("512x512x8_rooms", np.stack([room_map(np, 512, 10 + k) for k in range(8)])),
            ("512x512x64_rooms", np.stack([room_map(np, 512, 100 + k) for k in range(64)])), ("1024x1024x1_corner_obstacle", corner),
            ("512x512x1_one_obstacle", middle)]

    def host_edt(src):
        maps = src.cpu().numpy()                                   # D2H of the grid
        return [distance_transform_edt(m == 0, sampling=SCALE) <= RADIUS_M for m in maps]

    timed = []
    for name, maps in jobs:
        src = torch.from_numpy(maps.astype(np.uint8)).to(r.device)
        out = r.clearance_map(src, max_d2=L)                       # equal first (and the warm-up)
        d2 = out[0].cpu().numpy().view(np.uint32)
        for k in range(min(len(maps), 8)):
            assert np.array_equal(d2[k], ref.d2_two_pass(maps[k])), name
        if distance_transform_edt is not None:
            for k, grown in enumerate(host_edt(src)):
                assert np.array_equal(grown, d2[k] <= L), name
        walk = sum(walk_rows(np, d2[k], maps[k]) for k in range(len(maps)))
        timed.append((name, src, out, [], [], walk))
    torch.cuda.synchronize()
    for _ in range(ROUNDS):                                        # alternating rounds: every case once per round
        for name, src, out, ms_k, ms_h, _ in timed:
            reps = 10
            e0.record()
            for _ in range(reps):
                r.clearance_map(src, max_d2=L, out=out)
            e1.record(); torch.cuda.synchronize()
            ms_k.append(e0.elapsed_time(e1) / reps)
            if distance_transform_edt is not None:
                t0 = time.perf_counter()
                host_edt(src)
                ms_h.append((time.perf_counter() - t0) * 1e3)
    for name, src, out, ms_k, ms_h, walk in timed:
        k = spread(ms_k)
        cells = src.numel()
        nbytes = cells * (1 + 4 + 4 + 4) + 16 * src.shape[0]        # the mask read, g written and read (at least once), d2 written
        c = {"kernel": k, "cells": cells, "rows_walked_at_least": walk, "rows_walked_per_cell": round(walk / cells, 2),
             "walk_rows_per_ns": round(walk / k["median_ms"] / 1e6, 2), "algorithmic_bytes": nbytes,
             "GBs": round(nbytes / k["median_ms"] / 1e6, 1), "share_of_hbm_peak": round(nbytes / k["median_ms"] / 1e6 / HBM_PEAK_GBS, 4)}
        if ms_h:
            c["host_edt"] = spread(ms_h)
            c["host_over_kernel"] = round(c["host_edt"]["median_ms"] / k["median_ms"], 1)
        res["map_cases"][name] = c

    # queries against one 512 x 512 room-like map: world coordinates negated and flipped as the reference's defaults do
    ob = room_map(np, 512, 7)
    d2_dev, _ = r.clearance_map(torch.from_numpy(ob.astype(np.uint8)).to(r.device), max_d2=L)
    d2_host = d2_dev.cpu().numpy().view(np.uint32)
    extent = 511 * SCALE
    frame = ClearanceFrame(0.0, 0.0, extent, extent, SCALE, max_d2=L)
    f = ref.Frame(0.0, 0.0, extent, extent, SCALE, max_d2=L, n_samples=10)
    rs = np.random.RandomState(3)
    timed = []
    for n in (10, 10 ** 4, 10 ** 6):
        start = rs.uniform(-extent - 0.3, 0.3, (n, 2))
        segs = np.concatenate([start, start + rs.uniform(-0.5, 0.5, (n, 2))], 1)      # steps of up to half a metre
        dev = torch.from_numpy(segs).to(r.device)
        got = r.clearance_query(d2_dev, frame, dev).cpu().numpy()
        assert np.array_equal(got, ref.query_vectorised(d2_host, f, segs)), n
        timed.append((n, segs, dev, [], [], int((got[:, 0] != 0).sum())))
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for n, segs, dev, ms_k, ms_h, _ in timed:
            reps = 10
            e0.record()
            for _ in range(reps):
                r.clearance_query(d2_dev, frame, dev)
            e1.record(); torch.cuda.synchronize()
            ms_k.append(e0.elapsed_time(e1) / reps)
            t0 = time.perf_counter()
            ref.query_vectorised(d2_host, f, segs)
            ms_h.append((time.perf_counter() - t0) * 1e3)
    for n, segs, dev, ms_k, ms_h, hits in timed:
        k, h = spread(ms_k), spread(ms_h)
        res["query_cases"][f"{n}_segments_x10"] = {"kernel": k, "host_lookup": h, "host_over_kernel": round(h["median_ms"] / k["median_ms"], 1),
                                                   "colliding": hits, "segments_per_us": round(n / k["median_ms"] / 1e3, 2)}
    print(json.dumps(res))
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
