"""Connected-regions timing (sgs_regions_label), in one run: 64 maps of 512x512 in one call, for five kinds of set —
  - the walls of rooms joined by doors (tests/geodesic_ref.py rooms_with_doors, 64 seeds) and their free space;
  - the free space of the serpentine maze: one region that winds through every tile;
  - a checkerboard under 4-connectivity: every cell of the set its own region, 131072 per map;
  - a 50 % random mask (64 seeds);
per kind the ms of the whole call by HIP events (64 rows per map), the share of every kernel — the phases local, merge, flatten, scan,
rank, labels, rows, largest — from torch's profiler over the same calls (null where the profiler reports no kernel of ours: then
the phases are unmeasured), and beside them scipy.ndimage.label over the same 64 maps on the host, in the same run (null without
SciPy).  The first map of every kind is checked equal to the restatement (tests/regions_ref.py) before anything is timed.  Nothing
here has a threshold.  Writes profiles/regions_bench.json and prints it as one JSON line.  Usage: python scripts/regions_bench.py"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS = 5
N, N_MAPS, MAX_REGIONS = 512, 64, 64
PHASES = ("clear", "local", "merge", "flatten", "scan", "rank", "labels", "rows", "largest")


def spread(xs):
    return {"median_ms": round(sorted(xs)[len(xs) // 2], 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def kernel_ms(r, src, conn, rounds):
    """{phase: ms per call} from torch's profiler over `rounds` calls, or None when it saw no k_reg_* kernel."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(rounds):
                r.label_regions(src, connectivity=conn, max_regions=MAX_REGIONS)
            torch.cuda.synchronize()
        us = {}
        for e in prof.events():
            m = re.search(r"k_reg_(\w+)", e.name)
            if m:
                us[m.group(1)] = us.get(m.group(1), 0.0) + float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
    except Exception as exc:                                       # the profiler is an extra: the whole-call figure does not depend on it
        print(f"profiler: {exc}", file=sys.stderr)
        return None
    return {p: round(us.get(p, 0.0) / rounds / 1e3, 4) for p in PHASES} if us else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import geodesic_ref
    import regions_ref as ref
    from sage_gs import Renderer, _capi
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    r = Renderer("cuda:0")
    rooms = np.stack([geodesic_ref.rooms_with_doors(N, seed=k) for k in range(N_MAPS)])
    j, i = np.mgrid[:N, :N]
    kinds = {"walls": (rooms, 8), "free_space": (~rooms, 8), "serpentine_maze": (np.repeat(~geodesic_ref.serpentine_maze(N)[None], N_MAPS, 0), 8),
             "checkerboard_4": (np.repeat(((i + j) % 2 == 0)[None], N_MAPS, 0), 4),
             "random_50": (np.stack([np.random.RandomState(k).rand(N, N) < 0.5 for k in range(N_MAPS)]), 8)}
    res = {"metric": "regions_ms", "rounds_timed": ROUNDS, "device": torch.cuda.get_device_name(0), "map": [N, N], "maps": N_MAPS,
           "tile": int(r._lib.sgs_regions_tile()), "max_regions": MAX_REGIONS, "work_bytes": 4 * int(r._lib.sgs_regions_work_words(N, N, N_MAPS)), "kinds": {}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    timed = []
    for name, (maps, conn) in kinds.items():
        src = torch.from_numpy(maps).to(r.device)
        labels, rows, counts = r.label_regions(src, connectivity=conn, max_regions=MAX_REGIONS)      # equal first (and the warm-up)
        wl, wr, wc = ref.regions(maps[0], conn, max_regions=MAX_REGIONS)
        assert np.array_equal(labels[0].cpu().numpy(), wl) and counts[0].cpu().numpy().view(np.uint32).tolist() == wc.tolist(), name
        assert rows[0].cpu().numpy().reshape(-1).view(_capi.REGION_ROW_DTYPE).tobytes() == wr.tobytes(), name
        n_regions = counts[:, 0].cpu().numpy().view(np.uint32)
        host = None
        if ndimage is not None:
            structure = np.ones((3, 3), int) if conn == 8 else None
            host = []
            for _ in range(2):
                t0 = time.perf_counter()
                ns = [ndimage.label(m, structure=structure)[1] for m in maps]
                host.append((time.perf_counter() - t0) * 1e3)
            assert ns == n_regions.tolist(), name
        timed.append((name, src, conn, maps, n_regions, host, []))
    torch.cuda.synchronize()
    for _ in range(ROUNDS):                                        # alternating rounds: every kind once per round
        for name, src, conn, maps, n_regions, host, ms in timed:
            torch.cuda.synchronize()
            e0.record()
            r.label_regions(src, connectivity=conn, max_regions=MAX_REGIONS)
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
    for name, src, conn, maps, n_regions, host, ms in timed:
        call = spread(ms)
        h = None if host is None else spread(host)
        res["kinds"][name] = {"connectivity": conn, "cells_in_set_per_map": int(maps[0].sum()), "regions_per_map": [int(n_regions.min()), int(n_regions.max())],
                              "call_64_maps": call, "ms_per_map": round(call["median_ms"] / N_MAPS, 4), "kernels_ms_per_call": kernel_ms(r, src, conn, ROUNDS),
                              "host_scipy_64_maps": h, "host_over_device": None if h is None else round(h["median_ms"] / call["median_ms"], 1)}
    res["slowest_kind"] = max(res["kinds"], key=lambda k: res["kinds"][k]["call_64_maps"]["median_ms"])
    print(json.dumps(res))
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
