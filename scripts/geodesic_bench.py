"""Geodesic field timing (sgs_geodesic_field, sgs_geodesic_path), in one run:
  - 64 fields — 64 seeded goals on one map — on 512x512 maps of three kinds: an open room, rooms joined by doors, and a serpentine
    maze (tests/geodesic_ref.py makes them); per kind the rounds until no tile is dirty and the wall-clock ms of
    Renderer.geodesic_field, which owns the CONTINUE loop and reads the status back once per call;
  - 10^4 shortest paths down the fields of each kind, one launch, by HIP events;
  - beside them the host search they replace — this project's own restatement of a heap search with the straight-line heuristic
    (geodesic_ref.heap_search), one search per (start, goal) pair — on a few pairs per kind, with the ms per pair; its step counts are
    checked equal to the field's before anything is timed;
  - one field per kind is checked equal to the integer restatement (geodesic_ref.field) first.
Nothing here has a threshold.  Writes profiles/geodesic_bench.json and prints it as one JSON line.  Usage: python scripts/geodesic_bench.py"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS = 3
N, N_FIELDS, N_PATHS, HOST_PAIRS = 512, 64, 10 ** 4, 4


def spread(xs):
    return {"median_ms": round(sorted(xs)[len(xs) // 2], 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geodesic_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import geodesic_ref as ref
    from sage_gs import Renderer
    r = Renderer("cuda:0")
    T = int(r._lib.sgs_geodesic_tile())
    res = {"metric": "geodesic_ms", "rounds_timed": ROUNDS, "device": torch.cuda.get_device_name(0), "map": [N, N], "tile": T, "fields": N_FIELDS,
           "paths": N_PATHS, "rounds_per_call": 2 * 2 * (N // T), "kinds": {}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kinds = {"open_room": ref.open_room(N), "rooms_with_doors": ref.rooms_with_doors(N), "serpentine_maze": ref.serpentine_maze(N)}
    timed = []
    for name, ob in kinds.items():
        src = torch.from_numpy(ob).to(r.device)
        goals = ref.seeded_free_cells(ob, N_FIELDS, seed=1)
        seeds = [(f,) + g for f, g in enumerate(goals)]
        fm = [0] * N_FIELDS
        steps, _ = r.geodesic_field(src, seeds, field_map=fm)      # equal first (and the warm-up)
        rounds = int(r.last_geodesic_rounds)
        got = steps.cpu().numpy().view(np.uint32)
        want0 = ref.field(ob, [goals[0]])
        assert np.array_equal(got[0], want0), name
        starts = ref.seeded_free_cells(ob, N_PATHS, seed=2)
        q = torch.tensor([(k % N_FIELDS,) + s for k, s in enumerate(starts)], dtype=torch.int32, device=r.device)
        longest = int(got.astype(np.int64).sum(-1)[got[..., 0] != ref.NONE].max()) + 1
        cells, info = r.geodesic_path(src, steps, q, field_map=fm, max_len=longest)
        info = info.cpu().numpy()
        assert (info[:, 1] == 0).all(), name
        host = []
        for k in range(HOST_PAIRS):                                # the host search on a few of the same pairs, field 0's
            s = starts[k * N_FIELDS]
            t0 = time.perf_counter()
            p = ref.heap_search(ob, s, goals[0])
            host.append((time.perf_counter() - t0) * 1e3)
            assert ref.count_steps(p) == tuple(int(v) for v in want0[s[1], s[0]]), (name, s)
        timed.append((name, src, seeds, fm, steps, q, longest, rounds, host, int(info[:, 0].sum()), [], []))
    torch.cuda.synchronize()
    for _ in range(ROUNDS):                                        # alternating rounds: every kind once per round
        for name, src, seeds, fm, steps, q, longest, rounds, host, n_cells, ms_f, ms_p in timed:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.geodesic_field(src, seeds, field_map=fm)
            torch.cuda.synchronize()
            ms_f.append((time.perf_counter() - t0) * 1e3)
            e0.record()
            r.geodesic_path(src, steps, q, field_map=fm, max_len=longest)
            e1.record(); torch.cuda.synchronize()
            ms_p.append(e0.elapsed_time(e1))
    for name, src, seeds, fm, steps, q, longest, rounds, host, n_cells, ms_f, ms_p in timed:
        f, p, h = spread(ms_f), spread(ms_p), spread(host)
        res["kinds"][name] = {"rounds": rounds, "field_calls": rounds // res["rounds_per_call"], "fields_64": f, "ms_per_field": round(f["median_ms"] / N_FIELDS, 4),
                              "paths_10k": p, "path_cells": n_cells, "longest_path_cells": longest, "host_heap_search_per_pair": h,
                              "host_pairs_timed": HOST_PAIRS,
                              "host_64_pairs_over_64_fields": round(64 * h["median_ms"] / f["median_ms"], 1)}
    res["slowest_kind"] = max(res["kinds"], key=lambda k: res["kinds"][k]["fields_64"]["median_ms"])
    print(json.dumps(res))
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
