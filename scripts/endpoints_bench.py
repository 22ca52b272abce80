"""Item-endpoints timing (sgs_endpoints), in one run: a 512x512 map of rooms joined by doors (tests/geodesic_ref.py rooms_with_doors)
with 64, 256 and 1 024 rectangular items of seeded place and size (2 .. 24 cells a side), and 10 000 seeded queries each — an item
towards another item's centroid, as the trajectory generator asks, every tenth without a target.  Per item count the ms of the whole
Renderer.endpoints call (items to answers, its scratch and the read-back of the bytes needed included) by HIP events over five
alternating rounds, the share of every kernel from torch's profiler over the same calls (null where the profiler reports no kernel of
ours: then the phases are unmeasured), and beside them a host search written here — a level-by-level breadth-first search from the
item's boundary on NumPy arrays, one search per query as the reference runs one — over the same queries, in the same run.  Every
device answer is checked equal to the host search's before anything is timed.  Nothing here has a threshold.  Writes
profiles/endpoints_bench.json and prints it as one JSON line.  Usage: python scripts/endpoints_bench.py"""
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
N, N_QUERIES, MAX_DIST = 512, 10000, 50
ITEM_COUNTS = (64, 256, 1024)
PHASES = ("items", "scan", "clear", "mark", "boundary", "rows", "cols", "query")


def spread(xs):
    return {"median_ms": round(sorted(xs)[len(xs) // 2], 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def host_search(np, free, rect, n, sx, sy, target):
    """(x, y, d, n_at_d) of one query by a breadth-first search, level by level, inside the item's box grown by MAX_DIST."""
    x0, y0, x1, y1 = rect
    wx0, wy0, wx1, wy1 = max(x0 - MAX_DIST, 0), max(y0 - MAX_DIST, 0), min(x1 + MAX_DIST, N), min(y1 + MAX_DIST, N)
    h, w = wy1 - wy0, wx1 - wx0
    member = np.zeros((h + 2, w + 2), bool)
    member[y0 - wy0 + 1:y1 - wy0 + 1, x0 - wx0 + 1:x1 - wx0 + 1] = True
    inner = member[:-2, 1:-1] & member[2:, 1:-1] & member[1:-1, :-2] & member[1:-1, 2:]
    frontier = member[1:-1, 1:-1] & ~inner
    ok = free[wy0:wy1, wx0:wx1]
    if target is not None:
        ys, xs = np.mgrid[wy0:wy1, wx0:wx1]
        ok = ok & ((n * xs - sx) * (n * target[0] - sx) + (n * ys - sy) * (n * target[1] - sy) >= 0)
    seen = frontier.copy()
    for d in range(MAX_DIST + 1):
        hit = frontier & ok
        if hit.any():
            at = np.flatnonzero(hit)
            return wx0 + int(at[0]) % w, wy0 + int(at[0]) // w, d, len(at)
        grown = frontier.copy()
        grown[1:] |= frontier[:-1]; grown[:-1] |= frontier[1:]; grown[:, 1:] |= frontier[:, :-1]; grown[:, :-1] |= frontier[:, 1:]
        frontier = grown & ~seen
        seen |= frontier
        if not frontier.any():
            break
    return -1, -1, -1, 0


def kernel_ms(r, args, rounds):
    """{phase: ms per call} from torch's profiler over `rounds` calls, or None when it saw no k_ep_* kernel."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(rounds):
                r.endpoints(*args, max_dist=MAX_DIST)
            torch.cuda.synchronize()
        us = {}
        for e in prof.events():
            m = re.search(r"k_ep_(\w+)", e.name)
            if m:
                us[m.group(1)] = us.get(m.group(1), 0.0) + float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
    except Exception as exc:                                       # the profiler is an extra: the whole-call figure does not depend on it
        print(f"profiler: {exc}", file=sys.stderr)
        return None
    return {p: round(us.get(p, 0.0) / rounds / 1e3, 4) for p in PHASES} if us else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "endpoints_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import geodesic_ref
    from sage_gs import Renderer, _capi
    r = Renderer("cuda:0")
    blocked = geodesic_ref.rooms_with_doors(N)
    free = ~blocked
    src = torch.from_numpy(blocked).to(r.device)
    res = {"metric": "endpoints_ms", "rounds_timed": ROUNDS, "device": torch.cuda.get_device_name(0), "map": [N, N], "queries": N_QUERIES,
           "max_dist": MAX_DIST, "item_counts": {}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    timed = []
    for n_items in ITEM_COUNTS:
        rs = np.random.RandomState(n_items)
        rects = []
        for _ in range(n_items):
            w, h = int(rs.randint(2, 25)), int(rs.randint(2, 25))
            x0, y0 = int(rs.randint(0, N - w + 1)), int(rs.randint(0, N - h + 1))
            rects.append((x0, y0, x0 + w, y0 + h))
        lists = [(np.mgrid[y0:y1, x0:x1][0] * N + np.mgrid[y0:y1, x0:x1][1]).reshape(-1) for x0, y0, x1, y1 in rects]
        offsets = np.concatenate([[0], np.cumsum([len(c) for c in lists])])
        items = (torch.from_numpy(offsets.astype(np.int32)).to(r.device), torch.from_numpy(np.concatenate(lists).astype(np.int32)).to(r.device))
        rows, _, _ = r.endpoints(src, items, [], max_dist=0)
        rows = rows.cpu().numpy().reshape(-1).view(_capi.ENDPOINTS_ITEM_DTYPE)
        who, other = rs.randint(0, n_items, N_QUERIES), rs.randint(0, n_items, N_QUERIES)
        flags = (np.arange(N_QUERIES) % 10 != 0).astype(np.int64)
        q = np.stack([who, rows["cx"][other].astype(np.int64), rows["cy"][other].astype(np.int64), flags], 1)
        qd = torch.from_numpy(q.astype(np.int32)).to(r.device)
        _, answers, counts = r.endpoints(src, items, qd, max_dist=MAX_DIST)          # equal first (and the warm-up)
        got = answers.cpu().numpy()
        t0 = time.perf_counter()
        want = [host_search(np, free, rects[k], int(rows["n"][k]), int(rows["sum_x"][k]), int(rows["sum_y"][k]), (int(tx), int(ty)) if f else None)
                for k, tx, ty, f in q.tolist()]
        host_ms = (time.perf_counter() - t0) * 1e3
        assert got.tolist() == [list(w) for w in want], f"{n_items} items: the device and the host search disagree"
        c = [int(v) for v in counts.cpu().tolist()]
        timed.append((n_items, (src, items, qd), c, host_ms, int((got[:, 3] == 1).sum()), []))
    torch.cuda.synchronize()
    for _ in range(ROUNDS):                                        # alternating rounds: every item count once per round
        for n_items, args, c, host_ms, forced, ms in timed:
            torch.cuda.synchronize()
            e0.record()
            r.endpoints(*args, max_dist=MAX_DIST)
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
    for n_items, args, c, host_ms, forced, ms in timed:
        call = spread(ms)
        res["item_counts"][str(n_items)] = {"answered": c[0], "none": c[1], "forced": forced, "work_bytes": c[3], "call": call,
                                            "us_per_query": round(1e3 * call["median_ms"] / N_QUERIES, 4), "kernels_ms_per_call": kernel_ms(r, args, ROUNDS),
                                            "host_search_ms": round(host_ms, 1), "host_over_device": round(host_ms / call["median_ms"], 1)}
    print(json.dumps(res))
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
