"""Visible-object table timing (sgs_object_table), in one run:
  - 640x480 x 1, 1024x768 x 64 and 1920x1080 x 8 frames; the frames are rendered room frames (make_room_mesh_parts, 12 labels), and
    the two contention extremes: one label on every pixel, and every pixel its own label (n_labels = H W; at most 8 frames of those);
  - per case the ms per call by HIP events after a warm-up, in alternating rounds, with the spread between rounds;
  - beside it the same table computed the way a caller must without the kernel: torch.bincount plus scatter_reduce_ amin / amax on the
    flattened ids, written out below, on the same device and frames — its result is checked equal to the kernel's first;
  - the call's algorithmic bytes (8 B read per pixel with depth, plus the table written) over its time, against the HBM peak.
Writes profiles/object_table_bench.json and prints it as one JSON line.  Usage: python scripts/object_table_bench.py"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))

SHAPES = ((640, 480, 1), (1024, 768, 64), (1920, 1080, 8))
ROUNDS = 5
HBM_PEAK_GBS = 8000.0          # MI355X: 8 TB/s


def spread(xs):
    return {"median_ms": round(sorted(xs)[len(xs) // 2], 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def torch_table(ids, depth, n_labels):
    """(n [B,L], x_min, y_min, x_end, y_end, z_min, sum_x, sum_y, counts [B,2]) with torch's own reductions."""
    import torch
    B, H, W = ids.shape
    dev = ids.device
    flat = ids.reshape(B, -1).long()
    ok = (flat >= 0) & (flat < n_labels)
    key = (flat + torch.arange(B, device=dev)[:, None] * n_labels)[ok]
    pix = torch.arange(H * W, device=dev).expand(B, -1)[ok]
    ys, xs = pix // W, pix % W
    L = B * n_labels
    n = torch.bincount(key, minlength=L)
    sum_x = torch.zeros(L, dtype=torch.int64, device=dev).scatter_add_(0, key, xs)
    sum_y = torch.zeros(L, dtype=torch.int64, device=dev).scatter_add_(0, key, ys)
    big = 2 ** 31 - 1
    x_min = torch.full((L,), big, dtype=torch.int64, device=dev).scatter_reduce_(0, key, xs, "amin")
    y_min = torch.full((L,), big, dtype=torch.int64, device=dev).scatter_reduce_(0, key, ys, "amin")
    x_end = torch.zeros(L, dtype=torch.int64, device=dev).scatter_reduce_(0, key, xs + 1, "amax")
    y_end = torch.zeros(L, dtype=torch.int64, device=dev).scatter_reduce_(0, key, ys + 1, "amax")
    z_min = torch.full((L,), float("inf"), dtype=torch.float32, device=dev).scatter_reduce_(0, key, depth.reshape(B, -1)[ok], "amin")
    counts = torch.stack([(flat == -1).sum(1), (~ok & (flat != -1)).sum(1)], 1)
    return [t.reshape(B, n_labels) for t in (n, x_min, y_min, x_end, y_end, z_min, sum_x, sum_y)] + [counts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_table_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from sage_gs import Renderer, _capi, scenes
    r = Renderer("cuda:0")
    V, T, part = scenes.make_room_mesh_parts(2000)
    mesh = r.upload_mesh(V, T, labels=part)
    room = scenes.make_room_mesh(2000)
    res = {"metric": "object_table_ms", "rounds": ROUNDS, "hbm_peak_GBs": HBM_PEAK_GBS, "cases": {}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    jobs = []
    for W, H, B in SHAPES:
        cams = scenes.room_cameras(room, W, H, n_positions=4, n_yaw=16, seed=0)[:B]
        ids, depth = r.render_mesh_ids_batch(cams, mesh, return_depth=True)
        jobs.append((f"{W}x{H}x{B}_room", ids, depth, 12))
        Be = min(B, 8)
        flat_depth = depth[:Be].contiguous()
        jobs.append((f"{W}x{H}x{Be}_one_label", torch.zeros((Be, H, W), dtype=torch.int32, device=r.device), flat_depth, 12))
        own = torch.arange(H * W, dtype=torch.int32, device=r.device).reshape(1, H, W).repeat(Be, 1, 1)
        jobs.append((f"{W}x{H}x{Be}_own_label", own, flat_depth, H * W))

    def check(ids, depth, n_labels):
        rows, counts = r.object_table(ids, depth, n_labels=n_labels)
        rec = rows.cpu().numpy().view(_capi.OBJECT_ROW_DTYPE).reshape(ids.shape[0], n_labels)
        ref = [t.cpu().numpy() for t in torch_table(ids, depth, n_labels)]
        for k, name in enumerate(_capi.OBJECT_ROW_DTYPE.names):
            assert np.array_equal(rec[name].astype(ref[k].dtype), ref[k]), name
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), ref[8])

    timed = []
    for name, ids, depth, n_labels in jobs:
        check(ids, depth, n_labels)                                # equal first (and the warm-up of both)
        out = r.object_table(ids, depth, n_labels=n_labels)
        timed.append((name, ids, depth, n_labels, out, [], []))
    torch.cuda.synchronize()
    for _ in range(ROUNDS):                                        # alternating rounds: every case once per round
        for name, ids, depth, n_labels, out, ms_k, ms_t in timed:
            reps = 20
            e0.record()
            for _ in range(reps):
                r.object_table(ids, depth, n_labels=n_labels, out=out)
            e1.record(); torch.cuda.synchronize()
            ms_k.append(e0.elapsed_time(e1) / reps)
            reps = 3
            e0.record()
            for _ in range(reps):
                torch_table(ids, depth, n_labels)
            e1.record(); torch.cuda.synchronize()
            ms_t.append(e0.elapsed_time(e1) / reps)
    for name, ids, depth, n_labels, out, ms_k, ms_t in timed:
        k, t = spread(ms_k), spread(ms_t)
        nbytes = ids.numel() * 8 + ids.shape[0] * (n_labels * 40 + 8)
        res["cases"][name] = {"kernel": k, "torch": t, "torch_over_kernel": round(t["median_ms"] / k["median_ms"], 2),
                              "algorithmic_bytes": nbytes, "GBs": round(nbytes / k["median_ms"] / 1e6, 1),
                              "share_of_hbm_peak": round(nbytes / k["median_ms"] / 1e6 / HBM_PEAK_GBS, 4)}
    print(json.dumps(res))
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
