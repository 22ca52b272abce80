"""Top-down seen map timing (sgs_topdown_map), in one run:
  - 640x480 x 1, 1024x768 x 64 and 1920x1080 x 8 mesh depth frames of the synthetic room (make_room_mesh) from cameras pitched down at
    eye height, into the default 256 x 256 grid of 0.05 m cells moved over the room; and the two contention extremes at each size (at
    most 8 frames of those): every pixel in one cell, and every pixel in a cell of its own (a grid of W x H cells);
  - per case the ms per call by HIP events after a warm-up, in alternating rounds, with the spread between rounds;
  - beside it the same grid computed the way a caller must without the kernel: the keys computed in torch, in the same fp32 steps, and
    torch.bincount over them, on the same device and frames — its result is checked equal to the kernel's first;
  - the call's algorithmic bytes (4 B read per pixel, plus the grid cleared and the counters) over its time, against the HBM peak.
Writes profiles/topdown_bench.json and prints it as one JSON line.  Usage: python scripts/topdown_bench.py"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))

SHAPES = ((640, 480, 1), (1024, 768, 64), (1920, 1080, 8))
ROUNDS = 5
HBM_PEAK_GBS = 8000.0          # MI355X: 8 TB/s


def spread(xs):
    return {"median_ms": round(sorted(xs)[len(xs) // 2], 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def torch_map(depth, P, g):
    """(grid int64 [ny,nx,2], counts int64 [B,4]) with torch's own elementwise kernels (one rounding each, in the header's order) and bincount."""
    import torch
    B, H, W = depth.shape
    dev = depth.device
    x = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    y = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    a = P.reshape(B, 12, 1, 1)
    d = [(x * a[:, 3 * k] + y * a[:, 3 * k + 1]) + a[:, 3 * k + 2] for k in range(3)]
    p = [depth * d[k] + a[:, 9 + k] for k in range(3)]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)       # noqa: E731
    inv = f32(1.0) / f32(g.cell_size)
    u, v, h = (p[0] - f32(g.origin_x)) * inv, (p[1] - f32(g.origin_y)) * inv, p[2]
    in_z = (depth >= f32(g.min_z)) & (depth <= f32(g.max_z))
    inside = (u >= 0) & (u < float(g.nx)) & (v >= 0) & (v < float(g.ny))
    free = (h >= f32(g.free_lo)) & (h <= f32(g.free_hi))
    occ = ~free & (h > f32(g.occ_lo)) & (h <= f32(g.occ_hi))
    binned = in_z & inside & (free | occ)
    key = 2 * (v[binned].long() * g.nx + u[binned].long()) + occ[binned].long()
    grid = torch.bincount(key, minlength=2 * g.nx * g.ny).reshape(g.ny, g.nx, 2)
    counts = torch.stack([(~in_z).sum((1, 2)), (in_z & ~inside).sum((1, 2)), (in_z & inside & ~(free | occ)).sum((1, 2)), binned.sum((1, 2))], 1)
    return grid, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topdown_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from sage_gs import Camera, Renderer, TopdownGrid, scenes
    r = Renderer("cuda:0")
    room = scenes.make_room_mesh(2000)
    mesh = r.upload_mesh(room.vertices, room.triangles)
    res = {"metric": "topdown_map_ms", "rounds": ROUNDS, "hbm_peak_GBs": HBM_PEAK_GBS, "device": torch.cuda.get_device_name(0), "cases": {}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    jobs = []
    room_grid = TopdownGrid(origin_x=-3.0, origin_y=-3.5)
    for W, H, B in SHAPES:
        fx, fy, cx, cy = scenes.reference_intrinsics(W, H)
        cams = [Camera(W, H, fx, fy, cx, cy, scenes.view_from_yaw((2.0 + 2.0 * (k % 4) / 4, 1.5 + 2.0 * ((k // 4) % 4) / 4, 1.2), 2 * math.pi * k / min(B, 16), -0.6))
                for k in range(B)]
        depth = r.render_mesh_depth_batch(cams, mesh)
        jobs.append((f"{W}x{H}x{B}_room", depth, r.pix_to_map(cams), room_grid))
        Be = min(B, 8)
        ones = torch.ones((Be, H, W), dtype=torch.float32, device=r.device)
        one_cell = torch.tensor([0, 0, 0, 0, 0, 0, 0, 0, 0, 0.625, 0.375, 0.0], dtype=torch.float32, device=r.device).repeat(Be, 1)
        jobs.append((f"{W}x{H}x{Be}_one_cell", ones, one_cell, TopdownGrid(nx=4, ny=3, origin_x=0.0, origin_y=0.0, cell_size=0.25)))
        own = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=r.device).repeat(Be, 1)
        jobs.append((f"{W}x{H}x{Be}_own_cell", ones, own, TopdownGrid(nx=W, ny=H, origin_x=0.0, origin_y=0.0, cell_size=1.0)))

    timed = []
    for name, depth, P, g in jobs:
        grid, counts = r.topdown_map(depth, P, g)                   # equal first (and the warm-up of both)
        want, want_counts = torch_map(depth, P, g)
        assert torch.equal(grid.long() & 0xFFFFFFFF, want) and torch.equal(counts.long() & 0xFFFFFFFF, want_counts), name
        assert int(want_counts.sum()) == depth.numel()
        timed.append((name, depth, P, g, (grid, counts), [], [], int(want_counts[:, 3].sum()), int((want > 0).sum())))
    torch.cuda.synchronize()
    for _ in range(ROUNDS):                                        # alternating rounds: every case once per round
        for name, depth, P, g, out, ms_k, ms_t, _, _ in timed:
            reps = 20
            e0.record()
            for _ in range(reps):
                r.topdown_map(depth, P, g, out=out)
            e1.record(); torch.cuda.synchronize()
            ms_k.append(e0.elapsed_time(e1) / reps)
            reps = 3
            e0.record()
            for _ in range(reps):
                torch_map(depth, P, g)
            e1.record(); torch.cuda.synchronize()
            ms_t.append(e0.elapsed_time(e1) / reps)
    for name, depth, P, g, out, ms_k, ms_t, binned, cells in timed:
        k, t = spread(ms_k), spread(ms_t)
        nbytes = depth.numel() * 4 + 8 * g.nx * g.ny + depth.shape[0] * (48 + 16)
        res["cases"][name] = {"kernel": k, "torch": t, "torch_over_kernel": round(t["median_ms"] / k["median_ms"], 2),
                              "binned_pixels": binned, "cells_hit": cells,
                              "algorithmic_bytes": nbytes, "GBs": round(nbytes / k["median_ms"] / 1e6, 1),
                              "share_of_hbm_peak": round(nbytes / k["median_ms"] / 1e6 / HBM_PEAK_GBS, 4)}
    print(json.dumps(res))
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
