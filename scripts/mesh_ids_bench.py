"""Collision-mesh object-id timing (sgs_render_mesh_ids*) against the depth path of the same run: ms per frame of render_mesh_ids with
depth, render_mesh_ids without depth and render_mesh_depth, measured ALTERNATELY (round after round, HIP events around each block) on the
shapes of scripts/mesh_depth_bench.py — make_room_mesh meshes of ~1e5 and ~1e6 triangles, 640x480 and 1920x1080, single frames and
batches of 8, room_cameras poses; labels are make_room_mesh_parts' objects.  The yardstick is render_mesh_depth of the same run.
Prints one JSON line and writes it to --out.  Usage: python scripts/mesh_ids_bench.py [--frames 104] [--rounds 4] [--warmup 16] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=104, help="frames per variant and shape, over all rounds")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_ids_bench.json"))
    a = ap.parse_args()
    import torch
    from sage_gs import Renderer, scenes
    r = Renderer("cuda:0")
    per_round = max(8, (a.frames + a.rounds - 1) // a.rounds)
    res = {"metric": "mesh_ids_ms_per_frame", "frames": per_round * a.rounds, "rounds": a.rounds, "rows": []}
    for n_tri in (100_000, 1_000_000):
        V, T, part = scenes.make_room_mesh_parts(n_tri, seed=1)
        rm = scenes.make_room_mesh(n_tri, seed=1)
        mesh = r.upload_mesh(V, T, labels=part)
        for (w, h) in ((640, 480), (1920, 1080)):
            cams = scenes.room_cameras(rm, w, h, n_positions=4, n_yaw=16, seed=0)
            z1, i1 = torch.empty((h, w), device=r.device), torch.empty((h, w), dtype=torch.int32, device=r.device)
            z8, i8 = torch.empty((8, h, w), device=r.device), torch.empty((8, h, w), dtype=torch.int32, device=r.device)
            single = {
                "ids_depth": lambda c: r.render_mesh_ids(c, mesh, out=i1, out_depth=z1),
                "ids": lambda c: r.render_mesh_ids(c, mesh, out=i1),
                "depth": lambda c: r.render_mesh_depth(c, mesh, out=z1),
            }
            batch = {
                "ids_depth": lambda cs: r.render_mesh_ids_batch(cs, mesh, out=i8, out_depth=z8),
                "ids": lambda cs: r.render_mesh_ids_batch(cs, mesh, out=i8),
                "depth": lambda cs: r.render_mesh_depth_batch(cs, mesh, out=z8),
            }
            for k in range(a.warmup):
                for f in single.values():
                    f(cams[k % len(cams)])
                for f in batch.values():
                    f(cams[:8])
            single["depth"](cams[0])
            st = r.last_stats
            row = {"triangles": int(len(T)), "width": w, "height": h, "records": int(st["d_total"]), "max_tile_len": int(st["max_tile_len"])}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = {("single", v): [] for v in single}
            ms.update({("batch8", v): [] for v in batch})
            nb = (per_round + 7) // 8
            for rnd in range(a.rounds):
                for v, f in single.items():
                    torch.cuda.synchronize()
                    e0.record()
                    for k in range(per_round):
                        f(cams[(rnd * per_round + k) % len(cams)])
                    e1.record(); torch.cuda.synchronize()
                    ms[("single", v)].append(e0.elapsed_time(e1) / per_round)
                for v, f in batch.items():
                    torch.cuda.synchronize()
                    e0.record()
                    for k in range(nb):
                        b = (8 * (rnd * nb + k)) % (len(cams) - 7)
                        f(cams[b:b + 8])
                    e1.record(); torch.cuda.synchronize()
                    ms[("batch8", v)].append(e0.elapsed_time(e1) / (8 * nb))
            for mode in ("single", "batch8"):
                d = {v: round(statistics.median(ms[(mode, v)]), 4) for v in single}
                d["rounds"] = {v: [round(x, 4) for x in ms[(mode, v)]] for v in single}
                d["depth_spread"] = round((max(ms[(mode, "depth")]) - min(ms[(mode, "depth")])) / d["depth"], 4)
                d["ids_depth_over_depth"] = round(d["ids_depth"] / d["depth"], 4)
                d["ids_over_depth"] = round(d["ids"] / d["depth"], 4)
                row[mode] = d
            res["rows"].append(row)
        mesh.free()
    r.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
