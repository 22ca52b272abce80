"""Collision-mesh depth timing (sgs_render_mesh_depth*): ms per frame for single frames and batches of 8, at 640x480 and 1920x1080, on
make_room_mesh meshes of ~1e5 and ~1e6 triangles, from room_cameras poses.  HIP events around >= 100 frames after a warm-up; prints one
JSON line.  Usage: python scripts/mesh_depth_bench.py [--frames 100] [--warmup 10]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--warmup", type=int, default=16)
    a = ap.parse_args()
    import torch
    from sage_gs import Renderer, scenes
    r = Renderer("cuda:0")
    res = {"metric": "mesh_depth_ms_per_frame", "frames": a.frames, "rows": []}
    for n_tri in (100_000, 1_000_000):
        rm = scenes.make_room_mesh(n_tri, seed=1)
        mesh = r.upload_mesh(rm.vertices, rm.triangles)
        for (w, h) in ((640, 480), (1920, 1080)):
            cams = scenes.room_cameras(rm, w, h, n_positions=4, n_yaw=16, seed=0)
            out1 = torch.empty((h, w), device=r.device)
            out8 = torch.empty((8, h, w), device=r.device)
            for k in range(a.warmup):
                r.render_mesh_depth(cams[k % len(cams)], mesh, out=out1)
                r.render_mesh_depth_batch(cams[:8], mesh, out=out8)
            r.render_mesh_depth(cams[0], mesh, out=out1)
            st = r.last_stats
            row = {"triangles": int(len(rm.triangles)), "width": w, "height": h, "n_visible": int(st["n_visible"]),
                   "records": int(st["d_total"]), "max_tile_len": int(st["max_tile_len"])}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for k in range(a.frames):
                r.render_mesh_depth(cams[k % len(cams)], mesh, out=out1)
            e1.record(); torch.cuda.synchronize()
            row["ms_single"] = round(e0.elapsed_time(e1) / a.frames, 4)
            nb = (a.frames + 7) // 8
            e0.record()
            for k in range(nb):
                b = (8 * k) % (len(cams) - 7)
                r.render_mesh_depth_batch(cams[b:b + 8], mesh, out=out8)
            e1.record(); torch.cuda.synchronize()
            row["ms_per_frame_batch8"] = round(e0.elapsed_time(e1) / (8 * nb), 4)
            res["rows"].append(row)
        mesh.free()
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
