"""PNG encoder timing (sgs_encode_png), in one run:
  - 640x480 depth (16-bit grey) of make_room_mesh from 64 room_cameras poses, and 1024x768 colour of make_room and make_trained_like;
  - GPU time of the encode alone per frame and per batch of 64 (HIP events after a warm-up);
  - the reference's own route per frame: D2H of the fp32 array, the conversion NumPy does (clip * 10000 -> uint16, or the 8-bit
    levels), PIL save(format="PNG") at its default level and at compress_level=1;
  - bytes per file for each.
Writes profiles/png_encode_bench.json and prints it as one JSON line.  Usage: python scripts/png_encode_bench.py [--gaussians 500000]"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--host-frames", type=int, default=8, help="frames the PIL route is timed on (mean per frame)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from sage_gs import Renderer, _capi, scenes
    r = Renderer("cuda:0")
    res = {"metric": "png_encode_ms_per_frame", "batch": 64, "gaussians": a.gaussians, "cases": {}}

    def measure(frames, fmt, to_samples):
        """frames: device fp32 [64,H,W(,3)]."""
        n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        params = _capi.png_params(fmt)
        cap = n * int(r._lib.sgs_png_bound(w, h, C.byref(params)))
        out = torch.empty((cap,), dtype=torch.uint8, device=r.device)
        meta = torch.zeros((2, n), dtype=torch.int64, pin_memory=True)
        floats = int(frames[0].numel())

        def enc(k):
            r._lib.check(r._lib.sgs_encode_png(r._ctx, frames.data_ptr(), w, h, k, floats, C.byref(params), out.data_ptr(), cap, meta[0].data_ptr(),
                                               meta[1].data_ptr(), r._stream()), r._ctx)
        row = {"width": w, "height": h, "format": fmt}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for k, reps, key in ((1, 100, "gpu_encode_ms_single_frame"), (n, 10, "gpu_encode_ms_batch_of_64")):
            for _ in range(3):
                enc(k)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                enc(k)
            e1.record(); torch.cuda.synchronize()
            row[key] = round(e0.elapsed_time(e1) / reps, 4)
        row["gpu_encode_ms_per_frame_in_batch"] = round(row["gpu_encode_ms_batch_of_64"] / n, 4)
        sizes = meta[1].tolist()
        row["gpu_bytes_per_file_mean"] = round(sum(sizes) / n)
        # the reference's route: the fp32 array crosses the link, NumPy makes the samples, PIL (zlib) makes the file
        for key, kw in (("pil_default", {}), ("pil_compress_level_1", {"compress_level": 1})):
            t_total, nbytes = 0.0, 0
            for i in range(a.host_frames):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = frames[i].cpu().numpy()
                b = io.BytesIO()
                Image.fromarray(to_samples(host)).save(b, format="PNG", **kw)
                t_total += time.perf_counter() - t0
                nbytes += len(b.getvalue())
            row[key + "_ms_per_frame"] = round(1e3 * t_total / a.host_frames, 3)
            row[key + "_bytes_per_file_mean"] = round(nbytes / a.host_frames)
        return row

    room = scenes.make_room_mesh(50_000, seed=1)
    mesh = r.upload_mesh(room.vertices, room.triangles)
    cams = scenes.room_cameras(room, 640, 480, n_positions=2, n_yaw=32, seed=2)
    depth = r.render_mesh_depth_batch(cams, mesh).contiguous()
    res["cases"]["depth16_640x480_make_room_mesh"] = measure(depth, "depth16", lambda d: (np.clip(d, 0.0, 6.5) * 10000.0).astype(np.uint16))
    mesh.free()
    levels = lambda x: (np.clip(x, 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    for name, make in (("make_room", scenes.make_room), ("make_trained_like", scenes.make_trained_like)):
        sc = make(a.gaussians, seed=1)
        scene = r.upload(scenes.to_gaussians(sc, "cuda:0"))
        cams = scenes.room_cameras(sc, 1024, 768, n_positions=2, n_yaw=32, seed=2)
        frames = r.render_batch(cams, scene).contiguous()
        res["cases"][f"rgb8_1024x768_{name}"] = measure(frames, "rgb8", levels)
        scene.free()
    r.close()
    res["value"] = max(c["gpu_encode_ms_per_frame_in_batch"] for c in res["cases"].values())
    res["what"] = "value = the slowest case's device encode per frame in a batch of 64, ms; the host route per frame is beside it in every case"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
