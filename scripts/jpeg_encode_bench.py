"""JPEG encoder timing (sgs_encode_jpeg): at 1024x768 on a 128-pose trajectory of make_room and of make_trained_like,
  - frames/s of sweep.run(write=True) with encoder="pil" (8 PIL threads) and with encoder="gpu", same process, same run, and their ratio;
  - GPU time of the encode alone per frame and per batch of 64 (HIP events after a warm-up);
  - bytes per file for both encoders.
Writes profiles/jpeg_encode_bench.json and prints it as one JSON line.  Usage: python scripts/jpeg_encode_bench.py [--gaussians 500000]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--repeats", type=int, default=3, help="timed sweeps per encoder (the best is reported, all are listed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode_bench.json"))
    a = ap.parse_args()
    import torch
    from sage_gs import Renderer, _capi, scenes, sweep
    from sage_gs import camera as cam_conv
    w, h, n_poses, quality = 1024, 768, 128, 95
    r = Renderer("cuda:0")
    res = {"metric": "jpeg_sweep_frames_per_s", "width": w, "height": h, "poses": n_poses, "quality": quality, "subsampling": "4:2:0",
           "gaussians": a.gaussians, "encode_workers": 8, "chunk": 64, "scenes": {}}
    for name, make in (("make_room", scenes.make_room), ("make_trained_like", scenes.make_trained_like)):
        sc = make(a.gaussians, seed=1)
        scene = r.upload(scenes.to_gaussians(sc, "cuda:0"))
        cams = scenes.room_cameras(sc, w, h, n_positions=2, n_yaw=n_poses // 2, seed=2)
        poses = [cam_conv.isaac_pose_from_view(c.view) for c in cams]
        traj = [{"trajectory_id": "bench", "instruction_index": 0,
                 "points": [{"point": i, "position": [float(v) for v in p], "rotation": [float(v) for v in q]} for i, (p, q) in enumerate(poses)]}]
        row = {}
        with tempfile.TemporaryDirectory() as td:
            for enc in ("pil", "gpu"):
                out = os.path.join(td, enc)
                sweep.run(r, scene, traj, "bench", out, resolution=(w, h), force=True, quality=quality, encoder=enc)      # warm-up
                fps = []
                for _ in range(a.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n = sweep.run(r, scene, traj, "bench", out, resolution=(w, h), force=True, quality=quality, encoder=enc)
                    fps.append(n / (time.perf_counter() - t0))
                d = os.path.join(out, "images", "trajectory_bench")
                sizes = [os.path.getsize(os.path.join(d, f)) for f in sorted(os.listdir(d))]
                assert len(sizes) == n_poses
                row[enc] = {"frames_per_s": round(max(fps), 1), "frames_per_s_runs": [round(v, 1) for v in fps],
                            "bytes_per_file_mean": round(sum(sizes) / len(sizes)), "bytes_per_file_max": max(sizes)}
        row["gpu_over_pil"] = round(row["gpu"]["frames_per_s"] / row["pil"]["frames_per_s"], 2)
        # the encode alone: HIP events around back-to-back calls on frames that stay on the device
        frames = r.render_batch(cams[:64], scene)
        params = _capi.jpeg_params(quality, "4:2:0")
        out_buf = torch.empty((64 * w * h,), dtype=torch.uint8, device=r.device)
        meta = torch.zeros((2, 64), dtype=torch.int64, pin_memory=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for n, reps, key in ((1, 200, "encode_ms_single_frame"), (64, 10, "encode_ms_batch_of_64")):
            for _ in range(3):
                r._encode_jpeg_into(frames, n, params, out_buf, meta)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                r._encode_jpeg_into(frames, n, params, out_buf, meta)
            e1.record(); torch.cuda.synchronize()
            row[key] = round(e0.elapsed_time(e1) / reps, 4)
            assert int(meta[0, n - 1]) + int(meta[1, n - 1]) <= out_buf.numel()
        row["encode_ms_per_frame_in_batch"] = round(row["encode_ms_batch_of_64"] / 64, 4)
        res["scenes"][name] = row
        scene.free()
    r.close()
    res["value"] = min(s["gpu_over_pil"] for s in res["scenes"].values())
    res["what"] = "value = the smaller of the two scenes' ratios: frames/s of sweep.run(write=True, encoder='gpu') over encoder='pil', same run"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
