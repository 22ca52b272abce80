"""Resize timing (sgs_resize), in one run:
  - 640x480, 1024x768 and 1920x1080, each -> 320x240; both formats (rgb8, f32) and both filters (bicubic, linear); one frame and a
    batch of 8; GPU time by HIP events after a warm-up, in alternating rounds, with the spread between rounds;
  - PIL.Image.resize on this machine's host for the same arrays (uint8 RGB and mode F);
  - GsCamera.get_rgba() at 640x480 with output_size=(320, 240) against get_rgba() at 640x480 followed by PIL's resize;
  - get_rgba() at 640x480 without output_size (the path that runs no new code), in rounds of its own: --baseline-json names the result
    of the same script run on another build, whose figure is then set beside this one.
Writes profiles/resize_bench.json and prints it as one JSON line.  Usage: python scripts/resize_bench.py [--gaussians 200000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))

SHAPES = ((640, 480), (1024, 768), (1920, 1080))
OUT = (320, 240)
ROUNDS = 5


def spread(xs):
    return {"median_ms": round(sorted(xs)[len(xs) // 2], 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=200_000)
    ap.add_argument("--only-get-rgba", action="store_true", help="time get_rgba() at 640x480 alone (works on a build without sgs_resize)")
    ap.add_argument("--baseline-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from sage_gs import Renderer, _capi, scenes
    from sage_gs.adapter import GsCamera
    from sage_gs import camera as cam_conv
    r = Renderer("cuda:0")
    res = {"metric": "resize_ms", "out_size": list(OUT), "rounds": ROUNDS, "gaussians": a.gaussians, "cases": {}}
    rs = np.random.RandomState(0)

    sc = scenes.make_room(a.gaussians, seed=6)
    scene = r.upload(scenes.to_gaussians(sc, "cuda:0"))
    view = scenes.room_cameras(sc, 640, 480, n_positions=1, n_yaw=4, seed=2)[1].view
    pose = cam_conv.isaac_pose_from_view(view)

    def time_host(fn, reps):
        fn()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t) / reps * 1e3

    plain = GsCamera(r, scene, resolution=(640, 480))
    plain.set_world_pose(*pose)
    rounds = [time_host(lambda: plain.get_rgba(copy=False), 200) for _ in range(ROUNDS)]
    res["get_rgba_640x480_no_output_size"] = spread(rounds)
    if a.baseline_json and os.path.exists(a.baseline_json):
        res["get_rgba_640x480_no_output_size_other_build"] = json.load(open(a.baseline_json))["get_rgba_640x480_no_output_size"]
    if a.only_get_rgba:
        print(json.dumps(res))
        json.dump(res, open(a.out, "w"), indent=1)
        return

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    jobs = []
    for (W, H) in SHAPES:
        rgb = torch.from_numpy(rs.rand(8, H, W, 3).astype(np.float32)).to(r.device)
        dep = torch.from_numpy((rs.rand(8, H, W) * 7).astype(np.float32)).to(r.device)
        for kind, src in (("rgb", rgb), ("depth", dep)):
            for filt in ("bicubic", "linear"):
                for n in (1, 8):
                    out = torch.empty((n, OUT[1], OUT[0], 3) if kind == "rgb" else (n, OUT[1], OUT[0]), dtype=torch.float32, device=r.device)
                    jobs.append((f"{W}x{H}_{kind}_{filt}_n{n}", src[:n], kind, filt, out, []))
    for _, src, kind, filt, out, _ in jobs:                # warm-up: tables, scratch
        for _ in range(3):
            r.resize(src, OUT, filter=filt, kind=kind, clip=(0.1, 6.5) if kind == "depth" else None, out=out)
    torch.cuda.synchronize()
    for _ in range(ROUNDS):                                # alternating rounds: every case once per round
        for _, src, kind, filt, out, ms in jobs:
            reps = 50
            e0.record()
            for _ in range(reps):
                r.resize(src, OUT, filter=filt, kind=kind, clip=(0.1, 6.5) if kind == "depth" else None, out=out)
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
    for name, src, kind, filt, out, ms in jobs:
        res["cases"][name] = spread(ms)

    # the host's route for the same arrays
    for (W, H) in SHAPES:
        u8 = Image.fromarray(rs.randint(0, 256, (H, W, 3)).astype(np.uint8))
        f = Image.fromarray((rs.rand(H, W) * 7).astype(np.float32))
        res["cases"][f"{W}x{H}_pil_rgb_bicubic"] = spread([time_host(lambda: u8.resize(OUT), 10) for _ in range(ROUNDS)])
        res["cases"][f"{W}x{H}_pil_depth_bicubic"] = spread([time_host(lambda: f.resize(OUT), 10) for _ in range(ROUNDS)])

    small = GsCamera(r, scene, resolution=(640, 480), output_size=OUT)
    small.set_world_pose(*pose)
    a_ms, b_ms = [], []
    for _ in range(ROUNDS):
        a_ms.append(time_host(lambda: small.get_rgba(copy=False), 100))
        b_ms.append(time_host(lambda: np.asarray(Image.fromarray(np.ascontiguousarray(plain.get_rgba(copy=False)[..., :3])).resize(OUT)), 20))
    res["get_rgba_640x480_output_size_320x240"] = spread(a_ms)
    res["get_rgba_640x480_then_pil_resize"] = spread(b_ms)
    print(json.dumps(res))
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
