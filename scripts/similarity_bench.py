"""Image similarity timing (sgs_image_similarity), in one run:
  - 640x480 x 1, 1024x768 x 64 and 1920x1080 x 8 rendered room frames against one shared target (frame 0's levels);
  - per case the ms per call by HIP events after a warm-up, in alternating rounds, with the spread between rounds;
  - beside it the same quantity by a torch formulation on the same device and frames: the levels, then conv2d of the five moment maps
    (x, y, x^2, y^2, x y) with the float 11 x 11 Gaussian, fp32, and the SSIM map's mean — what a caller writes without the kernel;
  - first the scores are checked: the kernel's against an fp64 evaluation of the float-Gaussian SSIM (shifted slices, no conv) within
    the window-quantisation bound of tests/test_similarity_ref.py; the fp32 conv2d's distance from the kernel's score is recorded;
  - the call's algorithmic bytes (12 B of frame + 3 B of target per pixel) over its time, against the HBM peak.
Writes profiles/similarity_bench.json and prints it as one JSON line.  Usage: python scripts/similarity_bench.py"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))

SHAPES = ((640, 480, 1), (1024, 768, 64), (1920, 1080, 8))
ROUNDS = 5
HBM_PEAK_GBS = 8000.0          # MI355X: 8 TB/s
WINDOW_QUANTISATION_BOUND = 6e-4
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def spread(xs):
    return {"median_ms": round(sorted(xs)[len(xs) // 2], 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def gaussian(torch, dtype, device):
    g = torch.exp(-((torch.arange(11, dtype=torch.float64, device=device) - 5.0) ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def levels(torch, frames):
    return torch.floor(frames.clamp(0.0, 1.0) * 255.0 + 0.5)


def torch_ssim(torch, frames, target):
    """Mean SSIM per frame [B] by conv2d with the float window, fp32: frames fp32 [B,H,W,3], target uint8 [H,W,3]."""
    F = torch.nn.functional
    B, H, W, _ = frames.shape
    x = levels(torch, frames).permute(0, 3, 1, 2).reshape(B * 3, 1, H, W)
    y = target.to(torch.float32).permute(2, 0, 1).reshape(1, 3, H, W).expand(B, 3, H, W).reshape(B * 3, 1, H, W)
    g = gaussian(torch, torch.float32, frames.device)
    k = (g[:, None] * g[None, :]).reshape(1, 1, 11, 11)
    mx, my, xx, yy, xy = (F.conv2d(v, k) for v in (x, y, x * x, y * y, x * y))
    s = ((2 * mx * my + C1) * (2 * (xy - mx * my) + C2)) / ((mx * mx + my * my + C1) * ((xx - mx * mx) + (yy - my * my) + C2))
    return s.reshape(B, -1).mean(1)


def slices_ssim64(torch, frames, target):
    """The same in fp64 by shifted slices (elementwise only): the yardstick of the check."""
    B, H, W, _ = frames.shape
    x = levels(torch, frames).double()
    y = target.double()[None].expand(B, H, W, 3)
    g = gaussian(torch, torch.float64, frames.device)

    def blur(v):
        h = sum(g[i] * v[:, :, i:i + W - 10] for i in range(11))
        return sum(g[j] * h[:, j:j + H - 10] for j in range(11))

    mx, my, xx, yy, xy = (blur(v) for v in (x, y, x * x, y * y, x * y))
    s = ((2 * mx * my + C1) * (2 * (xy - mx * my) + C2)) / ((mx * mx + my * my + C1) * ((xx - mx * mx) + (yy - my * my) + C2))
    return s.reshape(B, -1).mean(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from sage_gs import Renderer, scenes
    r = Renderer("cuda:0")
    room = scenes.make_room(50_000)
    scene = r.upload(scenes.to_gaussians(room, "cuda:0"))
    res = {"metric": "image_similarity_ms", "rounds": ROUNDS, "hbm_peak_GBs": HBM_PEAK_GBS, "bound": WINDOW_QUANTISATION_BOUND, "cases": {}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    timed = []
    for W, H, B in SHAPES:
        cams = scenes.room_cameras(room, W, H, n_positions=4, n_yaw=16, seed=0)[:B]
        frames = r.render_batch(cams, scene)
        target = r.pack_rgba8(frames[0])[..., :3].contiguous()
        got = r.image_similarity(frames, target)                   # (the warm-up of both, and the check)
        assert got["ssim"][0] == 1.0 and (got["sse"][0] == 0).all()
        n = min(B, 4)
        want = slices_ssim64(torch, frames[:n], target).cpu().numpy()
        worst = float(np.abs(got["ssim"][:n] - want).max())
        assert worst <= WINDOW_QUANTISATION_BOUND, (W, H, B, worst)
        conv = torch_ssim(torch, frames, target).cpu().numpy().astype(np.float64)
        timed.append((f"{W}x{H}x{B}", frames, target, worst, float(np.abs(got["ssim"] - conv).max()), [], []))
    torch.cuda.synchronize()
    lib, ctx = r._lib, r._ctx
    for _ in range(ROUNDS):                                        # alternating rounds: every case once per round
        for name, frames, target, _, _, ms_k, ms_t in timed:
            B, H, W, _ = frames.shape
            rows = torch.empty((B, 8), dtype=torch.int64, device=r.device)
            st = r._stream()
            reps = 20
            e0.record()
            for _ in range(reps):                                  # the C ABI itself: no copy of the rows to the host between calls
                lib.check(lib.sgs_image_similarity(ctx, frames.data_ptr(), W, H, B, 3 * H * W, target.data_ptr(), 0, rows.data_ptr(), st), ctx)
            e1.record(); torch.cuda.synchronize()
            ms_k.append(e0.elapsed_time(e1) / reps)
            reps = 3
            e0.record()
            for _ in range(reps):
                torch_ssim(torch, frames, target)
            e1.record(); torch.cuda.synchronize()
            ms_t.append(e0.elapsed_time(e1) / reps)
    for name, frames, target, worst, conv_gap, ms_k, ms_t in timed:
        k, t = spread(ms_k), spread(ms_t)
        B, H, W, _ = frames.shape
        nbytes = B * H * W * 15
        res["cases"][name] = {"kernel": k, "torch_conv2d": t, "torch_over_kernel": round(t["median_ms"] / k["median_ms"], 2),
                              "worst_score_gap_to_fp64_float_window": worst, "worst_score_gap_to_fp32_conv2d": conv_gap,
                              "algorithmic_bytes": nbytes, "GBs": round(nbytes / k["median_ms"] / 1e6, 1),
                              "share_of_hbm_peak": round(nbytes / k["median_ms"] / 1e6 / HBM_PEAK_GBS, 4)}
    print(json.dumps(res))
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
