"""The per-seed bodies of the GPU fuzz campaigns (scripts/gpu_fuzz_rooms.py, gpu_fuzz_trained.py, gpu_fuzz_batch.py), written once: the
scripts sweep seed ranges with them, tests/test_gpu_campaigns.py pins fixed slices in the suite.  A seed fixes the whole case (scene, size,
resolution, pose, band); nothing depends on the clock."""
import numpy as np

import oracle_np as onp
import parity_cases as pc


def _oracle_camera(c):
    from sage_gs import scenes
    view = (np.asarray(c.view, np.float64) @ np.asarray(scenes.MODEL_TO_WORLD, np.float64)).astype(np.float32)
    return onp.Camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy, view)


def _scene_seed(drv, seed, make, n_range, w_range, h_range, what):
    from sage_gs import scenes
    rng = np.random.default_rng(50_000 + seed)
    n = int(rng.integers(*n_range))
    w, h = int(rng.integers(*w_range)), int(rng.integers(*h_range))
    sc = make(n, seed=int(rng.integers(1 << 30)))
    cams = scenes.room_cameras(sc, w, h, n_positions=2, n_yaw=8, seed=int(rng.integers(1 << 30)))
    cam = _oracle_camera(cams[int(rng.integers(len(cams)))])
    gy = (h + 15) // 16
    rows = (0, -1) if rng.random() < 0.6 else tuple(sorted(int(v) for v in rng.choice(gy + 1, 2, replace=False)))
    _, st, aux, _ = pc.check_against_oracle(drv, sc.as_tuple(), cam, None, rows, what=f"{what} seed {seed} (n={n} {w}x{h} rows {rows})")
    aux["recheck"].close()
    return st


def room_seed(drv, seed):
    """A random indoor scene (scenes.make_room, SH degree 3, the asset's -90 degree model transform) at a random size, resolution and pose,
    the whole frame or a band, through the full oracle comparison (parity_cases.check_against_oracle)."""
    from sage_gs import scenes
    return _scene_seed(drv, seed, scenes.make_room, (20_000, 600_000), (320, 2000), (240, 1200), "room")


def trained_seed(drv, seed):
    """The same with trained-3DGS statistics (scenes.make_trained_like)."""
    from sage_gs import scenes
    return _scene_seed(drv, seed, scenes.make_trained_like, (10_000, 250_000), (160, 1400), (120, 900), "trained-like")


def batch_seed(r, seed):
    """sgs_render_batch against the same frames rendered alone, bit for bit, on a random indoor scene (make_room, or make_trained_like one time
    in three) with a random camera set — a run of neighbouring headings (the groups projected by ONE launch over the scene's chunks,
    k_preprocess_shared), views that share nothing (every frame its own live list), or a mix — at a random resolution (some small enough
    for fine tiles), the whole frame or a band of tile rows.  r: a sage_gs.Renderer.  Returns the number of frames compared."""
    import torch
    from sage_gs import scenes
    dev = r.device
    rng = np.random.default_rng(90_000 + seed)
    n = int(rng.integers(20_000, 500_000))
    w, h = [(320, 240), (640, 480), (1024, 768), (1920, 1080), (int(rng.integers(200, 1500)), int(rng.integers(150, 900)))][int(rng.integers(5))]
    sc = (scenes.make_trained_like if rng.random() < 0.3 else scenes.make_room)(n, seed=int(rng.integers(1 << 30)))
    cams = scenes.room_cameras(sc, w, h, n_positions=2, n_yaw=32, seed=int(rng.integers(1 << 30)))
    nb = int(rng.integers(2, 14))
    kind = int(rng.integers(3))
    if kind == 0:      # a path: neighbouring headings from one position
        p0 = int(rng.integers(64)); sel = [(p0 // 32) * 32 + (p0 + k) % 32 for k in range(nb)]
    elif kind == 1:    # anything
        sel = [int(v) for v in rng.integers(0, 64, nb)]
    else:              # runs of neighbours between unrelated views
        sel = []
        while len(sel) < nb:
            p0 = int(rng.integers(64)); run = int(rng.integers(1, 5))
            sel += [(p0 // 32) * 32 + (p0 + k) % 32 for k in range(run)]
        sel = sel[:nb]
    cl = [cams[p] for p in sel]
    gy = (h + 15) // 16
    rows = None if rng.random() < 0.6 else tuple(sorted(int(v) for v in rng.choice(gy + 1, 2, replace=False)))
    fine = bool(rng.random() < 0.7)
    what = f"batch seed {seed} (n={n} {w}x{h} kind={kind} rows={rows} fine={fine})"
    gs = r.upload(scenes.to_gaussians(sc, dev))
    try:
        alone = [r.render(c, gs, tile_rows=rows, fine_tiles=fine).clone() for c in cl]
        out = torch.full((nb, h, w, 3), -1.0, dtype=torch.float32, device=dev)
        r.render_batch(cl, gs, out=out, tile_rows=rows, fine_tiles=fine)
        y0, y1 = (0, h) if rows is None else (16 * rows[0], min(h, 16 * rows[1]))
        for i, fr in enumerate(alone):
            if not torch.equal(out[i, y0:y1], fr[y0:y1]):
                raise AssertionError(f"{what}: frame {i} of {nb} (pose {sel[i]}) differs: "
                                     f"{int((out[i, y0:y1] != fr[y0:y1]).any(dim=-1).sum())} pixels")
        if y1 > y0 and float(torch.stack([f[y0:y1].max() for f in alone]).max()) <= 0.0:
            print(f"  ({what}: empty frames)")
    finally:
        gs.free()
    return nb
