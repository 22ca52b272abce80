"""Parity tests proper: the HIP path on a real MI355X, called through the C ABI (via the Python
host side), against the oracle — same cases as the emulator run plus full-size scenes and
size-independent properties at BASELINE.json's sizes."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle_c
import oracle_np as onp
import frontend_cases as fc
import parity_cases as pc
from conftest import assert_frame_close, stored_variants
from tight_parity import assert_frame_tight


class GpuDriver:
    """Adapts sage_gs.Renderer (torch tensors, C ABI underneath) to the parity_cases driver shape."""

    def __init__(self):
        import torch
        from sage_gs import Renderer
        assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
        self.torch = torch
        self.r = Renderer("cuda:0")
        self.scene = None

    def upload(self, means, scales, quats, opac, sh, deg):
        from sage_gs import Gaussians
        t = lambda a: self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        if self.scene is not None:
            self.scene.free()
        self.scene = self.r.upload(Gaussians(t(means), t(scales), t(quats), t(opac), t(sh), deg))

    def render(self, cam, cfg=None, rows=(0, -1), out=None, full_sort=False, loose_cull=False, interleave=None,
               chunk_cull=True, stats=True, deep=True, fine=True):
        from sage_gs import Camera
        c = Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, np.asarray(cam.view, np.float64))
        k = self._config(cfg)
        if interleave is not None:         # (stride, phase): compact image of the owned tile rows
            owned = len(range(interleave[1], (cam.height + 15) // 16, interleave[0]))
            band = self.torch.full((16 * owned, cam.width, 3), -1.0, dtype=self.torch.float32, device="cuda:0")
            img = self.r.render(c, self.scene, config=k, out_band=band, tile_rows=None if rows == (0, -1) else rows,
                                full_sort=full_sort, loose_cull=loose_cull, interleave=interleave, chunk_cull=chunk_cull, stats=stats,
                                deep_cull=deep, fine_tiles=fine)
            return img.cpu().numpy(), self.r.last_stats
        o = None if out is None else self.torch.from_numpy(out).to("cuda:0")
        img = self.r.render(c, self.scene, config=k, out=o, tile_rows=None if rows == (0, -1) else rows,
                            full_sort=full_sort, loose_cull=loose_cull, chunk_cull=chunk_cull, stats=stats, deep_cull=deep, fine_tiles=fine)
        return img.cpu().numpy(), self.r.last_stats

    def _config(self, cfg):
        from sage_gs import RenderConfig
        return None if cfg is None else RenderConfig(cfg.near, cfg.far, cfg.dilation, cfg.clamp, cfg.alpha_min,
                                                     cfg.alpha_max, cfg.t_min, cfg.background, cfg.sh_degree)

    def render_batch(self, cams, fine=True, cfg=None):
        from sage_gs import Camera
        cl = [Camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy, np.asarray(c.view, np.float64)) for c in cams]
        return self.r.render_batch(cl, self.scene, config=self._config(cfg), fine_tiles=fine).cpu().numpy()

    def render_batch_stats(self, cams):
        from sage_gs import Camera
        cl = [Camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy, np.asarray(c.view, np.float64)) for c in cams]
        batch, stats = self.r.render_batch(cl, self.scene, want_stats=True)
        return batch.cpu().numpy(), stats

    def frames_in_flight(self, cams):
        """One asynchronous pipelined render per camera, each into its own buffer, then ONE sync()."""
        from sage_gs import Camera
        outs = [self.torch.full((c.height, c.width, 3), -1.0, dtype=self.torch.float32, device="cuda:0") for c in cams]
        for c, o in zip(cams, outs):
            self.r.render(Camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy, np.asarray(c.view, np.float64)), self.scene, out=o, sync=False, pipelined=True)
        self.r.sync()
        return [o.cpu().numpy() for o in outs]

    def render_aux(self, cam, cfg=None, rows=(0, -1), fine=True, deep=True, stats=False, out=None, out_aux=None):
        """Renderer.render(return_aux / out_aux): (rgb [H, W, 3], aux [H, W, 2] = expected depth and coverage, stats).  `out` / `out_aux`:
        pre-filled host arrays, copied to the device, rendered into and copied back (a band leaves the other rows alone)."""
        from sage_gs import Camera
        c = Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, np.asarray(cam.view, np.float64))
        o = None if out is None else self.torch.from_numpy(np.ascontiguousarray(out, np.float32)).to("cuda:0")
        oa = None if out_aux is None else self.torch.from_numpy(np.ascontiguousarray(out_aux, np.float32)).to("cuda:0")
        img, aux = self.r.render(c, self.scene, config=self._config(cfg), out=o, out_aux=oa, return_aux=True,
                                 tile_rows=None if rows == (0, -1) else rows, deep_cull=deep, stats=stats, fine_tiles=fine)
        return img.cpu().numpy(), aux.cpu().numpy(), self.r.last_stats

    def intermediates(self):
        return self.r.intermediates()

    def set_record_capacity(self, n):
        self.r.set_record_capacity(n)

    def set_tuning(self, **kw):
        self.r.set_tuning(**kw)

    def tuning(self):
        return self.r.tuning()

    def chunk_skipped(self):
        from sage_gs import _capi
        return self.r.debug_buffer(_capi.BUF_CHUNK_SKIPPED, np.uint8)

    def row_records(self, n_rows, reset=True):
        return self.r.row_records(n_rows, reset)

    def close(self):
        if self.scene is not None:
            self.scene.free()
        self.r.close()


@pytest.fixture(scope="module")
def drv():
    d = GpuDriver()
    yield d
    d.close()


def test_library_is_the_hip_build(drv):
    """The GPU tests must run the in-tree HIP library, not anything else."""
    import os
    assert os.path.basename(drv.r._lib.path) == "libsage_gs.so"
    assert "sage-3d_official_amd/lib" in drv.r._lib.path.replace("\\", "/")
    from sage_gs import _capi
    assert drv.r._lib.version() == _capi.ABI_VERSION


def test_config1(drv):
    pc.case_config1(drv, n=10_000)


def test_sh_degrees(drv):
    pc.case_sh_degrees(drv, n=3000)


def test_ragged_sizes(drv):
    pc.case_ragged(drv)


def test_seeded_random_frames(drv):
    pc.case_fuzz(drv, range(60))


def test_seeded_random_frames_with_needles_and_specks(drv):
    """Splats from far below a pixel to needles and pancakes the size of the scene (aspect ratios up to 1e4): what the
    completed-square form of q2 is for (seeds 8019 and 8036 failed the three-term form by 1.6e-3)."""
    pc.case_fuzz(drv, range(7000, 7040), 700, wild=True)
    pc.case_fuzz(drv, [8019, 8036] + list(range(8000, 8010)), 3000, (900, 600), wild=True)


def test_needle_extents_follow_the_rounded_conic(drv):
    """A needle thousands of pixels long blends pixels (alpha 1.01 alpha_min, 2 500 px from its centre) that the ellipse of
    its fp64 covariance ends 5 px short of: the fp32 rounding of the conic's three nearly dependent entries moves the length
    of the long axis.  The bin rect and the staging extents are derived from the conic the composite blends with; before
    (rounds 1-2 and most of round 3) the production frame of this seed differed from the reference-binning frame in three
    pixels by 1.4e-4 — inside the pixel tolerance, outside the bit-identity the culling stages promise."""
    pc.case_fuzz(drv, [3002], 3000, (2400, 1400), wild=True)
    pc.case_fuzz(drv, range(3003, 3010), 3000, (2400, 1400), wild=True)


def test_seeded_random_frames_over_a_background_with_depth_and_coverage(drv):
    pc.case_fuzz_variants(drv, range(9100, 9112))


def test_non_finite_gaussians_are_invisible_and_harmless(drv):
    pc.case_non_finite_gaussians(drv)
    pc.case_non_finite_gaussians(drv, n=700, res=(96, 64), seed=4)


def test_padding_lanes_stay_culled(drv):
    pc.case_padding_lanes(drv)


def test_empty_and_all_culled(drv):
    pc.case_empty(drv)


def test_tile_row_bands(drv):
    pc.case_tile_rows(drv, n=6000, res=(400, 300))


def test_chunk_bounds_skip_only_invisible_chunks(drv):
    pc.case_chunk_bounds(drv, n=60_000, res=(640, 400))


@pytest.mark.parametrize("stride", [2, 3, 8])
def test_interleaved_tile_rows(drv, stride):
    pc.case_interleaved_rows(drv, stride)


def test_depth_ties(drv):
    pc.case_depth_ties(drv)


def test_big_depth_bucket(drv):
    pc.case_big_depth_bucket(drv, n_slab=6000)


def test_sort_classes(drv):
    pc.case_sort_classes(drv, sizes=(700, 2500, 6000, 9500, 20000))


def test_sparse_lists(drv):
    pc.case_sparse_lists(drv)


def test_deep_tile(drv):
    pc.case_deep_tile(drv, n_back=12000)


def test_full_grid_splat(drv):
    pc.case_full_grid_splat(drv, res=(1920, 1080), variants=True)
    pc.case_full_grid_splat(drv, res=(3840, 2160))


def test_depth_and_coverage_outputs(drv):
    pc.case_depth_aux(drv, n=20_000, res=(320, 240))


def test_batch_shares_scene_reads(drv):
    pc.case_batch_shares_scene_reads(drv, n=60_000, res=(640, 368))


def test_determinism(drv):
    pc.case_determinism(drv, n=50_000)


def test_overflow_retry():
    d = GpuDriver()
    try:
        pc.case_overflow_retry(d)
    finally:
        d.close()


def test_more_frames_in_flight_than_the_status_ring_has_slots():
    d = GpuDriver()
    try:
        pc.case_status_ring(d)
    finally:
        d.close()


# ---- room scenes at 1080p against the C oracle -----------------------------------------------------
def _room(n, seed):
    from sage_gs import scenes
    sc = scenes.make_room(n, seed=seed)
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=2, n_yaw=8, seed=seed)
    return sc, cams


@pytest.mark.parametrize("n,seed,cam_ids", [(120_000, 1, (0, 3, 5)), (400_000, 2, (9,))])
def test_room_1080p_vs_oracle(drv, n, seed, cam_ids):
    sc, cams = _room(n, seed)
    for ci in cam_ids:
        cam = cams[ci]
        view = (np.asarray(cam.view) @ sc.model_to_world).astype(np.float32)
        ocam = onp.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, view)
        pc.check_against_oracle(drv, sc.as_tuple(), ocam, what=f"room n={n} cam {ci}")


# ---- BASELINE.json full sizes: size-independent properties ------------------------------------------
@pytest.fixture(scope="module")
def big_scene():
    from sage_gs import scenes
    sc = scenes.make_room(3_000_000, seed=2)
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=2, n_yaw=4, seed=2)
    return sc, cams


def _check_frame_properties(drv, ocam, n_gauss, bands, stride=8, background=False):
    """Size-independent properties of one full-size frame of the scene uploaded in `drv` (beside the whole-frame oracle
    comparisons further down): queues strictly ordered by (depth bits, index), D == sum of rect areas, tile-row bands and
    interleaved rows reproduce the frame bit for bit (the multi-GPU sharding property), the lazy sort consumes what the
    full sort consumed, culling hooks never change a pixel, determinism, background linearity."""
    W, H = ocam.width, ocam.height
    gy = (H + 15) // 16
    prod, st_prod = drv.render(ocam, full_sort=True)                    # production binning (tight rects)
    full, st = drv.render(ocam, full_sort=True, loose_cull=True)          # reference binning: the structures checked below
    assert (prod == full).all() and st_prod["d_total"] <= st["d_total"] and st_prod["d_fetched"] <= st["d_fetched"]
    assert np.isfinite(full).all() and full.min() >= 0.0
    assert 0 < st["n_visible"] <= n_gauss and st["d_total"] >= st["n_visible"] and st["d_fetched"] <= st["d_total"]
    off, ids, slot_ids, splats = drv.intermediates()
    # (1) every queue is sorted by (depth bits, index); the offsets are a partition of D
    assert off[-1] == st["d_total"] and (np.diff(off) >= 0).all() and len(off) == ((W + 15) // 16) * gy + 1
    key_of = np.zeros(n_gauss, np.uint64); key_of[slot_ids] = splats[:, 9].astype(np.uint64)
    comp = (key_of[ids] << np.uint64(32)) | ids.astype(np.uint64)
    tile_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    same = tile_of[1:] == tile_of[:-1]
    assert (comp[1:][same] > comp[:-1][same]).all(), "a queue is not strictly ordered by (depth, index)"
    del comp, tile_of, same, key_of
    # (2) D == sum of rect areas of the visible splats (a checksum of the binning)
    x0, y0 = splats[:, 10] & 0xffff, splats[:, 10] >> 16
    x1, y1 = splats[:, 11] & 0xffff, splats[:, 11] >> 16
    assert int(((x1 - x0).astype(np.int64) * (y1 - y0)).sum()) == st["d_total"]
    # (2b) the per-chunk bounds skipped no visible Gaussian
    no_cull, st_nc = drv.render(ocam, chunk_cull=False)
    assert (no_cull == full).all() and st_nc["n_visible"] == st["n_visible"] and st_nc["d_total"] == st_prod["d_total"]
    # (3) tile-row bands reproduce the full frame bit-exactly (the multi-GPU sharding property)
    union = np.zeros_like(full); d_sum = 0
    for r0, r1 in bands:
        band, st_b = drv.render(ocam, None, (r0, r1))
        union[r0 * 16:min(r1 * 16, H)] = band[r0 * 16:min(r1 * 16, H)]
        d_sum += st_b["d_total"]
    assert (union == full).all() and d_sum == st_prod["d_total"] and bands[0][0] == 0 and bands[-1][1] == gy
    # (3b) so do interleaved rows (rank p of `stride` owns rows p, p+stride, ...), and their queues add up to the frame's
    union = np.zeros_like(full); d_sum = 0
    for phase in range(stride):
        comp_img, st_p = drv.render(ocam, interleave=(stride, phase))
        for k, row in enumerate(range(phase, gy, stride)):
            ya, yb = 16 * row, min(16 * row + 16, H)
            union[ya:yb] = comp_img[16 * k: 16 * k + (yb - ya)]
        d_sum += st_p["d_total"]
    assert (union == full).all() and d_sum == st_prod["d_total"]
    # (4) idempotence / determinism
    # ... of the PRODUCTION instantiation (what a sweep runs: no D_f bookkeeping, the deep-tile cull): the same frame, twice; and — the
    # sharding property again — the union of ITS tile-row bands is the frame itself
    again, st_again = drv.render(ocam, stats=False)
    assert (again == full).all() and st_again["d_total"] == st_prod["d_total"] and st_again["d_fetched"] == 0
    again2, _ = drv.render(ocam, stats=False)
    assert (again2 == again).all(), "two production renders of one frame differ"
    union = np.zeros_like(full)
    for r0, r1 in bands:
        band, _ = drv.render(ocam, None, (r0, r1), stats=False)
        union[r0 * 16:min(r1 * 16, H)] = band[r0 * 16:min(r1 * 16, H)]
    assert (union == again).all(), "the union of production bands differs from the production frame"
    # (5) lazy sort under reference binning consumes exactly as many records as the full sort did
    loose, st_loose = drv.render(ocam, loose_cull=True)
    assert (loose == full).all() and st_loose["d_fetched"] == st["d_fetched"]
    # (6) background linearity: frame(bg) = frame(black) + (1 - coverage) * bg, coverage from the depth/coverage output
    if background:
        from sage_gs import Camera, RenderConfig
        c = Camera(W, H, ocam.fx, ocam.fy, ocam.cx, ocam.cy, np.asarray(ocam.view, np.float64))
        bg = (0.25, 0.5, 0.75)
        over = drv.r.render(c, drv.scene, config=RenderConfig(background=bg)).cpu().numpy()
        _, aux = drv.r.render(c, drv.scene, return_aux=True)
        t_final = 1.0 - aux.cpu().numpy()[..., 1:2]
        assert np.abs(over - (full + t_final * np.asarray(bg, np.float32))).max() < 2e-6
        assert (t_final >= 0).all() and (t_final <= 1).all()
    return full, st_prod


def _ocam(cam, sc):
    view = (np.asarray(cam.view) @ sc.model_to_world).astype(np.float32)
    return onp.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, view)


BANDS_1080_8 = ((0, 9), (9, 18), (18, 27), (27, 36), (36, 44), (44, 52), (52, 60), (60, 68))
BANDS_4K_8 = tuple((17 * i, min(135, 17 * (i + 1))) for i in range(8))                             # 17 x 7 + 16


def test_3m_scene_properties(drv, big_scene):
    """BASELINE configs[2] at its real size."""
    sc, cams = big_scene
    drv.upload(*sc.as_tuple())
    frames = {}
    for cam in (cams[0], cams[5]):
        frames[id(cam)] = _check_frame_properties(drv, _ocam(cam, sc), 3_000_000, BANDS_1080_8, background=cam is cams[0])
    # (7) the ORDER of the input arrays does not matter: the same Gaussians uploaded in a random order (another Z-order sort on the device,
    # other original indices everywhere) give the same N_v and D and the same frame — bit for bit in every tile whose queue holds no two
    # records of EQUAL depth bits (ties break on the original index, which the permutation changes; these poses look straight at walls
    # whose surfels share their depth, so such tiles exist — and only there may a pixel move)
    means, scales, quats, opac, sh = sc.as_tuple()[:5]
    perm = np.random.default_rng(11).permutation(means.shape[0])
    drv.upload(means[perm], scales[perm], quats[perm], opac[perm], sh[perm], *sc.as_tuple()[5:])
    for cam in (cams[0], cams[5]):
        full, st = frames[id(cam)]
        again, st2 = drv.render(_ocam(cam, sc), full_sort=True)
        assert st2["n_visible"] == st["n_visible"] and st2["d_total"] == st["d_total"]
        off, ids, slot_ids, splats = drv.intermediates()
        key_of = np.zeros(3_000_000, np.uint32); key_of[slot_ids] = splats[:, 9]
        keys = key_of[ids]
        tile_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
        tie = (tile_of[1:] == tile_of[:-1]) & (keys[1:] == keys[:-1])
        tie_tile = np.zeros(len(off) - 1, bool); tie_tile[tile_of[1:][tie]] = True
        gx = (1920 + 15) // 16
        differs = (again != full).any(axis=2)
        ys, xs = np.nonzero(differs)
        assert tie_tile[(ys // 16) * gx + xs // 16].all(), "a pixel moved in a tile without depth ties after permuting the input"
        assert differs.mean() < 0.02 and np.abs(again - full).max() < 0.25 and (~tie_tile).sum() > 1000


def test_3m_scene_rigid_motion_invariance(drv, big_scene):
    """BASELINE configs[2] at its real size, SH degree 0 evaluated (the higher bands live in the model frame): the scene and the camera moved by
    the SAME rigid motion give the same frame.  Not bit for bit — every mean, covariance and view vector is computed from different
    floats — but N_v and D to a few parts in 10^5 and all but a sliver of the pixels to 1e-3 (the rest: decisions within rounding of a
    threshold, bounded by the largest single contribution)."""
    from scipy.spatial.transform import Rotation
    sc, cams = big_scene
    means, scales, quats, opac, sh = sc.as_tuple()[:5]
    cfg = onp.Config(sh_degree=0)
    drv.upload(*sc.as_tuple())
    ref = {}
    for cam in (cams[1], cams[6]):
        ref[id(cam)] = drv.render(_ocam(cam, sc), cfg)
    rot = Rotation.from_euler("zyx", [37.0, -21.0, 63.0], degrees=True)
    Q = rot.as_matrix(); t = np.array([0.7, -1.3, 2.1])
    qx, qy, qz, qw = rot.as_quat()
    a = np.array([qw, qx, qy, qz]); b = quats.astype(np.float64)
    moved_q = np.stack([a[0] * b[:, 0] - a[1] * b[:, 1] - a[2] * b[:, 2] - a[3] * b[:, 3],
                        a[0] * b[:, 1] + a[1] * b[:, 0] + a[2] * b[:, 3] - a[3] * b[:, 2],
                        a[0] * b[:, 2] - a[1] * b[:, 3] + a[2] * b[:, 0] + a[3] * b[:, 1],
                        a[0] * b[:, 3] + a[1] * b[:, 2] - a[2] * b[:, 1] + a[3] * b[:, 0]], 1).astype(np.float32)
    moved_m = (means.astype(np.float64) @ Q.T + t).astype(np.float32)
    drv.upload(moved_m, scales, moved_q, opac, sh, *sc.as_tuple()[5:])
    inv = np.eye(4); inv[:3, :3] = Q.T; inv[:3, 3] = -Q.T @ t                     # model' -> model
    for cam in (cams[1], cams[6]):
        img0, st0 = ref[id(cam)]
        oc = _ocam(cam, sc)
        oc2 = onp.Camera(oc.width, oc.height, oc.fx, oc.fy, oc.cx, oc.cy, (np.asarray(oc.view, np.float64) @ inv).astype(np.float32))
        img1, st1 = drv.render(oc2, cfg)
        # (measured: N_v identical, D 13 and 8 of 6.5 M apart, 1.5e-4 / 1.8e-4 of the pixels beyond 1e-3, largest move 0.008 — a few times that is allowed)
        assert abs(st1["n_visible"] - st0["n_visible"]) <= 1e-5 * st0["n_visible"] and abs(st1["d_total"] - st0["d_total"]) <= 2e-5 * st0["d_total"]
        d = np.abs(img1 - img0).max(axis=2)
        print(f"[parity] rigid motion at 3 M: N_v {st0['n_visible']} -> {st1['n_visible']}, D {st0['d_total']} -> {st1['d_total']}, pixels moved by > 1e-3: "
              f"{(d > 1e-3).mean():.2e}, > 1e-5: {(d > 1e-5).mean():.2e}, max {d.max():.4f}")
        assert (d > 1e-3).mean() < 1e-3 and d.max() < 0.05 and img0.max() > 0.2, f"{(d > 1e-3).mean():.2e} of the pixels moved by more than 1e-3 (max {d.max():.3f})"


def test_room_500k_1080p_config2(drv):
    """BASELINE configs[1]: make_room(500 000, seed 1) at 1920x1080, SH degree 3.  Two poses: the full comparison with the
    oracle (counts, offsets, queue order, splat attributes, pixels) on two bands of tile rows each — the oracle finishes a
    band in seconds — and the size-independent properties on the full frame."""
    from sage_gs import scenes
    sc = scenes.make_room(500_000, seed=1)
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=2, n_yaw=8, seed=1)
    for ci, bands in ((2, ((30, 34), (50, 53))), (13, ((0, 3), (36, 40)))):
        ocam = _ocam(cams[ci], sc)
        for rows in bands:
            pc.check_against_oracle(drv, sc.as_tuple(), ocam, rows=rows, what=f"config2 500k cam {ci} rows {rows}")
        _check_frame_properties(drv, ocam, 500_000, BANDS_1080_8, background=(ci == 2))


def test_3m_scene_4k_config5_geometry(drv, big_scene):
    """BASELINE configs[4] geometry at its real size: the 3 M-Gaussian scene at 3840x2160 (240 x 135 tiles = four binning
    windows), a pose of the 1-degree yaw sweep.  Size-independent properties on the full frame, bands = the 8-rank
    partition (17 x 7 + 16); oracle check of a band that straddles a binning-window boundary (tile row 34)."""
    from sage_gs import scenes
    sc, _ = big_scene
    cam = scenes.sweep_cameras(sc, 3840, 2160, n=360)[77]
    ocam = _ocam(cam, sc)
    drv.upload(*sc.as_tuple())
    _check_frame_properties(drv, ocam, 3_000_000, BANDS_4K_8)
    r0, r1 = 33, 36
    img, st_b = drv.render(ocam, None, (r0, r1))
    img_ref, st_bref = drv.render(ocam, None, (r0, r1), loose_cull=True)
    ref, aux = oracle_c.render(*sc.as_tuple(), ocam, None, r0, r1, want="image")
    assert (img_ref == img).all() and st_bref["d_total"] == aux["D"] and st_b["n_visible"] == aux["n_visible"]
    sl = slice(r0 * 16, r1 * 16)
    assert_frame_close(img[sl], ref[sl], aux["margin"][sl], aux["recheck"], what="3M @ 4K band", y0=sl.start)
    assert_frame_tight(img[sl], ref[sl], aux, y0=sl.start, what="3M @ 4K band")


# ---- BASELINE.json full sizes: FULL frames against the oracle ----------------------------------------------------------
# The C oracle renders a 3 M-Gaussian 1080p frame in a second or two on the GPU box's host cores, so the headline configuration
# gets the complete comparison — N_v, D, tile offsets, every queue's order, rects and depth bits bit for bit, conics / colours to
# fp32 rounding, every pixel within 1e-3 (threshold-sensitive ones two-sidedly) — on whole frames at poses of bench.py's own sweep
# (step i renders pose 77 i mod 256 of room_cameras(n_positions=4, n_yaw=64, seed=2)).
BENCH_POSE_STRIDE = 77


def _bench_pose_ids(steps):
    return [(i * BENCH_POSE_STRIDE) % 256 for i in steps]


def test_3m_scene_full_frames_vs_oracle_at_the_bench_poses(drv, big_scene):
    """BASELINE configs[2]: make_room(3 000 000, seed 2), SH degree 3, 1920x1080 — TEN whole frames of the bench's sweep (steps 0-8: poses
    0, 77, 154, 231, 52, 129 — the slowest of the 256 —, 206, 27, 104; and step 15, pose 131), each through check_against_oracle."""
    from sage_gs import scenes
    sc, _ = big_scene
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=4, n_yaw=64, seed=2)
    ids = _bench_pose_ids(list(range(9)) + [15])
    assert 129 in ids and len(set(ids)) == 10
    drv.upload(*sc.as_tuple())
    d_f = []
    for pid in ids:
        _, st, aux, _ = pc.check_against_oracle(drv, sc.as_tuple(), _ocam(cams[pid], sc), what=f"3M @1080p bench pose {pid} (full frame)", upload=False)
        d_f.append(st["d_fetched"])
        aux["recheck"].close()
    assert min(d_f) > 100_000


def test_3m_scene_more_bench_poses_images_and_counts_vs_oracle(drv, big_scene):
    """Twenty-two more poses of the bench's sweep (steps 16-37), whole frames: N_v, D (reference binning) and every pixel against the oracle —
    with the ten of the test above, every eighth pose of the 256 the headline is measured on has been held against the oracle."""
    from sage_gs import scenes
    sc, _ = big_scene
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=4, n_yaw=64, seed=2)
    drv.upload(*sc.as_tuple())
    for pid in _bench_pose_ids(range(16, 38)):
        ocam = _ocam(cams[pid], sc)
        img, st = drv.render(ocam, stats=False)                          # the instantiation the sweep runs
        img_ref, st_ref = drv.render(ocam, loose_cull=True)
        ref, aux = oracle_c.render(*sc.as_tuple(), ocam, want="image")
        assert (img_ref == img).all() and st["n_visible"] == aux["n_visible"] and st_ref["d_total"] == aux["D"] and st["d_total"] <= aux["D"]
        assert_frame_close(img, ref, aux["margin"], aux["recheck"], what=f"3M @1080p bench pose {pid} (image + counts)")
        assert_frame_tight(img, ref, aux, what=f"3M @1080p bench pose {pid} (image + counts)")
        aux["recheck"].close()


def test_3m_scene_at_the_reference_resolutions_vs_oracle(drv, big_scene):
    """The 3 M-Gaussian scene at the resolutions the reference itself renders (run_benchmark.py:1409-1419 --low-res 320x240, simple_env.py:52
    640x480, generate_images.py:43 1024x768), whole frames through check_against_oracle at the sweep's slowest pose (129) and another: a
    320x240 tile sees thirty-six times the scene area of a 1080p tile — queues of 10-40 k records, windows of whole buckets, the bucket-ordered
    copy, refinements, the deep-tile cull — the composite's longest code paths, on real queues, against the oracle's queues and pixels."""
    from sage_gs import scenes
    sc, _ = big_scene
    drv.upload(*sc.as_tuple())
    deep = 0
    for (w, h), poses in (((320, 240), (129, 206)), ((640, 480), (129,)), ((1024, 768), (27,))):
        cams = scenes.room_cameras(sc, w, h, n_positions=4, n_yaw=64, seed=2)
        for pid in poses:
            _, st, aux, _ = pc.check_against_oracle(drv, sc.as_tuple(), _ocam(cams[pid], sc), what=f"3M @{w}x{h} pose {pid} (full frame)", upload=False)
            deep += st["n_deep_windows_plain"]
            assert st["max_tile_len"] > (4096 if w <= 640 else 1024)
            aux["recheck"].close()
    assert deep > 0, "no window was culled against live pixels: the deep-tile path was not exercised"


def test_trained_like_3m_full_frame_vs_oracle(drv):
    """A scene with trained-3DGS statistics (scenes.make_trained_like: heavy-tailed anisotropic scales, 40 % nearly transparent splats, floaters,
    no spatial order; D = 28 M records at 1080p, six times the room scene's) — one whole 1080p frame through check_against_oracle."""
    from sage_gs import scenes
    sc = scenes.make_trained_like(3_000_000, seed=2)
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=4, n_yaw=64, seed=2)
    drv.set_record_capacity(96 << 20)
    _, st, aux, _ = pc.check_against_oracle(drv, sc.as_tuple(), _ocam(cams[77], sc), what="trained-like 3M @1080p pose 77 (full frame)")
    assert st["d_total"] > 10_000_000
    aux["recheck"].close()


def test_room_500k_full_frames_vs_oracle(drv):
    """BASELINE configs[1]: make_room(500 000, seed 1) at 1920x1080, SH degree 3 — two whole frames."""
    from sage_gs import scenes
    sc = scenes.make_room(500_000, seed=1)
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=2, n_yaw=8, seed=1)
    drv.upload(*sc.as_tuple())
    for ci in (2, 13):
        _, _, aux, _ = pc.check_against_oracle(drv, sc.as_tuple(), _ocam(cams[ci], sc), what=f"config2 500k cam {ci} (full frame)", upload=False)
        aux["recheck"].close()


def test_3m_scene_4k_full_frame_vs_oracle(drv, big_scene):
    """BASELINE configs[4]: the 3 M-Gaussian scene at 3840x2160, pose 77 of the 360-camera yaw sweep — the whole frame (240 x 135 tiles,
    four binning windows) through check_against_oracle."""
    from sage_gs import scenes
    sc, _ = big_scene
    cam = scenes.sweep_cameras(sc, 3840, 2160, n=360, seed=2)[77]          # (bench.py --config 5, step 1)
    _, _, aux, _ = pc.check_against_oracle(drv, sc.as_tuple(), _ocam(cam, sc), what="3M @ 3840x2160 sweep pose 77 (full frame)")
    aux["recheck"].close()


def test_4k_frame_multi_window_binning(drv):
    """configs[4] geometry: 3840x2160 is 240 x 135 tiles = four binning windows of the LDS tile histogram.
    Oracle-checked on a band that straddles a window boundary; size-independent properties on the full frame."""
    from sage_gs import scenes
    sc = scenes.make_room(300_000, seed=7)
    cams = scenes.room_cameras(sc, 3840, 2160, n_positions=1, n_yaw=4, seed=7)
    cam = cams[1]
    view = (np.asarray(cam.view) @ sc.model_to_world).astype(np.float32)
    ocam = onp.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, view)
    drv.upload(*sc.as_tuple())
    full, st = drv.render(ocam)
    ref_bin, st_ref = drv.render(ocam, full_sort=True, loose_cull=True)
    assert (ref_bin == full).all() and 0 < st["d_total"] <= st_ref["d_total"]
    off, ids, slot_ids, splats = drv.intermediates()
    assert off[-1] == st_ref["d_total"] and len(off) == 240 * 135 + 1
    x0, y0 = splats[:, 10] & 0xffff, splats[:, 10] >> 16
    x1, y1 = splats[:, 11] & 0xffff, splats[:, 11] >> 16
    assert int(((x1 - x0).astype(np.int64) * (y1 - y0)).sum()) == st_ref["d_total"]      # checksum of the binning
    # bands (one of them cutting through window boundaries at tile rows 34 / 68 / 102) reproduce the frame
    union = np.zeros_like(full)
    for r0, r1 in ((0, 30), (30, 70), (70, 103), (103, 135)):
        band, _ = drv.render(ocam, None, (r0, r1))
        union[r0 * 16:min(r1 * 16, 2160)] = band[r0 * 16:min(r1 * 16, 2160)]
    assert (union == full).all()
    r0, r1 = 32, 36                                                # straddles the first window boundary
    img, st_b = drv.render(ocam, None, (r0, r1))
    _, st_bref = drv.render(ocam, None, (r0, r1), loose_cull=True)
    ref, aux = oracle_c.render(*sc.as_tuple(), ocam, None, r0, r1, want="image")
    assert st_bref["d_total"] == aux["D"] and st_b["n_visible"] == aux["n_visible"]
    sl = slice(r0 * 16, r1 * 16)
    assert_frame_close(img[sl], ref[sl], aux["margin"][sl], aux["recheck"], what="4K band", y0=sl.start)
    assert_frame_tight(img[sl], ref[sl], aux, y0=sl.start, what="4K band")


def test_culling_never_changes_a_pixel_stress(drv):
    """The tight bin rects and the exact quadrant test may only remove work no pixel can see: production frames must be
    bit-identical to reference-binning frames over a sweep of poses and over splats built to sit on every edge of
    those tests (needle-thin diagonal ellipses, opacities straddling alpha_min, splats larger than the image,
    centres on tile and quadrant borders)."""
    import torch
    from sage_gs import Camera, Gaussians, scenes
    # (a) a sweep through the indoor scene
    sc = scenes.make_room(1_000_000, seed=11)
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=3, n_yaw=8, seed=11)
    scene = drv.r.upload(scenes.to_gaussians(sc, "cuda:0"))
    for cam in cams:
        prod = drv.r.render(cam, scene).clone()
        ref = drv.r.render(cam, scene, loose_cull=True)
        assert (prod == ref).all()
        assert (drv.r.render(cam, scene, deep_cull=False) == ref).all()
    scene.free()
    # (b) adversarial splats in front of a fixed camera
    rng = np.random.default_rng(5)
    n = 60_000
    means = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(0.5, 9, n)], 1).astype(np.float32)
    kind = rng.integers(0, 5, n)
    s = np.exp(rng.uniform(np.log(0.002), np.log(0.05), (n, 3)))
    s[kind == 0, 0] *= 60.0                                            # needles
    s[kind == 1] *= np.array([40.0, 0.2, 1.0])                         # thin sheets
    s[kind == 2] *= 30.0                                               # very large
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    opac = rng.uniform(0.0, 1.0, n)
    opac[kind == 3] = rng.uniform(0.9 / 255.0, 1.3 / 255.0, (kind == 3).sum())     # straddling alpha_min
    opac[kind == 4] = rng.uniform(0.985, 1.0, (kind == 4).sum())                    # straddling alpha_max
    # some centres exactly on tile / quadrant borders of the 640x480 image (fx = 400: x = (px - 320) z / 400)
    sel = rng.choice(n, 4000, replace=False)
    pxs = rng.choice([0, 7.5, 8, 15.5, 16, 31.5, 320, 639], 4000); pys = rng.choice([0, 7.5, 8, 15.5, 16, 239.5, 479], 4000)
    means[sel, 0] = ((pxs + 0.5 - 320.0) * means[sel, 2] / 400.0).astype(np.float32)
    means[sel, 1] = ((pys + 0.5 - 240.0) * means[sel, 2] / 400.0).astype(np.float32)
    sh = (rng.normal(size=(n, 16, 3)) * 0.3).astype(np.float32); sh[:, 0] += 1.0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")
    scene = drv.r.upload(Gaussians(t(means), t(s), t(quats), t(opac), t(sh), 3))
    for yaw in (0.0, 0.35, -0.6):
        c, si = np.cos(yaw), np.sin(yaw)
        V = np.eye(4); V[:3, :3] = np.array([[c, 0, -si], [0, 1, 0], [si, 0, c]])
        cam = Camera(640, 480, 400.0, 400.0, 320.0, 240.0, V)
        prod = drv.r.render(cam, scene, fine_tiles=False).clone()
        st = drv.r.last_stats
        ref = drv.r.render(cam, scene, loose_cull=True)
        st_ref = drv.r.last_stats
        assert (prod == ref).all(), f"yaw {yaw}: {(prod != ref).sum().item()} values differ"
        assert st["n_visible"] == st_ref["n_visible"] and st["d_total"] < st_ref["d_total"]
        assert torch.isfinite(prod).all()
        # ... and through 8x8-pixel tiles (what a 640x480 frame of smaller splats gets by default, sgs_tuning.fine_tile_pixels / _growth; forced
        # here — these splats are large, the library itself keeps 16x16): the same splats reach
        # every pixel, the blend's coordinates are relative to another origin; held against the ORACLE here, every pixel, threshold-sensitive
        # ones two-sidedly (the needles' exponents cancel from ~1e6 to ~1: the scene the completed-square form was made for)
        with pc.forced_fine(drv):
            fine = drv.r.render(cam, scene).cpu().numpy()
        st_f = drv.r.last_stats
        assert st_f["n_tiles"] == 80 * 60 and st_f["n_visible"] == st["n_visible"]
        ocam = onp.Camera(640, 480, 400.0, 400.0, 320.0, 240.0, V.astype(np.float32))
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        o_ref, aux = oracle_c.render(f32(means), f32(s), f32(quats), f32(opac), f32(sh), 3, ocam)
        assert st_f["n_visible"] == aux["n_visible"]
        assert_frame_close(fine, o_ref, aux["margin"], aux["recheck"], what=f"adversarial splats, yaw {yaw} [fine tiles]")
        assert_frame_tight(fine, o_ref, aux, what=f"adversarial splats, yaw {yaw} [fine tiles]")
        aux["recheck"].close()
    scene.free()


@pytest.mark.parametrize("case", __import__("known_answer_cases").ALL, ids=lambda f: f.__name__)
def test_kernels_against_closed_form_answers(drv, case):
    """The analytic cases that pin the oracle, run straight against the HIP path — no oracle involved."""
    case(drv)
    with pc.forced_fine(drv):              # ... and through the fine tiles a frame this small may get (the library decides per frame)
        case(drv)


def test_against_committed_golden_fixture(drv):
    """The HIP path against tests/golden/config1_golden.npz — no oracle run involved."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config1_golden.npz"))
    scene, _ = onp.config1_scene(n=int(g["n"]), seed=int(g["seed"]))
    cam = onp.Camera(int(g["width"]), int(g["height"]), float(g["f"]), float(g["f"]), 64.0, 64.0, np.eye(4, dtype=np.float32))
    drv.upload(*scene)
    prod, st_prod = drv.render(cam, fine=False)                       # production: tight bin rects, lazy sort (16x16-pixel tiles, as the hooks)
    img, st = drv.render(cam, full_sort=True, loose_cull=True)          # reference binning: the fixture's integer structures
    assert (prod == img).all() and st_prod["d_total"] <= st["d_total"]
    off, ids, _, _ = drv.intermediates()
    assert st["d_total"] == int(g["D"]) and st["n_visible"] == int(g["n_visible"]) and st["d_fetched"] == int(g["D_f"])
    assert (off == g["offsets"]).all() and (ids == g["ids"]).all()
    assert_frame_close(img, g["image"], g["margin"], stored_variants(g["flag_yx"], g["flag_ptr"], g["flag_rgb"]), what="golden config1")
    gaux = dict(n_contrib=g["n_contrib"], margin=g["margin"], recheck=stored_variants(g["flag_yx"], g["flag_ptr"], g["flag_rgb"]))
    assert_frame_tight(img, g["image"], gaux, what="golden config1")
    with pc.forced_fine(drv):
        fine, st_fine = drv.render(cam)                               # ... and through fine tiles
    assert st_fine["n_tiles"] > st_prod["n_tiles"] and st_fine["n_visible"] == int(g["n_visible"])
    assert_frame_close(fine, g["image"], g["margin"], stored_variants(g["flag_yx"], g["flag_ptr"], g["flag_rgb"]), what="golden config1 [fine tiles]")
    assert_frame_tight(fine, g["image"], gaux, what="golden config1 [fine tiles]")


def test_batch_equals_single_frames(drv):
    from sage_gs import Camera, scenes
    sc = scenes.make_room(60_000, seed=4)
    cams = scenes.room_cameras(sc, 640, 480, n_positions=1, n_yaw=6, seed=4)
    g = scenes.to_gaussians(sc, "cuda:0")
    scene = drv.r.upload(g)
    batch, stats = drv.r.render_batch(cams, scene, want_stats=True)
    for i, c in enumerate(cams):
        single = drv.r.render(c, scene)
        assert (batch[i] == single).all()
        assert stats[i]["d_total"] == drv.r.last_stats["d_total"] and stats[i]["d_fetched"] == 0
    # the same batch counting D_f (the other instantiation of the composite): same frames, D_f as one frame at a time
    batch2, stats2 = drv.r.render_batch(cams, scene, want_stats=True, stats=True)
    assert (batch2 == batch).all()
    for i, c in enumerate(cams):
        drv.r.render(c, scene, stats=True)
        assert stats2[i]["d_fetched"] == drv.r.last_stats["d_fetched"] > 0
    scene.free()


def test_issue_paths_agree_on_random_scenes(drv):
    """Synchronous, pipelined, batched and banded frames of random scenes at random resolutions: the same bits."""
    from gpu_stress import stress_issue_paths
    assert stress_issue_paths(drv.r, 6, 123) == 0


def test_pipelined_frames_equal_sequential_frames(drv):
    """SGS_FLAG_PIPELINED: frames in flight on the library's lanes (own streams, own intermediates) must
    produce exactly the frames that one-at-a-time rendering produces, also when ordinary frames are mixed in."""
    import torch
    from sage_gs import scenes
    sc = scenes.make_room(150_000, seed=6)
    cams = scenes.room_cameras(sc, 800, 608, n_positions=2, n_yaw=6, seed=6)
    scene = drv.r.upload(scenes.to_gaussians(sc, "cuda:0"))
    seq = [drv.r.render(c, scene).clone() for c in cams]
    outs = [torch.full((608, 800, 3), -1.0, device="cuda:0") for _ in cams]
    for rep in range(2):                       # second round reuses lanes whose buffers are warm
        for c, o in zip(cams, outs):
            drv.r.render(c, scene, out=o, sync=False, pipelined=True)
        st = drv.r.sync()
        assert st["d_total"] > 0
        for a, b in zip(seq, outs):
            assert (a == b).all()
        # an ordinary frame right after pipelined ones (lane 0 may still be busy when it is enqueued)
        drv.r.render(cams[0], scene, out=outs[0], sync=False, pipelined=True)
        drv.r.render(cams[1], scene, out=outs[1], sync=False, pipelined=True)
        drv.r.render(cams[2], scene, out=outs[2], sync=False, pipelined=True)
        drv.r.render(cams[3], scene, out=outs[3], sync=False, pipelined=True)
        plain = drv.r.render(cams[4], scene)   # synchronous, lane 0, caller's stream
        assert (plain == seq[4]).all()
        for k in range(4):
            assert (outs[k] == seq[k]).all()
    scene.free()


def test_asynchronous_rgbd_frames_equal_synchronous_frames(drv):
    """sgs_render_rgbd with SGS_FLAG_ASYNC | SGS_FLAG_PIPELINED: eight cameras in flight on the library's lanes, each with its own `out`
    and `out_aux` (pre-filled), every other one over a background — after ONE sync() every RGB and every depth / coverage buffer equals
    the synchronous render bit for bit (nothing written late, nothing written into another lane's frame), twice (warm lanes)."""
    import torch
    from sage_gs import RenderConfig, scenes
    sc = scenes.make_room(150_000, seed=6)
    cams = scenes.room_cameras(sc, 800, 608, n_positions=2, n_yaw=4, seed=6)
    assert len(cams) == 8
    scene = drv.r.upload(scenes.to_gaussians(sc, "cuda:0"))
    cfg_of = lambda i: RenderConfig(background=pc.BG) if i % 2 else None
    want = []
    for i, c in enumerate(cams):
        rgb, aux = drv.r.render(c, scene, config=cfg_of(i), return_aux=True)
        want.append((rgb.clone(), aux.clone()))
        assert (drv.r.render(c, scene, config=cfg_of(i)) == rgb).all(), "the AUX instantiation changed the colours"
    for rep in range(2):
        outs = [(torch.full((608, 800, 3), pc.SENTINEL, device="cuda:0"), torch.full((608, 800, 2), pc.SENTINEL, device="cuda:0")) for _ in cams]
        for i, (c, (o, oa)) in enumerate(zip(cams, outs)):
            drv.r.render(c, scene, config=cfg_of(i), out=o, out_aux=oa, sync=False, pipelined=True)
        st = drv.r.sync()
        assert st["d_total"] > 0
        for i, ((o, oa), (w_rgb, w_aux)) in enumerate(zip(outs, want)):
            assert (o == w_rgb).all() and (oa == w_aux).all(), f"round {rep}: pipelined RGB-D frame {i} differs from the synchronous one"
    assert (want[0][1][..., 1] > 0.5).any() and (want[1][0] != drv.r.render(cams[1], scene)).any()
    # ... and render_batch over a background (the TF instantiation with one frame per blockIdx.y) equals the frames rendered alone
    batch = drv.r.render_batch(cams, scene, config=RenderConfig(background=pc.BG))
    for i, c in enumerate(cams):
        assert (batch[i] == drv.r.render(c, scene, config=RenderConfig(background=pc.BG))).all(), f"frame {i} of a batch over a background differs from the frame alone"
    scene.free()


# ---- the TF and AUX instantiations at scale ----------------------------------------------------------------------------------------
def _variants_at_scale(drv, sc, ocam, what, fine=False):
    """check_variants_against_oracle on a frame of a full-size scene uploaded in `drv`: the black-background frame is first held to the
    oracle (image and counts), as the shared check presumes."""
    img, st = drv.render(ocam, stats=False, fine=False)
    ref, aux = oracle_c.render(*sc.as_tuple(), ocam, want="image")
    assert st["n_visible"] == aux["n_visible"]
    assert_frame_close(img, ref, aux["margin"], aux["recheck"], what=what)
    assert_frame_tight(img, ref, aux, what=what)
    aux["recheck"].close()
    v = pc.check_variants_against_oracle(drv, sc.as_tuple(), ocam, what=what, fine=fine)
    assert (v["img0"] == img).all()
    return v


def test_3m_scene_background_and_rgbd_vs_oracle(drv, big_scene):
    """BASELINE configs[2] (make_room(3 000 000, seed 2), SH degree 3): the TF and AUX instantiations of the composite — a background of
    (0.25, 0.5, 0.75), the depth / coverage outputs — against the oracle rendered with the same config, whole frames: 1920x1080 at two
    poses of the bench's sweep (129, the slowest, and 77), 640x480 (through 16x16-pixel tiles and through the fine tiles, forced; and the
    tiling the library picks there by itself is one of the two, bit for bit) and 3840x2160 (one pose of the yaw sweep)."""
    from sage_gs import scenes
    sc, _ = big_scene
    drv.upload(*sc.as_tuple())
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=4, n_yaw=64, seed=2)
    for pid in (129, 77):
        _variants_at_scale(drv, sc, _ocam(cams[pid], sc), f"3M @1080p bench pose {pid} (TF / AUX)")
    ocam = _ocam(scenes.room_cameras(sc, 640, 480, n_positions=4, n_yaw=64, seed=2)[129], sc)
    v = _variants_at_scale(drv, sc, ocam, "3M @640x480 pose 129 (TF / AUX)", fine=True)
    assert "fine" in v and v["st_aux"]["max_tile_len"] > 4096
    rgb_d, aux_d, st_d = drv.render_aux(ocam, pc.with_background(None, pc.BG))          # the library's own choice of tiling
    pick = v if st_d["n_tiles"] == v["st_aux"]["n_tiles"] else v["fine"] if st_d["n_tiles"] == v["fine"]["st_aux"]["n_tiles"] else None
    assert pick is None or ((rgb_d == pick["img_bg"]).all() and (aux_d == pick["aux"]).all()), "the default tiling's RGB-D frame is not that tiling's frame"
    cam4k = scenes.sweep_cameras(sc, 3840, 2160, n=360, seed=2)[77]
    _variants_at_scale(drv, sc, _ocam(cam4k, sc), "3M @3840x2160 sweep pose 77 (TF / AUX)")


def test_trained_like_3m_background_and_rgbd_vs_oracle(drv):
    """The trained-like 3 M scene (D = 28 M records at 1080p) at pose 129 of the bench's sweep through the TF and AUX instantiations."""
    from sage_gs import scenes
    sc = scenes.make_trained_like(3_000_000, seed=2)
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=4, n_yaw=64, seed=2)
    drv.set_record_capacity(96 << 20)
    drv.upload(*sc.as_tuple())
    v = _variants_at_scale(drv, sc, _ocam(cams[129], sc), "trained-like 3M @1080p pose 129 (TF / AUX)")
    assert v["st_aux"]["d_total"] > 10_000_000


def test_room_500k_background_and_rgbd_vs_oracle(drv):
    """BASELINE configs[1] (make_room(500 000, seed 1), 1920x1080): one pose through the TF and AUX instantiations."""
    from sage_gs import scenes
    sc = scenes.make_room(500_000, seed=1)
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=2, n_yaw=8, seed=1)
    drv.upload(*sc.as_tuple())
    _variants_at_scale(drv, sc, _ocam(cams[2], sc), "config2 500k cam 2 (TF / AUX)")


def test_pack_rgba8(drv):
    import torch
    rgb = torch.rand((37, 53, 3), device="cuda:0") * 1.4 - 0.2
    out = drv.r.pack_rgba8(rgb).cpu().numpy()
    exp = (np.clip(rgb.cpu().numpy(), 0, 1) * 255.0 + 0.5).astype(np.uint8)
    assert (out[..., :3] == exp).all() and (out[..., 3] == 255).all()
    # the optional Reinhard operator of the reference's stage (template.usda:102,196): x / (1 + x) before quantisation
    tm = drv.r.pack_rgba8(rgb, tonemap="reinhard").cpu().numpy()
    x = np.maximum(rgb.cpu().numpy(), 0.0)
    exp_tm = (np.clip(rgb.cpu().numpy() / (1.0 + x), 0, 1) * 255.0 + 0.5).astype(np.uint8)
    assert np.abs(tm[..., :3].astype(int) - exp_tm.astype(int)).max() <= 1 and (tm[..., 3] == 255).all()


def test_render_function_surface():
    """render(camera, gaussians) — the drop-in call named by BASELINE.json."""
    import torch
    from sage_gs import Camera, render, scenes
    sc = scenes.config1(2000)
    g = scenes.to_gaussians(sc, "cuda:0")
    cam = Camera(256, 256, 128.0, 128.0, 128.0, 128.0, np.eye(4))
    img = render(cam, g)
    assert isinstance(img, torch.Tensor) and img.shape == (256, 256, 3) and img.dtype == torch.float32 and img.is_cuda
    ocam = onp.Camera(256, 256, 128.0, 128.0, 128.0, 128.0, np.eye(4, dtype=np.float32))
    ref, aux = oracle_c.render(*sc.as_tuple(), ocam)
    assert_frame_close(img.cpu().numpy(), ref, aux["margin"], aux["recheck"], what="render()")
    assert_frame_tight(img.cpu().numpy(), ref, aux, what="render()")


# ---- "next" rows on the GPU ------------------------------------------------------------
def _pose_points(n=None):
    """(position, rotation) pairs the reference's own trajectory code produced (tests/golden/pose_golden.json:
    `points_after` of trajectory_2d_to_3d.transform_trajectory_points)."""
    import json, os
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_golden.json")))
    pts = [c["points_after"][0] for c in g["cases"]]
    return pts if n is None else pts[:n]


def _oracle_view(sc, cam):
    """oracle_np.Camera for a renderer Camera + the scene's model->world transform (what Renderer._c_camera folds in)."""
    view = (np.asarray(cam.view, np.float64) @ np.asarray(sc.model_to_world, np.float64)).astype(np.float32)
    return onp.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, view)


def _u8(img):
    return (np.clip(np.asarray(img, np.float64), 0, 1) * 255.0 + 0.5).astype(np.uint8)


def test_ply_scene_against_the_oracle(drv, tmp_path):
    """f-1: a scene written to a standard 3DGS PLY, loaded back and rendered by the HIP path — against the ORACLE's
    render of the SAME loaded arrays, with the suite's ordinary checker (per-pixel 1e-3, threshold-sensitive pixels two-sidedly at the
    ordinary 1e-4 margin; rounds 3-5 rendered the oracle on the arrays that were WRITTEN and widened the margin 20x to absorb the fp32
    round trip of log-scales and logit opacities through the file).  That round trip is checked on the arrays themselves."""
    from sage_gs import ply, scenes
    sc = scenes.make_room(30_000, seed=6)
    path = str(tmp_path / "room.ply")
    ply.save_ply(path, *sc.as_tuple())
    arrays = ply.load_ply(path)
    assert arrays[5] == 3 and arrays[0].shape == (30_000, 3)
    g = ply.to_gaussians(arrays, "cuda:0", sc.model_to_world)
    w_m, w_s, w_q, w_o, w_sh, _ = sc.as_tuple()
    assert np.array_equal(arrays[0], w_m) and np.allclose(arrays[1], w_s, rtol=3e-6) and np.allclose(arrays[3], w_o, rtol=1e-5, atol=1e-7)
    assert np.array_equal(arrays[4], w_sh) and np.allclose(arrays[2], w_q / np.linalg.norm(w_q, axis=1, keepdims=True), atol=1e-6)
    for k, cam in enumerate(scenes.room_cameras(sc, 640, 480, n_positions=1, n_yaw=4, seed=6)[1:3]):
        img = drv.r.render(cam, g).cpu().numpy()
        ref, aux = oracle_c.render(*arrays, _oracle_view(sc, cam), want="image")
        assert_frame_close(img, ref, aux["margin"], aux["recheck"], what=f"3DGS .ply scene, camera {k}")
        assert_frame_tight(img, ref, aux, what=f"3DGS .ply scene, camera {k}")
        aux["recheck"].close()
        assert img.max() > 0.2


@pytest.mark.parametrize("deg", [3, 0])
def test_compressed_ply_scene_against_the_oracle(drv, tmp_path, deg):
    """f-1, the format InteriorGS actually ships (PlayCanvas compressed.ply, README.md:210-231 of the reference): a scene is quantised
    into a file (chunk tables, 16-byte vertices, and at degree 3 the 8-bit `sh` element), the file's payload goes to the device AS IT IS
    (Renderer.upload_compressed: dequantised by the layout kernel, Z-order made by the device radix sort) and the HIP frame is held
    against the ORACLE's frame of the arrays THE DEVICE HOLDS (SGS_BUF_SCENE_GEOM / _SH: its own decode) with the suite's ordinary checker
    — rounds 4-5 rendered the oracle on NumPy's decode and widened the flag margin 20x to absorb the few ulp between the device's exp / sqrt
    and NumPy's — and against the oracle's frame of the ORIGINAL arrays within what the quantisation can move.  The device's decode is
    compared with NumPy's array by array."""
    from sage_gs import ply, scenes
    from sage_gs import _capi
    sc = scenes.make_room(30_000, seed=9)
    m, s_, q, o, sh, _ = sc.as_tuple()
    # (Z-order the scene before quantising, as a converter would: a chunk of 256 then spans decimetres, not the flat)
    key = np.lexsort((m[:, 0] // 0.5, m[:, 1] // 0.5, m[:, 2] // 0.5))
    m, s_, q, o, sh = m[key], s_[key], q[key], o[key], sh[key][:, :(deg + 1) ** 2]
    path = str(tmp_path / f"room_c{deg}.ply")
    ply.save_compressed_ply(path, m, s_, q, o, sh, deg)
    arrays = ply.load_compressed_ply(path, sh_decode="bin_centre")
    assert arrays[5] == deg
    payload = ply.read_compressed_payload(path)
    assert payload[1].shape == (30_000, 4) and (payload[2] is None) == (deg == 0)
    scene = drv.r.upload_compressed(*payload, model_to_world=sc.model_to_world, sh_decode="bin_centre")
    cams = scenes.room_cameras(sc, 640, 480, n_positions=1, n_yaw=4, seed=9)[1:3]
    held = None
    for k, cam in enumerate(cams):
        img = drv.r.render(cam, scene).cpu().numpy()
        if held is None:                                  # the scene as the device decoded it (by original index)
            gd = drv.r.debug_buffer(_capi.BUF_SCENE_GEOM, np.float32).reshape(-1, 11)
            shd = drv.r.debug_buffer(_capi.BUF_SCENE_SH, np.float32).reshape(len(m), -1, 3)
            held = (gd[:, 0:3].copy(), gd[:, 4:7].copy(), gd[:, 7:11].copy(), gd[:, 3].copy(), shd.copy(), deg)
        view = _oracle_view(sc, cam)
        ref, aux = oracle_c.render(*held, view, want="image")
        assert_frame_close(img, ref, aux["margin"], aux["recheck"], what=f"compressed .ply scene (degree {deg}), camera {k}")
        assert_frame_tight(img, ref, aux, what=f"compressed .ply scene (degree {deg}), camera {k}")
        aux["recheck"].close()
        orig, _ = oracle_c.render(m, s_, q, o, sh, deg, view, want="image")
        d0 = np.abs(img.astype(np.float64) - orig)
        assert d0.mean() < 0.03 and img.max() > 0.2       # quantisation: centimetres of position, 1/255 of colour and opacity
    assert np.array_equal(held[4][:, 1:], arrays[4][:, 1:]) and np.allclose(held[4][:, 0], arrays[4][:, 0], atol=1e-6)      # SH: NumPy's decode exactly (DC to rounding)
    g = drv.r.debug_buffer(_capi.BUF_SCENE_GEOM, np.float32).reshape(-1, 11)
    assert np.allclose(g[:, 0:3], arrays[0], atol=2e-6) and np.allclose(g[:, 4:7], arrays[1], rtol=5e-6) and np.allclose(g[:, 3], arrays[3], atol=1e-7)
    assert np.allclose(g[:, 7:11], arrays[2], atol=3e-6)
    scene.free()


@pytest.mark.parametrize("deg", [3, 2, 1, 0])
def test_compressed_scene_keeps_its_sh_bytes_in_hbm_and_renders_the_same_frames(drv, tmp_path, deg):
    """A scene uploaded from the compressed payload keeps its 8-bit SH coefficients as BYTES in HBM (64 B per Gaussian at degree 3 where
    the fp32 rows take 192 B) and k_preprocess dequantises them every frame.  The same scene as fp32 rows — the device-decoded geometry
    (SGS_BUF_SCENE_GEOM) and the dequantised coefficients (SGS_BUF_SCENE_SH) uploaded through sgs_scene_upload, the layout of rounds 1-4
    — must render the SAME frames, bit for bit, with identical N_v / D / D_f; the coefficients are NumPy's decode of the bytes exactly."""
    from sage_gs import ply, scenes
    from sage_gs import _capi
    import torch
    from sage_gs.renderer import Gaussians
    sc = scenes.make_room(120_000, seed=4)
    m, s_, q, o, sh, _ = sc.as_tuple()
    key = np.lexsort((m[:, 0] // 0.5, m[:, 1] // 0.5, m[:, 2] // 0.5))
    m, s_, q, o, sh = m[key], s_[key], q[key], o[key], sh[key][:, :(deg + 1) ** 2]
    path = str(tmp_path / f"room_packed_{deg}.ply")
    ply.save_compressed_ply(path, m, s_, q, o, sh, deg)
    chunks, packed, shb, deg_file = ply.read_compressed_payload(path)
    assert deg_file == deg
    scene_c = drv.r.upload_compressed(chunks, packed, shb, deg, model_to_world=sc.model_to_world, sh_decode="bin_centre")
    cams = scenes.room_cameras(sc, 1024, 768, n_positions=2, n_yaw=4, seed=4)[:5]
    frames, stats = [], []
    for cam in cams:
        frames.append(drv.r.render(cam, scene_c, stats=True).clone()); stats.append(dict(drv.r.last_stats))
    g = drv.r.debug_buffer(_capi.BUF_SCENE_GEOM, np.float32).reshape(-1, 11)
    shd = drv.r.debug_buffer(_capi.BUF_SCENE_SH, np.float32).reshape(len(m), -1, 3)
    if deg > 0:
        want = (shb.reshape(len(m), 3, -1).transpose(0, 2, 1).astype(np.float32) / 256.0 - 0.5) * 8.0 + 4.0 / 256.0      # ply.load_compressed_ply's decode
        assert np.array_equal(shd[:, 1:], want.astype(np.float32))
    scene_c.free()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    if deg == 3:     # the other readings of a coefficient byte: the kernel's arithmetic (fp64 on the device for linear255) is NumPy's, code for code
        shb2 = shb.copy(); shb2[:300] = np.arange(300)[:, None] % 256
        for mode in ("linear255", "bin_centre_ends"):
            sm = drv.r.upload_compressed(chunks, packed, shb2, deg, model_to_world=sc.model_to_world, sh_decode=mode)
            fm = drv.r.render(cams[0], sm).clone()
            got = drv.r.debug_buffer(_capi.BUF_SCENE_SH, np.float32).reshape(len(m), -1, 3)
            assert np.array_equal(got[:, 1:], ply.decode_sh_bytes(shb2, mode).reshape(len(m), 3, -1).transpose(0, 2, 1)), mode
            sm.free()
            sf = drv.r.upload(Gaussians(t(g[:, 0:3]), t(g[:, 4:7]), t(g[:, 7:11]), t(g[:, 3]), t(got), deg, sc.model_to_world))
            assert bool((drv.r.render(cams[0], sf) == fm).all()), mode          # (what k_preprocess dequantised == those floats)
            sf.free()
    scene_f = drv.r.upload(Gaussians(t(g[:, 0:3]), t(g[:, 4:7]), t(g[:, 7:11]), t(g[:, 3]), t(shd), deg, sc.model_to_world))
    for cam, f, st in zip(cams, frames, stats):
        f32 = drv.r.render(cam, scene_f, stats=True)
        st32 = drv.r.last_stats
        assert bool((f32 == f).all()) and float(f.max()) > 0.2
        assert (st32["n_visible"], st32["d_total"], st32["d_fetched"]) == (st["n_visible"], st["d_total"], st["d_fetched"]) and st["n_visible"] > 1_000
        assert deg == 0 or st["bytes"]["preprocess"] < st32["bytes"]["preprocess"]
    scene_f.free()


def test_ply_scene_at_full_size(drv, tmp_path):
    """f-1 at the size of configs[2]: a 3 M-Gaussian scene (trained-3DGS statistics, SH degree 3: a 744-MB file) written to
    a standard 3DGS PLY and read back; the loaded arrays go through `scenes.scene_from_arrays` + `ply.to_gaussians` (the
    path of `bench.py --scene`) and the frame must equal the frame of the same arrays uploaded directly, bit for bit,
    with identical N_v / D; against the arrays that were WRITTEN (an fp32 log/exp, logit/sigmoid round trip away) the
    frame stays within the parity tolerance on all but the few pixels such a perturbation moves across a threshold."""
    from sage_gs import ply, scenes
    sc = scenes.make_trained_like(3_000_000, seed=2)
    path = str(tmp_path / "scene_3m.ply")
    ply.save_ply(path, *sc.as_tuple())
    assert os.path.getsize(path) > 3_000_000 * 62 * 4
    arrays = ply.load_ply(path)
    assert arrays[5] == 3 and arrays[0].shape == (3_000_000, 3) and arrays[4].shape == (3_000_000, 16, 3)
    loaded = scenes.scene_from_arrays(arrays)
    assert np.allclose(loaded.extent, sc.extent, atol=0.5) and np.array_equal(loaded.model_to_world, scenes.MODEL_TO_WORLD)
    cams = scenes.room_cameras(loaded, 1920, 1080, n_positions=2, n_yaw=8, seed=2)
    g_file = drv.r.upload(ply.to_gaussians(arrays, "cuda:0", loaded.model_to_world))
    a = [drv.r.render(cams[i], g_file, stats=True).clone() for i in (1, 11)]
    st_a = dict(drv.r.last_stats)
    g_file.free()
    g_direct = drv.r.upload(scenes.to_gaussians(loaded, "cuda:0"))
    b = [drv.r.render(cams[i], g_direct, stats=True).clone() for i in (1, 11)]
    st_b = dict(drv.r.last_stats)
    g_direct.free()
    for x, y in zip(a, b):
        assert bool((x == y).all())
    assert st_a["n_visible"] == st_b["n_visible"] > 100_000 and st_a["d_total"] == st_b["d_total"] and st_a["d_fetched"] == st_b["d_fetched"]
    g_orig = drv.r.upload(scenes.to_gaussians(sc, "cuda:0"))
    c = [drv.r.render(cams[i], g_orig).clone() for i in (1, 11)]
    g_orig.free()
    for x, y in zip(a, c):
        d = (x - y).abs().max(dim=-1).values
        assert float((d >= 1e-3).float().mean()) < 2e-3 and float(d.median()) < 1e-5
    import json
    print("[trained-like 3M @1080p] N_v", st_a["n_visible"], "D", st_a["d_total"], "D_f", st_a["d_fetched"], "max tile", st_a["max_tile_len"])


def test_gscamera_adapter_against_the_oracle(drv):
    """f-3: the Isaac Camera protocol (set_world_pose / get_world_pose / get_rgba / get_current_frame / get_depth) over
    the renderer, at poses the reference's own trajectory code produced; the uint8 frame `get_rgba()` returns is checked
    against the ORACLE's render of the same view (<= 1 level), the depth against the oracle's expected depth."""
    from sage_gs import scenes
    from sage_gs.adapter import GsCamera
    from sage_gs import camera as cc
    sc = scenes.make_room(30_000, seed=6)
    scene = drv.r.upload(scenes.to_gaussians(sc, "cuda:0"))
    cam = GsCamera(drv.r, scene, prim_path="/World/NaVILACamera", frequency=30, resolution=(320, 240))
    cam.initialize()
    for pt in _pose_points(4):
        pos, orient = cc.datagen_pose(pt)
        cam.set_world_pose(position=np.array(pos, np.float32), orientation=np.array(orient, np.float32))
        p, o = cam.get_world_pose()
        assert np.allclose(p, pos) and np.allclose(o, orient) and abs(p[2] - 1.2) < 1e-6
        rgba = cam.get_rgba()
        assert rgba.shape == (240, 320, 4) and rgba.dtype == np.uint8 and (rgba[..., 3] == 255).all()
        ocam = _oracle_view(sc, cc.reference_camera(320, 240, p, o))            # the float32 pose the adapter holds
        ref, aux = oracle_c.render(*sc.as_tuple(), ocam, want="image")
        safe = aux["margin"] >= 1e-4
        assert np.abs(rgba[..., :3].astype(int) - _u8(ref).astype(int))[safe].max() <= 1, "get_rgba() vs the oracle"
        assert np.abs(rgba[..., :3].astype(int) - _u8(ref).astype(int)).max() <= 4        # threshold-sensitive pixels: <= c/255 + rounding
        frame = cam.get_current_frame()
        assert (frame["rgba"] == rgba).all() and frame["distance_to_image_plane"].shape == (240, 320)
        # depth: sum(T alpha z) / coverage where something was hit, inf elsewhere; get_depth() clips like simple_env.get_depth
        cov = 1.0 - aux["final_T"]
        hit = (cov > 1e-3) & safe
        exp = aux["depth_image"][hit] / cov[hit]
        assert np.abs(frame["distance_to_image_plane"][hit] - exp).max() < 2e-3 * max(1.0, exp.max())
        d = cam.get_depth()
        assert d.dtype == np.float32 and d.min() >= 0.1 and d.max() <= 6.5
        assert np.abs(d[hit] - np.clip(exp, 0.1, 6.5)).max() < 2e-3 * 6.5
        assert (d[cov < 1e-5] == 6.5).all()
    # get_rgba() hands out a fresh array by default: a SECOND camera of the same resolution on this renderer (a stereo pair) and later
    # frames leave an observation the caller kept intact; copy=False is the renderer's shared pinned ring, which comes round after two
    cam2 = GsCamera(drv.r, scene, prim_path="/World/Right", frequency=30, resolution=(320, 240))
    cam2.initialize()
    pts = _pose_points(4)
    for c_, pt in ((cam, pts[0]), (cam2, pts[1])):
        pos, orient = cc.datagen_pose(pt)
        c_.set_world_pose(position=np.array(pos, np.float32), orientation=np.array(orient, np.float32))
    first = cam.get_rgba()
    keep = first.copy()
    views = [cam2.get_rgba(), cam.get_rgba(), cam2.get_rgba()]
    assert (first == keep).all() and not np.shares_memory(first, views[1]) and (views[0] == views[2]).all() and (views[1] == keep).all()
    v0 = cam.get_rgba(copy=False)
    cam2.get_rgba(copy=False)
    v2 = cam.get_rgba(copy=False)
    assert np.shares_memory(v0, v2) and (v2 == keep).all()          # (the ring of depth 2: the third frame lands in the first one's buffer)
    scene.free()


def test_sweep_driver_against_the_oracle(drv, tmp_path):
    """f-2: action_groundtruth.json -> images/trajectory_<id>/<scene>_<traj>_<idx>.jpg + image_metadata.json in the reference's
    layout, AND every frame handed to the JPEG encoder equals the ORACLE's render of that waypoint's view to one uint8
    level (waypoints: poses produced by the reference's own trajectory code, tests/golden/pose_golden.json)."""
    import json, os
    from sage_gs import scenes, sweep
    from sage_gs import camera as cc
    sc = scenes.make_room(30_000, seed=6)
    scene = drv.r.upload(scenes.to_gaussians(sc, "cuda:0"))
    pts = [{"point_id": i, "position": p["position"], "rotation": p["rotation"]} for i, p in enumerate(_pose_points(5))]
    gt = {"groundtruth_data": [{"trajectory_id": "3", "instruction_index": 0, "sampled_points": pts},
                               {"trajectory_id": "3", "instruction_index": 1, "sampled_points": pts}]}
    ap = tmp_path / "action_groundtruth.json"; ap.write_text(json.dumps(gt))
    out = tmp_path / "images"
    seen = {}
    n = sweep.run(drv.r, scene, sweep.load_trajectories(str(ap)), "0007", str(out), resolution=(256, 192),
                  on_frame=lambda tid, i, rgb: seen.__setitem__((tid, i), rgb.copy()))
    assert n == 5 and sorted(seen) == [("3", i) for i in range(5)]
    files = sorted(os.listdir(out / "images" / "trajectory_3"))
    assert files == [f"0007_3_{i:03d}.jpg" for i in range(5)]
    meta = json.load(open(out / "image_metadata.json"))
    assert meta["scene_id"] == "0007" and meta["image_resolution"] == [256, 192] and meta["camera_settings"] == {"focal_length": 8.0, "height": 1.2}
    assert meta["sequences"][0]["frame_filenames"] == files and len(meta["sequences"][0]["trajectory_sampled_points"]) == 5
    from PIL import Image
    for i, pt in enumerate(pts):
        pos, orient = cc.datagen_pose(pt)
        ocam = _oracle_view(sc, cc.reference_camera(256, 192, pos, orient))
        ref, aux = oracle_c.render(*sc.as_tuple(), ocam, want="image")
        safe = aux["margin"] >= 1e-4
        d = np.abs(seen[("3", i)].astype(int) - _u8(ref).astype(int))
        assert d[safe].max() <= 1 and d.max() <= 4, f"sweep frame {i} vs the oracle"
        im = np.asarray(Image.open(out / "images" / "trajectory_3" / files[i]))
        assert im.shape == (192, 256, 3) and np.abs(im.astype(int) - seen[("3", i)].astype(int)).mean() < 3.0      # JPEG q95
    scene.free()


def test_fine_tile_decision_follows_the_growth_of_the_record_count(drv):
    pc.case_fine_tile_decision(drv)


def test_a_batch_whose_frames_choose_different_tilings(drv):
    """fine_shift_of decides per camera (the growth of the record count under a split depends on how large the splats are on THAT
    screen); the frames of a launch group share one grid of tiles, so a batch's groups end where the choice changes.  A batch that zooms
    in and out of a room — focal lengths from a quarter to four times the reference lens — must hold every frame as the single-frame
    call renders it, bit for bit, with the statistics the single call reports; and both tilings must occur, or the test proves nothing.
    The statistics compared: every field but the stage times, `retries` and `n_deep_windows`.  The last is not a property of the frame
    on the GPU: the SAME frame rendered alone three times reported 18, 17, 18 (zoom 0.3), 30, 28, 33 (zoom 0.25) and 24, 22, 23 windows,
    three batches 18, 18, 18 / 32, 30, 31 / 27, 21, 24, with identical pixels and identical values in every other field (a diagnostic
    of how the composite went about a tile, not of what it drew).  parity_cases.case_batch_stats_of_mixed_tilings (emulator) compares it too."""
    import torch
    from sage_gs import Camera, scenes
    sc = scenes.make_room(200_000, seed=9)
    base = scenes.room_cameras(sc, 640, 480, n_positions=2, n_yaw=4, seed=9)
    zooms = (1.0, 0.3, 3.5, 4.0, 0.25, 1.0, 3.0, 0.5, 0.3, 3.8, 1.2)
    cams = [Camera(c.width, c.height, c.fx * k, c.fy * k, c.cx, c.cy, c.view) for c, k in zip(base * 2, zooms)]
    scene = drv.r.upload(scenes.to_gaussians(sc, "cuda:0"))
    of_frame = lambda st: {k: v for k, v in pc.stats_without_times(st).items() if k != "n_deep_windows"}
    one, tiles, sts = [], [], []
    for c in cams:
        one.append(drv.r.render(c, scene).clone()); tiles.append(drv.r.last_stats["n_tiles"]); sts.append(drv.r.last_stats)
    assert set(tiles) == {40 * 30, 80 * 60}, tiles
    batch, bst = drv.r.render_batch(cams, scene, want_stats=True)
    outs = [torch.zeros_like(one[0]) for _ in cams]
    for c, o in zip(cams, outs):
        drv.r.render(c, scene, out=o, sync=False, pipelined=True)
    drv.r.sync()
    for i in range(len(cams)):
        assert bst[i]["n_tiles"] == tiles[i], (i, bst[i]["n_tiles"], tiles[i])
        assert of_frame(bst[i]) == of_frame(sts[i]), (i, bst[i], sts[i])     # (bytes[] too: of the frame's OWN grid)
        assert (batch[i] == one[i]).all() and (outs[i] == one[i]).all(), f"frame {i} (zoom {zooms[i]}) depends on how it is issued"
    scene.free()


def test_frames_do_not_depend_on_the_tuning(drv):
    """include/sage_gs.h sgs_tuning (the library's whole tuning surface: it reads nothing from the environment): lanes in flight, frames per
    launch group, streams per batch, Z-order at upload.  Pipelined single frames and a batch under non-default values must equal, bit for
    bit, the frames of the default context; N_v and D too (the scene's layout order only decides which chunk a Gaussian shares)."""
    import torch
    from sage_gs import Renderer, scenes
    sc = scenes.make_room(150_000, seed=6)
    cams = scenes.room_cameras(sc, 800, 600, n_positions=2, n_yaw=5, seed=6)
    g = scenes.to_gaussians(sc, "cuda:0")
    scene = drv.r.upload(g)
    assert drv.r.tuning() == {"lanes": 3, "group": 8, "group_lanes": 2, "morton": 1, "record_capacity": drv.r.tuning()["record_capacity"],
                              "fine_tile_pixels": 640 * 480, "fine_tile_growth": 2.2}
    want, stats = [], []
    for c in cams:
        want.append(drv.r.render(c, scene).clone()); stats.append((drv.r.last_stats["n_visible"], drv.r.last_stats["d_total"]))
    scene.free()
    for kw in (dict(lanes=1, group=1, group_lanes=1), dict(lanes=8, group=8, group_lanes=1), dict(lanes=2, group=2, group_lanes=4),
               dict(lanes=5, group=3, group_lanes=2, morton=False), dict(lanes=16, group=4, group_lanes=4)):
        r = Renderer("cuda:0", **kw)
        t = r.tuning()
        assert all(t[k] == int(v) for k, v in kw.items()), (t, kw)
        s2 = r.upload(g)
        outs = [torch.zeros_like(want[0]) for _ in cams]
        for c, o in zip(cams, outs):
            r.render(c, s2, out=o, sync=False, pipelined=True)
        r.sync()
        batch, bst = r.render_batch(cams, s2, want_stats=True)
        for i in range(len(cams)):
            assert (outs[i] == want[i]).all() and (batch[i] == want[i]).all(), f"{kw}: frame {i} differs"
            assert (bst[i]["n_visible"], bst[i]["d_total"]) == stats[i]
        # changing it on a live context: the next frames run under the new values
        r.set_tuning(lanes=3, group=8, group_lanes=2)
        assert (r.render_batch(cams, s2)[0] == want[0]).all()
        s2.free(); r.close()
    # refused, with a message, not clamped
    r = Renderer("cuda:0")
    for bad in (dict(lanes=0), dict(lanes=17), dict(group=9), dict(group=8, group_lanes=3), dict(record_capacity=-5), dict(fine_tile_pixels=-1),
                dict(fine_tile_growth=0.5)):
        with pytest.raises(Exception, match="sgs_tuning"):
            r.set_tuning(**bad)
    # fine_tile_pixels / fine_tile_growth — the fields a frame depends on, to rounding: which tiles a frame of W x H pixels is rendered
    # through (here with the growth rule out of the way).  A frame issued alone, pipelined and in a batch is the same frame under every
    # value; 0 = SGS_FLAG_NO_FINE_TILES, bit for bit
    r.set_tuning(fine_tile_growth=1.0e9)
    s2 = r.upload(g)
    small = scenes.room_cameras(sc, 400, 300, n_positions=2, n_yaw=3, seed=6)
    w16 = [r.render(c, s2, fine_tiles=False).clone() for c in small]
    n16 = r.last_stats["n_tiles"]
    for fp, side in ((0, 16), (400 * 300, 8), (640 * 480, 8), (4 * 400 * 300, 4)):
        r.set_tuning(fine_tile_pixels=fp)
        one = [r.render(c, s2).clone() for c in small]
        assert r.last_stats["n_tiles"] == -(-400 // side) * -(-300 // side), (fp, side, r.last_stats["n_tiles"])
        outs = [torch.zeros_like(one[0]) for _ in small]
        for c, o in zip(small, outs):
            r.render(c, s2, out=o, sync=False, pipelined=True)
        r.sync()
        batch = r.render_batch(small, s2)
        for i in range(len(small)):
            assert (outs[i] == one[i]).all() and (batch[i] == one[i]).all(), f"fine_tile_pixels {fp}: frame {i} depends on how it is issued"
            d = (one[i] - w16[i]).abs().amax(dim=-1)
            assert float((d > 1e-5).float().mean()) < 1e-3 and float(d.median()) < 1e-6, (fp, i, float(d.max()))
            if side == 16:
                assert (one[i] == w16[i]).all()
    assert n16 == 25 * 19
    s2.free(); r.close()


def test_compressed_payload_known_answer_vectors_on_the_device(drv):
    """tests/golden/compressed_ply_kat.json — packed words written out by hand from the PlayCanvas layout (11-10-11 / 2+10-10-10 / 8-8-8-8,
    chunk min / max lerp, 8-bit SH), expected values in exact rational arithmetic by a script that imports nothing of this repo — through
    sgs_scene_upload_compressed on the GPU: what the layout kernel dequantised (SGS_BUF_SCENE_GEOM) and what k_preprocess evaluates
    (SGS_BUF_SCENE_SH) under each of the three readings of a coefficient byte; sh_decode has no default."""
    import sys
    sys.path.insert(0, os.path.dirname(__file__))
    from test_next_rows import _kat_payload, _check_kat
    from sage_gs import Camera, _capi
    cases, chunks, packed, shb = _kat_payload()
    n = len(cases)
    cam = Camera(64, 48, 50.0, 50.0, 32.0, 24.0, np.eye(4))
    for mode in ("bin_centre", "linear255", "bin_centre_ends"):
        scene = drv.r.upload_compressed(chunks, packed, shb, 3, sh_decode=mode)
        drv.r.render(cam, scene)
        g = drv.r.debug_buffer(_capi.BUF_SCENE_GEOM, np.float32).reshape(-1, 11)
        shd = drv.r.debug_buffer(_capi.BUF_SCENE_SH, np.float32).reshape(n, -1, 3)
        assert g.shape == (n, 11) and shd.shape == (n, 16, 3)
        _check_kat(cases, g[:, 0:3], g[:, 4:7], g[:, 7:11], g[:, 3], shd[:, 0, :], shd[:, 1:, :], mode=mode)
        scene.free()
    with pytest.raises(ValueError, match="sh_decode"):
        drv.r.upload_compressed(chunks, packed, shb, 3)
    drv.r.upload_compressed(chunks, packed, None, 0).free()            # degree 0: no coefficient bytes, nothing to specify


# ---- regrowth of the library's own buffers: a frame does not depend on what its context rendered before ------------------------------
def test_regrown_intermediates_leave_frames_unchanged():
    """One Renderer through every regrowth of a lane's intermediates — the tile arrays (64x48 -> 320x240), the splat arrays (2 000 ->
    20 000 Gaussians), the records (a capacity the larger frame overflows: the synchronous retry grows them) — and back to the first
    frame, which must be bit for bit what it was, and what a fresh Renderer renders."""
    from sage_gs import Renderer, scenes
    small, large = scenes.make_room(2_000, seed=5), scenes.make_room(20_000, seed=6)
    cam_a = scenes.room_cameras(small, 64, 48, n_positions=1, n_yaw=1, seed=5)[0]
    cam_b = scenes.room_cameras(small, 320, 240, n_positions=1, n_yaw=1, seed=5)[0]
    cam_c = scenes.room_cameras(large, 64, 48, n_positions=1, n_yaw=1, seed=6)[0]
    r = Renderer("cuda:0")
    try:
        s_small, s_large = r.upload(scenes.to_gaussians(small, "cuda:0")), r.upload(scenes.to_gaussians(large, "cuda:0"))
        a0 = r.render(cam_a, s_small).cpu().numpy()
        b0 = r.render(cam_b, s_small, stats=True).cpu().numpy()
        d_b = int(r.last_stats["d_total"])
        assert d_b > 2048, d_b                                   # (frame B's records do not fit the capacity set below)
        c0 = r.render(cam_c, s_large).cpu().numpy()
        r.set_record_capacity(2048)
        b1 = r.render(cam_b, s_small, stats=True).cpu().numpy()
        assert r.last_stats["retries"] >= 1, r.last_stats
        a1 = r.render(cam_a, s_small).cpu().numpy()
        c1 = r.render(cam_c, s_large).cpu().numpy()
        assert np.isfinite(a0).all() and a0.max() > 0.0
        assert (a1 == a0).all() and (b1 == b0).all() and (c1 == c0).all()
    finally:
        r.close()
    fresh = Renderer("cuda:0")
    try:
        assert (fresh.render(cam_a, fresh.upload(scenes.to_gaussians(small, "cuda:0"))).cpu().numpy() == a0).all()
    finally:
        fresh.close()


def test_regrown_scratch_of_the_mesh_path_the_encoders_and_the_resize():
    """The same for the other owners of scratch: mesh depth and ids through 64x48 -> 320x240 -> 64x48 and a record buffer of one entry
    (the retry grows it); JPEG and PNG files of 1, then 5, then 1 frames (the first file's bytes stay); a both-pass resize at two sizes."""
    import torch
    from sage_gs import Renderer, scenes
    v, t, part = scenes.make_room_mesh_parts(2_000, seed=3)
    room = scenes.make_room(2_000, seed=5)
    cam_a = scenes.room_cameras(room, 64, 48, n_positions=1, n_yaw=1, seed=5)[0]
    cam_b = scenes.room_cameras(room, 320, 240, n_positions=1, n_yaw=1, seed=5)[0]
    r = Renderer("cuda:0")
    try:
        mesh = r.upload_mesh(v, t, labels=part)
        d0 = r.render_mesh_depth(cam_a, mesh).cpu().numpy()
        i0, e0 = [x.cpu().numpy() for x in r.render_mesh_ids(cam_a, mesh, return_depth=True)]
        D0 = r.render_mesh_depth(cam_b, mesh).cpu().numpy()
        I0 = r.render_mesh_ids(cam_b, mesh).cpu().numpy()
        r.set_mesh_record_capacity(1)
        D1 = r.render_mesh_depth(cam_b, mesh).cpu().numpy()
        assert r.last_stats["retries"] >= 1, r.last_stats
        I1 = r.render_mesh_ids(cam_b, mesh).cpu().numpy()
        d1 = r.render_mesh_depth(cam_a, mesh).cpu().numpy()
        i1 = r.render_mesh_ids(cam_a, mesh).cpu().numpy()
        assert np.isfinite(d0).any() and (i0 >= 0).any()
        for got, want in ((d1, d0), (e0, d0), (i1, i0), (D1, D0), (I1, I0)):
            assert got.tobytes() == want.tobytes()

        scene = r.upload(scenes.to_gaussians(room, "cuda:0"))
        frames = torch.stack([r.render(c, scene).clone() for c in scenes.room_cameras(room, 64, 48, n_positions=1, n_yaw=5, seed=5)])
        depth = torch.from_numpy(np.where(np.isfinite(d0), d0, 0.0).astype(np.float32)).to("cuda:0").expand(5, -1, -1).contiguous()
        for enc in (r.encode_jpeg, r.encode_png):
            one, five, again = enc(frames[:1]), enc(frames), enc(frames[:1])
            assert len(five) == 5 and one[0] == five[0] == again[0] and len(one[0]) > 100
        one, five, again = [r.encode_png(depth[:k], format="depth16") for k in (1, 5, 1)]
        assert len(five) == 5 and one[0] == five[0] == again[0]

        big = torch.stack([r.render(cam_b, scene)] * 3)
        s0 = r.resize(frames[0], (40, 30)).cpu().numpy()
        s_big = r.resize(big, (100, 70)).cpu().numpy()
        s1 = r.resize(frames, (40, 30)).cpu().numpy()
        assert (s1[0] == s0).all() and (s_big[0] == s_big[2]).all() and (r.resize(big[1], (100, 70)).cpu().numpy() == s_big[1]).all()
    finally:
        r.close()


# ---- the front end's and the HBM sort's integer decisions, each sat on by a deterministic case (frontend_cases.py) ----------------------
@pytest.mark.parametrize("which", ["identity", "turned", "off_centre"])
def test_chunk_cull_margins(drv, which):
    fc.case_chunk_margins(drv, which)


def test_near_and_far_plane_at_equality_and_one_ulp_to_either_side(drv):
    fc.case_near_far_equality(drv)


@pytest.mark.parametrize("which", ["identity", "turned", "off_centre"])
def test_giants_beyond_both_jacobian_clamps_at_every_edge(drv, which):
    fc.case_clamped_giants(drv, which)


def test_needle_determinant_needs_fp64(drv):
    fc.case_needle_determinant(drv)


@pytest.mark.parametrize("resort", [False, True], ids=["runs_up_to_32", "with_a_run_of_33"])
def test_tie_runs_in_a_bucket_sorted_through_hbm(drv, resort):
    fc.case_short_tie_runs(drv, resort=resort)


def test_batch_groups_of_eight_frames(drv):
    fc.case_batch_groups_of_eight(drv)


@pytest.mark.parametrize("survivor", ["last", "first"])
def test_deep_tile_window_whose_only_survivor_is_its_last_or_first_record(drv, survivor):
    fc.case_deep_window_ends(drv, survivor)
