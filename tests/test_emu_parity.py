"""Kernel LOGIC under the wave64 emulator (CPU; see tests/hipemu/hip/hip_runtime.h): the product's
own kernel source, compiled for the host, must reproduce the oracle — queues bit-exactly, images within
the parity tolerance.  The same cases run on the real GPU in test_gpu_parity.py."""
import numpy as np
import pytest

import emu_harness
import oracle_np as onp
import frontend_cases as fc
import parity_cases as pc


FUZZ_VARIANT_SEEDS = tuple(range(9100, 9112))      # case_fuzz_variants: every seed with thresholds, background, aux and (3+ tile rows) bands


@pytest.fixture(scope="module")
def drv():
    d = emu_harness.EmuRenderer(record_capacity=1 << 21)
    yield d
    d.close()


def test_config1(drv):
    pc.case_config1(drv, n=10_000)


def test_sh_degrees(drv):
    pc.case_sh_degrees(drv, n=600)


def test_ragged_sizes(drv):
    pc.case_ragged(drv)


def test_seeded_random_frames(drv):
    pc.case_fuzz(drv, range(28))


def test_seeded_random_frames_with_needles_and_specks(drv):
    """Splats from far below a pixel to needles and pancakes the size of the scene (aspect ratios up to 1e4): what the
    completed-square form of q2 is for (seeds 8019 and 8036 failed the three-term form by 1.6e-3)."""
    pc.case_fuzz(drv, range(7000, 7020), 400, (200, 120), wild=True)


def test_seeded_random_frames_over_a_background_with_depth_and_coverage(drv):
    pc.case_fuzz_variants(drv, FUZZ_VARIANT_SEEDS)


def test_non_finite_gaussians_are_invisible_and_harmless(drv):
    pc.case_non_finite_gaussians(drv)
    pc.case_non_finite_gaussians(drv, n=700, res=(96, 64), seed=4)


def test_padding_lanes_stay_culled(drv):
    pc.case_padding_lanes(drv)


def test_empty_and_all_culled(drv):
    pc.case_empty(drv)


def test_tile_row_bands(drv):
    pc.case_tile_rows(drv, n=1200, res=(112, 100))


def test_chunk_bounds_skip_only_invisible_chunks(drv):
    pc.case_chunk_bounds(drv, n=6000, res=(208, 150))


@pytest.mark.parametrize("stride", [2, 3])
def test_interleaved_tile_rows(drv, stride):
    pc.case_interleaved_rows(drv, stride, n=1200, res=(112, 100))


def test_depth_ties(drv):
    pc.case_depth_ties(drv)


def test_big_depth_bucket(drv):
    pc.case_big_depth_bucket(drv, n_slab=1500)


def test_sort_classes(drv):
    pc.case_sort_classes(drv, sizes=(700, 2500, 6000, 9500), variant_switches=False)


def test_sparse_lists(drv):
    pc.case_sparse_lists(drv, n=5000, res=(40, 32))


def test_deep_tile(drv):
    pc.case_deep_tile(drv, n_back=5000)


def test_full_grid_splat(drv):
    pc.case_full_grid_splat(drv, res=(640, 368), variants=True)


def test_wide_band_of_tiles(drv):
    # 129 x 65 = 8385 tiles (more than SGS_WT super-tile counters would be, were they per tile): one window of 33 x 17 super-tiles
    pc.case_full_grid_splat(drv, res=(2064, 1040))


def test_depth_and_coverage_outputs(drv):
    pc.case_depth_aux(drv, n=1500, res=(96, 80))


def test_fine_tile_decision_follows_the_growth_of_the_record_count(drv):
    pc.case_fine_tile_decision(drv)


def test_batch_shares_scene_reads(drv):
    pc.case_batch_shares_scene_reads(drv)


def test_determinism(drv):
    pc.case_determinism(drv, n=1500)


def test_overflow_retry():
    d = emu_harness.EmuRenderer(record_capacity=1 << 16)
    try:
        pc.case_overflow_retry(d)
    finally:
        d.close()


def test_float_reciprocal_division_is_exact():
    """wave_expand() replaces idx / w by (unsigned)((idx + 0.5f) * (1.0f / w)); exact over every
    rect a 16384x16384 frame can produce (w <= 1024 tiles, idx < 2^20)."""
    for w in range(1, 1025):
        idx = np.arange(0, min(1 << 20, w * 1024), dtype=np.uint32)
        rw = np.float32(1.0) / np.float32(w)
        q = ((idx.astype(np.float32) + np.float32(0.5)) * rw).astype(np.uint32)
        assert (q == idx // w).all(), w


def test_against_committed_golden_fixture(drv):
    """The kernels (under the emulator) against tests/golden/config1_golden.npz — no oracle run involved."""
    import os
    from conftest import assert_frame_close, stored_variants
    from tight_parity import assert_frame_tight
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


def test_pipelined_frames_and_batch_rotate_over_lanes(drv):
    """Host logic of the frames in flight (sgs_api.hip): SGS_FLAG_PIPELINED frames and sgs_render_batch rotate over the
    context's lanes (own intermediates each; streams are synchronous under the emulator) and must produce the frames
    that ordinary one-at-a-time rendering produces; ordinary frames mixed in use lane 0."""
    import ctypes as C
    from sage_gs import _capi
    scene, _ = onp.config1_scene(n=3000, seed=4)
    drv.upload(*scene)
    lib, ctx = drv.lib, drv.ctx
    cams = []
    for k in range(5):
        V = np.eye(4, dtype=np.float32); V[0, 3] = 0.15 * k - 0.3
        cams.append(onp.Camera(96, 80, 70.0, 70.0, 48.0, 40.0, V))
    seq = [drv.render(c, stats=False)[0].copy() for c in cams]          # (the production instantiation, as the batch runs it)
    outs = [np.full((80, 96, 3), -1.0, np.float32) for _ in cams]
    cfg = lib.default_config()
    cfg.flags = _capi.FLAG_ASYNC | _capi.FLAG_PIPELINED
    for c, o in zip(cams, outs):
        cc = _capi.make_camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy, np.asarray(c.view, np.float32).reshape(4, 4).tolist())
        lib.check(lib.sgs_render(ctx, drv.scene, C.byref(cc), C.byref(cfg), 0, -1, o.ctypes.data, None, None), ctx)
    plain = drv.render(cams[2], stats=False)[0]           # an ordinary frame while pipelined ones are pending
    st = _capi.SgsStats()
    lib.check(lib.sgs_frame_sync(ctx, C.byref(st)), ctx)
    assert (plain == seq[2]).all()
    for a, b in zip(seq, outs):
        assert (a == b).all()
    # RGB-D frames in flight: each with its own out / out_aux, every other one over a background; after one sgs_frame_sync every
    # RGB and every depth / coverage buffer is the synchronous render's, bit for bit
    cfg_of = lambda i: pc.with_background(None, pc.BG) if i % 2 else None
    want = [drv.render_aux(c, cfg_of(i))[:2] for i, c in enumerate(cams)]
    bufs = [(np.full((80, 96, 3), pc.SENTINEL, np.float32), np.full((80, 96, 2), pc.SENTINEL, np.float32)) for _ in cams]
    for i, (c, (o, oa)) in enumerate(zip(cams, bufs)):
        drv.render_aux(c, cfg_of(i), out=o, out_aux=oa, flags=_capi.FLAG_ASYNC | _capi.FLAG_PIPELINED)
    drv.sync()
    for i, ((o, oa), (w_rgb, w_aux)) in enumerate(zip(bufs, want)):
        assert (o == w_rgb).all() and (oa == w_aux).all(), f"pipelined RGB-D frame {i} differs from the synchronous one"
    assert (want[1][0] != want[0][0]).any() and want[0][1].max() > 0.5
    # the batch entry point (always pipelined)
    arr = (_capi.SgsCamera * len(cams))(*[_capi.make_camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy,
                                                            np.asarray(c.view, np.float32).reshape(4, 4).tolist()) for c in cams])
    batch = np.zeros((len(cams), 80, 96, 3), np.float32)
    stats = (_capi.SgsStats * len(cams))()
    cfg2 = lib.default_config()
    lib.check(lib.sgs_render_batch(ctx, drv.scene, arr, len(cams), C.byref(cfg2), 0, -1, batch.ctypes.data, stats, None), ctx)
    for i in range(len(cams)):
        assert (batch[i] == seq[i]).all() and stats[i].d_total > 0
    # frames a stride apart, one band of tile rows each, stored at the top of a slab (what a rank of a sharded sweep does):
    # frame i's "pixel (0,0)" is slab i's start minus the rows above the band
    r0, r1, slab_rows = 1, 3, 48                                     # tile rows [1,3) = pixel rows 16..47 of the 80
    slabs = np.full((len(cams), slab_rows, 96, 3), -1.0, np.float32)
    base = slabs.ctypes.data - r0 * 16 * 96 * 3 * 4
    lib.check(lib.sgs_render_batch_strided(ctx, drv.scene, arr, len(cams), C.byref(cfg2), r0, r1, base, slab_rows * 96 * 3, None, None), ctx)
    for i in range(len(cams)):
        assert (slabs[i, :32] == seq[i][16:48]).all() and (slabs[i, 32:] == -1.0).all()


def test_batch_on_a_fresh_context_survives_overflowing_frames():
    """sgs_render_batch on a context whose record capacity is too small for EVERY frame (round-1 advisor finding): the
    redo of frame 0 took ring slots 0, 1, ... — the slots of the batch's later frames — and cleared their overflow
    flags before they were looked at, so frame 1 came back unrendered with frame 0's statistics.  Every frame's verdict
    is now read before anything is re-rendered."""
    import ctypes as C
    from sage_gs import _capi
    d = emu_harness.EmuRenderer(record_capacity=1024)
    try:
        scene = pc.random_scene(1200, 9, 0, scale=(0.1, 0.5))
        d.upload(*scene)
        d.set_record_capacity(1024)
        cams = []
        for k in range(5):
            V = np.eye(4, dtype=np.float32); V[0, 3] = 0.2 * k - 0.4
            cams.append(onp.Camera(96, 96, 80.0, 80.0, 48.0, 48.0, V))
        arr = (_capi.SgsCamera * len(cams))(*[_capi.make_camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy,
                                                                np.asarray(c.view, np.float32).reshape(4, 4).tolist()) for c in cams])
        batch = np.full((len(cams), 96, 96, 3), -1.0, np.float32)
        stats = (_capi.SgsStats * len(cams))()
        cfg = d.lib.default_config()
        d.lib.check(d.lib.sgs_render_batch(d.ctx, d.scene, arr, len(cams), C.byref(cfg), 0, -1, batch.ctypes.data, stats, None), d.ctx)
        for i, c in enumerate(cams):
            single, st = d.render(c, stats=False)
            assert st["d_total"] > 1024
            assert (batch[i] == single).all(), f"frame {i} of the batch differs from the frame rendered alone"
            assert stats[i].d_total == st["d_total"] and stats[i].n_visible == st["n_visible"]
    finally:
        d.close()


def test_more_frames_in_flight_than_the_status_ring_has_slots():
    d = emu_harness.EmuRenderer()
    try:
        pc.case_status_ring(d)
    finally:
        d.close()


def test_batch_statistics_of_frames_that_choose_different_tilings(drv):
    pc.case_batch_stats_of_mixed_tilings(drv)


@pytest.mark.parametrize("case", __import__("known_answer_cases").ALL, ids=lambda f: f.__name__)
def test_kernels_against_closed_form_answers(drv, case):
    """The analytic cases that pin the oracle, run straight against the kernels (emulator) — no oracle involved."""
    case(drv)
    with pc.forced_fine(drv):              # ... and through the fine tiles a frame this small may get (the library decides per frame)
        case(drv)


def test_argument_errors_are_reported_not_swallowed(drv):
    """The reference swallows render failures into `None` / black frames (simple_env.py:1390-1393); this ABI returns a
    negative status and a message for every bad argument, and leaves the context usable."""
    import ctypes as C
    from sage_gs import _capi
    scene, _ = onp.config1_scene(n=200, seed=1)
    drv.upload(*scene)
    lib, ctx = drv.lib, drv.ctx
    out = np.zeros((32, 32, 3), np.float32)
    good = _capi.make_camera(32, 32, 30.0, 30.0, 16.0, 16.0, np.eye(4, dtype=np.float32).tolist())

    def call(cam=good, cfg=None, r0=0, r1=-1, dst=out.ctypes.data, sc=None):
        return lib.sgs_render(ctx, drv.scene if sc is None else sc, C.byref(cam) if cam is not None else None,
                              C.byref(cfg) if cfg is not None else None, r0, r1, dst, None, None)

    def expect_invalid(rc, word):
        assert rc == -1, rc                                    # SGS_ERR_INVALID
        msg = lib.sgs_last_error(ctx).decode()
        assert word in msg, msg

    expect_invalid(call(dst=None), "null")
    expect_invalid(call(cam=None), "null")
    expect_invalid(call(cam=_capi.make_camera(0, 32, 30.0, 30.0, 16.0, 16.0, np.eye(4).tolist())), "resolution")
    expect_invalid(call(cam=_capi.make_camera(32, 32, 0.0, 30.0, 16.0, 16.0, np.eye(4).tolist())), "focal")
    expect_invalid(call(r0=2, r1=1), "tile_row_begin")
    bad = lib.default_config(); bad.sh_degree = 4
    expect_invalid(call(cfg=bad), "sh_degree")
    bad = lib.default_config(); bad.tile_row_stride, bad.tile_row_phase = 2, 2
    expect_invalid(call(cfg=bad), "tile_row_phase")
    bad.tile_row_phase = -1
    expect_invalid(call(cfg=bad), "tile_row_phase")
    # depth / coverage have no compact form (sage_gs.h): interleaved rows through sgs_render_rgbd are refused, nothing is written
    aux_buf = np.full((32, 32, 2), -7.0, np.float32); rgb_buf = np.full((32, 32, 3), -7.0, np.float32)
    for stride in (2, 3):
        bad = lib.default_config(); bad.tile_row_stride, bad.tile_row_phase = stride, 1
        expect_invalid(lib.sgs_render_rgbd(ctx, drv.scene, C.byref(good), C.byref(bad), 0, -1, rgb_buf.ctypes.data, aux_buf.ctypes.data, None, None), "out_aux")
        assert call(cfg=bad) == 0                              # (the same rows without out_aux: rendered)
    assert (aux_buf == -7.0).all() and (rgb_buf == -7.0).all()
    # what the kernels assume of the constants and of the view (round-1 advisor finding: near_z <= 0 breaks the depth-key order)
    for field, value, word in (("near_z", 0.0, "near_z"), ("near_z", -1.0, "near_z"), ("far_z", 0.1, "near_z"),
                               ("alpha_min", 0.0, "alpha_min"), ("alpha_min", float("nan"), "alpha_min"),
                               ("alpha_max", 1.0, "alpha_min"), ("t_min", 0.0, "t_min"), ("t_min", float("inf"), "t_min")):
        bad = lib.default_config(); setattr(bad, field, value)
        expect_invalid(call(cfg=bad), word)
    scaled = np.eye(4, dtype=np.float32); scaled[:3, :3] *= 2.0            # e.g. a USD xformOp:scale folded into the view
    expect_invalid(call(cam=_capi.make_camera(32, 32, 30.0, 30.0, 16.0, 16.0, scaled.tolist())), "rigid")
    assert lib.sgs_set_record_capacity(ctx, 0) == -1
    assert lib.sgs_debug_read(ctx, 999, None, 0) == -1
    # an unknown backend is refused at creation, with a message that needs no context
    h = C.c_void_p()
    assert lib.sgs_create(0, 7, C.byref(h)) == -5 and b"SGS_BACKEND_HIP" in lib.sgs_last_error(None)
    # the context still renders after all of that
    img, st = drv.render(onp.Camera(32, 32, 30.0, 30.0, 16.0, 16.0, np.eye(4, dtype=np.float32)))
    assert np.isfinite(img).all() and st["n_gaussians"] == 200


def test_compressed_upload_decodes_on_the_device_and_sorts_in_z_order(tmp_path):
    """sgs_scene_upload_compressed under the emulator: (1) the known-answer words of tests/golden/compressed_ply_kat.json come out of the
    layout kernel's dequantiser as the expected floats (SGS_BUF_SCENE_GEOM: the scene as the device holds it, by original index);
    (2) a quantised scene renders like the same scene decoded by NumPy and uploaded as fp32 arrays — per-splat records and frame to
    rounding — with the scene in Z-order made by the device radix sort (every Gaussian present exactly once)."""
    import os, sys
    sys.path.insert(0, os.path.dirname(__file__))
    from test_next_rows import _kat_payload, _check_kat
    from sage_gs import ply
    d = emu_harness.EmuRenderer(record_capacity=1 << 20)
    try:
        cases, chunks, packed, shb = _kat_payload()
        d.upload_compressed(chunks, packed, shb, 3, sh_decode="bin_centre")
        cam = onp.Camera(64, 48, 50.0, 50.0, 32.0, 24.0, np.eye(4, dtype=np.float32))
        d.render(cam)
        g = d.scene_geom()
        assert g.shape == (len(cases), 11)
        _check_kat(cases, g[:, 0:3], g[:, 4:7], g[:, 7:11], g[:, 3], None, None)
        # the SH bytes under all three readings, and where a byte of the channel-major file order lands in [coefficient][channel]
        for mode in ("bin_centre", "linear255", "bin_centre_ends"):
            d.upload_compressed(chunks, packed, shb, 3, sh_decode=mode)
            d.render(cam)
            shd = d.scene_sh()
            _check_kat(cases, None, None, None, None, None, shd[:, 1:, :], mode=mode)
        # a scene of a few chunks (so that the radix sort has several tiles... of one workgroup each), degree 3 and degree 0
        rng = np.random.default_rng(12)
        n = 5000
        means = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 7, n)], 1).astype(np.float32)
        scales = np.exp(rng.normal(-2.6, 0.5, (n, 3))).astype(np.float32)
        quats = rng.normal(size=(n, 4)); quats /= np.linalg.norm(quats, axis=1, keepdims=True)
        opac = rng.uniform(0.05, 1.0, n).astype(np.float32)
        sh = (rng.normal(size=(n, 16, 3)) * 0.3).astype(np.float32)
        cam = onp.Camera(160, 112, 120.0, 120.0, 80.0, 56.0, np.eye(4, dtype=np.float32))
        for deg in (3, 0):
            path = str(tmp_path / f"c{deg}.ply")
            ply.save_compressed_ply(path, means, scales, quats, opac, sh[:, :(deg + 1) ** 2], deg)
            arrays = ply.load_compressed_ply(path, sh_decode="bin_centre")
            d.upload(*arrays)
            ref, st_ref = d.render(cam)
            d.upload_compressed(*ply.read_compressed_payload(path), sh_decode="bin_centre")
            img, st = d.render(cam)
            g = d.scene_geom()
            assert np.allclose(g[:, 0:3], arrays[0], atol=1e-6) and np.allclose(g[:, 4:7], arrays[1], rtol=3e-6) and np.allclose(g[:, 3], arrays[3], atol=1e-7)
            assert np.allclose(g[:, 7:11], arrays[2], atol=2e-6)
            assert st["n_visible"] == st_ref["n_visible"] and abs(st["d_total"] - st_ref["d_total"]) <= 2      # (a rect edge may move with a 1e-6 scale change)
            assert np.abs(img - ref).max() < 2e-4 and ref.max() > 0.2
            # The compressed scene keeps its 8-bit SH as BYTES in HBM and k_preprocess dequantises per frame: the coefficients it evaluates
            # (SGS_BUF_SCENE_SH) are NumPy's decode exactly, and the frame equals — bit for bit — the frame of the SAME device-decoded arrays
            # uploaded as fp32 rows (the inflated layout of rounds 1-4).
            shd = d.scene_sh()
            assert shd.shape == arrays[4].shape and np.array_equal(shd[:, 1:], arrays[4][:, 1:]) and np.allclose(shd[:, 0], arrays[4][:, 0], atol=1e-6)
            d.upload(g[:, 0:3].copy(), g[:, 4:7].copy(), g[:, 7:11].copy(), g[:, 3].copy(), shd, deg)
            img32, st32 = d.render(cam)
            assert np.array_equal(img32, img) and st32["d_total"] == st["d_total"] and st32["n_visible"] == st["n_visible"]
            assert st["bytes"]["preprocess"] < st32["bytes"]["preprocess"] or deg == 0     # (algorithmic bytes: 4 rows of SH per visible Gaussian instead of 12)
            if deg == 3:
                # the other two readings of a coefficient byte (sage_gs.h SGS_SH_DECODE_*): what the kernel evaluates is ply.decode_sh_bytes' arithmetic
                # bit for bit (SGS_BUF_SCENE_SH restates it on the host; the frame is checked against the fp32 upload of those floats)
                payload = ply.read_compressed_payload(path)
                shb = payload[2]
                shb[:7, :] = 0; shb[7:13, :] = 255                                     # (the end codes, where the readings differ most)
                for mode in ("linear255", "bin_centre_ends"):
                    d.upload_compressed(payload[0], payload[1], shb, deg, sh_decode=mode)
                    img_m, _ = d.render(cam)
                    shm = d.scene_sh()
                    want = np.transpose(ply.decode_sh_bytes(shb, mode).reshape(n, 3, -1), (0, 2, 1))
                    assert np.array_equal(shm[:, 1:], want), mode
                    assert (shm[:7, 1:] == -4.0).all() and (shm[7:13, 1:] == 4.0).all()          # the end codes: -4 and +4 exactly
                    gm = d.scene_geom()
                    d.upload(gm[:, 0:3].copy(), gm[:, 4:7].copy(), gm[:, 7:11].copy(), gm[:, 3].copy(), shm, deg)
                    img_f, _ = d.render(cam)
                    assert np.array_equal(img_f, img_m), mode
                import ctypes as C
                from sage_gs import _capi
                bad = _capi.SgsCompressedScene(n, payload[0].shape[0], deg, 7, payload[0].ctypes.data, np.ascontiguousarray(payload[1], np.uint32).ctypes.data, shb.ctypes.data)
                h = C.c_void_p()
                assert d.lib.sgs_scene_upload_compressed(d.ctx, C.byref(bad), 0, C.byref(h)) == -1 and b"sh_decode" in d.lib.sgs_last_error(d.ctx)
                # ... and there is NO default: a scene with coefficient bytes and sh_decode = 0 (unspecified) is refused, with a message
                unset = _capi.SgsCompressedScene(n, payload[0].shape[0], deg, 0, payload[0].ctypes.data, np.ascontiguousarray(payload[1], np.uint32).ctypes.data, shb.ctypes.data)
                assert d.lib.sgs_scene_upload_compressed(d.ctx, C.byref(unset), 0, C.byref(h)) == -1 and b"sh_decode is required" in d.lib.sgs_last_error(d.ctx)
            else:
                d.upload_compressed(*ply.read_compressed_payload(path))                # degree 0: no coefficient bytes, nothing to specify
    finally:
        d.close()


def test_z_order_sort_of_a_scene_that_spans_several_scan_workgroups():
    """The upload's radix sort with more digit counters than one k_radix_scan workgroup scans (256 * ceil(n / 2048) > 4096): the laid-out
    scene, read back by ORIGINAL index, is the input — every Gaussian present exactly once, i.e. the sort produced a permutation — and
    the frame renders."""
    rng = np.random.default_rng(5)
    n = 40_000
    means = rng.uniform(-3, 3, (n, 3)).astype(np.float32) + np.array([0, 0, 6], np.float32)
    scales = np.full((n, 3), 0.01, np.float32)
    quats = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    opac = rng.uniform(0.2, 1.0, n).astype(np.float32)
    sh = rng.uniform(-1, 1, (n, 1, 3)).astype(np.float32)
    d = emu_harness.EmuRenderer(record_capacity=1 << 20)
    try:
        d.upload(means, scales, quats, opac, sh, 0)
        cam = onp.Camera(48, 32, 40.0, 40.0, 24.0, 16.0, np.eye(4, dtype=np.float32))
        img, st = d.render(cam)
        g = d.scene_geom()
        assert g.shape == (n, 11)
        assert np.array_equal(g[:, 0:3], means) and np.array_equal(g[:, 3], opac)
        assert st["n_gaussians"] == n and np.isfinite(img).all() and img.max() > 0.05
    finally:
        d.close()


def test_tuning_surface(drv):
    """sgs_tuning_default / sgs_set_tuning / sgs_get_tuning (include/sage_gs.h): values are validated (an error and a message, never a
    clamp), readable back, and a frame rendered under non-default values equals the default one (the emulator's streams are synchronous:
    the GPU suite holds pipelined frames and batches against each other)."""
    import ctypes as C
    from sage_gs import _capi
    lib, ctx = drv.lib, drv.ctx
    t = _capi.SgsTuning()
    lib.sgs_tuning_default(C.byref(t))
    assert (t.lanes, t.group, t.group_lanes, t.morton, t.record_capacity, t.fine_tile_pixels, t.fine_tile_growth) == (3, 8, 2, 1, 16 << 20, 640 * 480, 2.2)
    scene = pc.random_scene(900, 41, 1, scale=(0.05, 0.3))
    cam = onp.Camera(96, 64, 70.0, 70.0, 48.0, 32.0, np.eye(4, dtype=np.float32))
    drv.upload(*scene)
    FORCE = 1.0e9                                           # fine_tile_growth >= 16: fine tiles whenever the pixel rule allows
    with pc.forced_fine(drv):
        want, st0 = drv.render(cam, stats=False)
    want16, st16 = drv.render(cam, stats=False, fine=False)
    lib.check(lib.sgs_get_tuning(ctx, C.byref(t)), ctx)
    keep = (t.lanes, t.group, t.group_lanes, t.morton, t.record_capacity, t.fine_tile_pixels, t.fine_tile_growth)
    for bad in ((0, 4, 2), (17, 4, 2), (3, 9, 1), (3, 8, 3), (3, 0, 1)):
        u = _capi.SgsTuning(bad[0], bad[1], bad[2], 1, 1 << 20, 640 * 480, 2.2)
        assert lib.sgs_set_tuning(ctx, C.byref(u)) == -1 and b"sgs_tuning" in lib.sgs_last_error(ctx)
    u = _capi.SgsTuning(3, 4, 2, 1, 0, 640 * 480, 2.2)
    assert lib.sgs_set_tuning(ctx, C.byref(u)) == -1
    u = _capi.SgsTuning(3, 4, 2, 1, 1 << 20, -1, 2.2)
    assert lib.sgs_set_tuning(ctx, C.byref(u)) == -1 and b"fine_tile_pixels" in lib.sgs_last_error(ctx)
    for g_bad in (0.5, float("nan")):
        u = _capi.SgsTuning(3, 4, 2, 1, 1 << 20, 640 * 480, g_bad)
        assert lib.sgs_set_tuning(ctx, C.byref(u)) == -1 and b"fine_tile_growth" in lib.sgs_last_error(ctx)
    lib.check(lib.sgs_get_tuning(ctx, C.byref(t)), ctx)
    assert (t.lanes, t.group, t.group_lanes, t.morton, t.record_capacity, t.fine_tile_pixels, t.fine_tile_growth) == keep, "a refused tuning changed the context"
    u = _capi.SgsTuning(5, 2, 3, 0, 1 << 20, 640 * 480, FORCE)
    lib.check(lib.sgs_set_tuning(ctx, C.byref(u)), ctx)
    lib.check(lib.sgs_get_tuning(ctx, C.byref(t)), ctx)
    assert (t.lanes, t.group, t.group_lanes, t.morton, t.record_capacity, t.fine_tile_pixels, t.fine_tile_growth) == (5, 2, 3, 0, 1 << 20, 640 * 480, FORCE)
    drv.upload(*scene)                                   # (morton = 0: the caller's order is kept)
    got, st1 = drv.render(cam, stats=False)
    assert (got == want).all() and st1["n_visible"] == st0["n_visible"] and st1["d_total"] == st0["d_total"]
    # fine_tile_pixels / fine_tile_growth are the fields a frame depends on (to rounding): which tiles a frame of W x H pixels is rendered
    # through — with the growth rule out of the way (FORCE): 4x4-pixel tiles up to a quarter of fine_tile_pixels, 8x8 up to it, 16x16 above
    # (= SGS_FLAG_NO_FINE_TILES, bit for bit); the count of tiles says which
    tiles = lambda c: -(-96 // c) * -(-64 // c)
    assert st0["n_tiles"] == tiles(4) and st16["n_tiles"] == tiles(16)
    for fp, side in ((0, 16), (96 * 64 - 1, 16), (96 * 64, 8), (4 * 96 * 64 - 1, 8), (4 * 96 * 64, 4), (1 << 40, 4)):
        u = _capi.SgsTuning(5, 2, 3, 0, 1 << 20, fp, FORCE)
        lib.check(lib.sgs_set_tuning(ctx, C.byref(u)), ctx)
        img, st = drv.render(cam, stats=False)
        assert st["n_tiles"] == tiles(side), (fp, side, st["n_tiles"])
        assert st["n_visible"] == st0["n_visible"] and float(np.abs(img - want16).max()) < 1e-5        # (no pixel of this frame sits on a threshold)
        if side == 16:
            assert (img == want16).all() and st["d_total"] == st16["d_total"]
        if side == 4:
            assert (img == want).all() and st["d_total"] == st0["d_total"]
    u = _capi.SgsTuning(*keep)
    lib.check(lib.sgs_set_tuning(ctx, C.byref(u)), ctx)


def test_tiling_does_not_depend_on_the_scene_layout(drv):
    """sgs_tuning.morton must not change a frame (include/sage_gs.h): the probe that decides a small frame's tiling is drawn by original
    index.  The scenes that flipped while it was drawn through the layout (parity_cases.LAYOUT_FLIPS), and others across the threshold."""
    _, tilings = pc.case_tiling_does_not_depend_on_the_layout(drv, picks=(2, 8) + pc.LAYOUT_FLIPS + (22, 27))
    assert {t for w, t in tilings if w == 128} == {48, 192, 768}, tilings          # (16x16, 8x8 and 4x4 tiles all chosen somewhere)


def test_refused_record_capacity_changes_nothing(drv):
    pc.case_refused_capacity_changes_nothing(drv)


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
