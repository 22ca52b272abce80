"""Parity cases, written once and run twice: under the wave64 emulator on CPU (test_emu_parity.py,
kernel LOGIC) and on a real MI355X through the C ABI (test_gpu_parity.py, the parity tests proper).

A `drv` offers: upload(means, scales, quats, opac, sh, deg); render(cam, cfg=None, rows=(0,-1))
-> (image ndarray, stats dict); render_aux(cam, cfg=None, rows=(0,-1), fine=True, deep=True, stats=False, out=None, out_aux=None)
-> (image, aux [H, W, 2] = expected depth and coverage, stats dict); intermediates() -> (tile_offsets, sorted ids, slot ids, splat words).
Cameras/configs are oracle_np.Camera / oracle_np.Config objects.
"""
import dataclasses
import math
import time

import numpy as np

import oracle_c
import oracle_np as onp
from conftest import assert_frame_close
from tight_parity import assert_aux_tilings_agree, assert_depth_coverage_tight, assert_frame_tight


def random_scene(n, seed, deg=0, box=((-2, 2), (-2, 2), (2, 8)), scale=(0.02, 0.2), opac_mu=0.0):
    rng = np.random.default_rng(seed)
    means = np.stack([rng.uniform(*box[0], n), rng.uniform(*box[1], n), rng.uniform(*box[2], n)], 1)
    scales = np.exp(rng.uniform(math.log(scale[0]), math.log(scale[1]), (n, 3)))
    quats = rng.normal(size=(n, 4)) + 1e-3
    opac = 1.0 / (1.0 + np.exp(-rng.normal(opac_mu, 1.5, n)))
    k = (deg + 1) ** 2
    sh = 0.5 * rng.normal(size=(n, k, 3))
    if k > 1:
        sh[:, 1:] *= 0.3
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return f(means), f(scales), f(quats), f(opac), f(sh), deg


def look_at_view(eye, target, down=(0, 1, 0)):
    """A rigid model->camera matrix (+Z forward, +Y roughly `down`, +X right)."""
    eye, target, down = (np.asarray(v, float) for v in (eye, target, down))
    z = target - eye; z /= np.linalg.norm(z)
    x = np.cross(down, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    V = np.eye(4); V[:3, :3] = R; V[:3, 3] = -R @ eye
    return V.astype(np.float32)


class forced_fine:
    """with forced_fine(drv): frames small enough for fine tiles (sgs_tuning.fine_tile_pixels) ARE rendered through them, whatever the
    growth of their record count says (sgs_tuning.fine_tile_growth >= 16: the pixel rule alone) — the tests' way to the fine-tile path on
    scenes of large splats, which the library itself would render through 16x16-pixel tiles."""

    def __init__(self, drv):
        self.drv = drv

    def __enter__(self):
        self.keep = self.drv.tuning()["fine_tile_growth"]
        self.drv.set_tuning(fine_tile_growth=1.0e9)
        return self

    def __exit__(self, *exc):
        self.drv.set_tuning(fine_tile_growth=self.keep)
        return False


def check_against_oracle(drv, scene, cam, cfg=None, rows=(0, -1), what="", queues=True, upload=True, thorough=True):
    """Full comparison of one frame: counts and queues bit-exact, splat attributes to fp32 rounding,
    image within the parity tolerance.  upload=False: `scene` is already the driver's uploaded scene (several poses
    of a multi-million-Gaussian scene are checked against one upload).  thorough=False (a few long cases of the CPU emulator, whose point
    lies elsewhere): the renders that only hold one switch against another — SGS_FLAG_NO_DEEP, no chunk culling, reference binning with
    the lazy sort, and the same under fine tiles — are left to the other cases; everything held against the ORACLE stays."""
    if upload:
        drv.upload(*scene)
    # production path: tight bin rects, queues sorted lazily and only as far as the composite reads them — on 16x16-pixel tiles, the tiling
    # of the reference's integer structures and of the test hooks (a small frame's default, fine tiles, is checked at the end)
    img, st = drv.render(cam, cfg, rows, fine=False)
    # ... which counts D_f only on request (the drivers ask for it): the instantiation without the bookkeeping — the one
    # a sweep runs — must produce the same frame from the same queues
    img_plain, st_plain = drv.render(cam, cfg, rows, stats=False, fine=False)
    assert (img_plain == img).all() and st_plain["d_total"] == st["d_total"] and st_plain["n_visible"] == st["n_visible"] \
        and st_plain["d_fetched"] == 0, f"{what}: the frame depends on whether D_f is counted"
    # (the instantiation without D_f is also the only one that takes the deep-tile path: windows of a long-lived tile culled against its
    #  live pixels before anything is ranked — the comparison above holds the two paths against each other, bit for bit; and so does the
    #  runtime switch, SGS_FLAG_NO_DEEP, inside the one instantiation)
    if thorough:
        img_nodeep, st_nodeep = drv.render(cam, cfg, rows, stats=False, deep=False, fine=False)
        assert (img_nodeep == img).all() and st_nodeep["n_deep_windows"] == 0, f"{what}: the deep-tile cull changed a pixel"
    assert st["n_deep_windows"] == 0
    st["n_deep_windows_plain"] = st_plain["n_deep_windows"]
    # test hook: no chunk culling (every chunk of the scene projected).  The per-chunk bounds may only have skipped
    # chunks none of whose Gaussians is visible: same N_v, same queues, same frame.
    if thorough:
        drv.row_records(0, reset=True)
        img_all, st_all = drv.render(cam, cfg, rows, chunk_cull=False, fine=False)
        assert (img_all == img).all() and st_all["n_visible"] == st["n_visible"] and st_all["d_total"] == st["d_total"] \
            and st_all["d_fetched"] == st["d_fetched"], f"{what}: chunk culling changed the frame"
        # the per-row record counters (what cost-balanced bands are cut from) add up to D
        gy_ = (cam.height + 15) // 16
        rr = drv.row_records(gy_, reset=True)
        assert int(rr.sum()) == st_all["d_total"] and (rr[:rows[0]] == 0).all() and (rows[1] < 0 or (rr[rows[1]:] == 0).all())
    # test hook: order every queue completely (production binning)
    img_full, st_full = drv.render(cam, cfg, rows, full_sort=True)
    assert (img_full == img).all(), f"{what}: lazy and full sort must blend the same records in the same order"
    assert st_full["d_fetched"] == st["d_fetched"] and st_full["d_total"] == st["d_total"]
    # test hook: REFERENCE binning (S3's rect, what the oracle defines) + extent-only quadrant test.  The production
    # path may only have dropped records / (wave, splat) pairs that no pixel could use: frames bit-identical.
    img_loose, st_loose = drv.render(cam, cfg, rows, full_sort=True, loose_cull=True)
    assert (img_loose == img).all(), f"{what}: culling changed the frame"
    if thorough:
        img_ref_lazy, st_ref_lazy = drv.render(cam, cfg, rows, loose_cull=True)
        assert (img_ref_lazy == img).all(), f"{what}: culling changed the frame (lazy sort)"
        assert st_ref_lazy["d_fetched"] == st_loose["d_fetched"] and st_ref_lazy["d_total"] == st_loose["d_total"]
    assert st["d_total"] <= st_loose["d_total"] and st["d_fetched"] <= st_loose["d_fetched"]
    ref, aux = oracle_c.render(*scene, cam, cfg, rows[0], rows[1])
    assert st["n_visible"] == aux["n_visible"] == st_loose["n_visible"], (what, st["n_visible"], aux["n_visible"])
    assert st_loose["d_total"] == aux["D"], (what, st_loose["d_total"], aux["D"])
    off, ids, slot_ids, splats = drv.intermediates()
    assert (off == aux["offsets"]).all(), f"{what}: tile offsets differ"
    if queues:
        assert (ids == aux["ids"]).all(), f"{what}: per-tile queue order differs from (depth bits, index) order"
    # splat table, keyed by Gaussian index
    vis = np.nonzero(aux["tiles"] > 0)[0]
    assert (np.sort(slot_ids) == vis).all(), f"{what}: set of visible Gaussians differs"
    sp = splats[np.argsort(slot_ids)]
    f = sp.view(np.float32)
    assert (sp[:, 9] == aux["depth_bits"][vis]).all(), f"{what}: depth bits differ"
    r = aux["rect"][vis]
    assert ((sp[:, 10] & 0xffff) == r[:, 0]).all() and ((sp[:, 10] >> 16) == r[:, 1]).all() and \
           ((sp[:, 11] & 0xffff) == r[:, 2]).all() and ((sp[:, 11] >> 16) == r[:, 3]).all(), f"{what}: tile rects differ"
    # mean2D: the oracle's fp64 value rounded to fp32 — bit for bit, but for ONE fp32 ulp where the two fp64 evaluations (a reciprocal and a
    # product here, a division there) fall on either side of a rounding boundary (gpu_fuzz_trained seed 415: one of 155 k splats, r06zh)
    dxy = np.abs(f[:, 0:2] - aux["xy"][vis])
    assert (dxy <= np.maximum(1e-3 * 2 ** -10, np.spacing(np.abs(aux["xy"][vis])))).all(), f"{what}: mean2D {dxy.max():.2e}"
    # conic: 1e-5 relative, entry by entry — an entry below a millionth of the conic's largest (a numerical zero: the off-diagonal of an
    # isotropic Gaussian comes out as 1e-17 on both sides, gpu_fuzz_rooms seed 434) is held against that scale instead of against itself
    cref = aux["conic"][vis]
    rel = np.abs(np.stack([f[:, 2], f[:, 3], f[:, 4]], 1) - cref) / np.maximum(np.abs(cref), 1e-6 * np.abs(cref).max(axis=1, keepdims=True, initial=0) + 1e-30)
    assert rel.max(initial=0) < 1e-5, f"{what}: conic {rel.max():.2e}"
    assert (f[:, 5] == aux["opacity"][vis]).all(), f"{what}: opacity"
    rgb = np.stack([f[:, 6], f[:, 7], f[:, 8]], 1)
    assert np.abs(rgb - aux["rgb"][vis]).max(initial=0) < 2e-5, f"{what}: SH colour"
    # the band's pixel rows only (rows outside it are not rendered by either side)
    gy = (cam.height + 15) // 16
    ya, yb = 16 * rows[0], min(cam.height, 16 * (gy if rows[1] < 0 else rows[1]))
    worst = assert_frame_close(img[ya:yb], ref[ya:yb], aux["margin"][ya:yb], aux["recheck"], what=what, y0=ya)
    assert_frame_tight(img[ya:yb], ref[ya:yb], aux, y0=ya, what=what)
    if "d_fetched" in st_loose and st_loose["d_fetched"]:
        # D_f (reference binning) only differs from the oracle's where a pixel sat on the termination threshold
        assert abs(st_loose["d_fetched"] - aux["D_f"]) <= max(8, 2e-3 * aux["D_f"]), (what, st_loose["d_fetched"], aux["D_f"])
    # FINE TILES — the frame through tiles of 8x8 or 4x4 pixels (sgs_tuning.fine_tile_pixels; sgs_common.h), forced here for every frame small
    # enough (the library itself also asks that the split does not multiply the records by more than fine_tile_growth).  The same splats reach
    # every pixel (S3's rect stays a rect of 16x16-pixel tiles: N_v is the oracle's), the blend's coordinates are relative to another origin:
    # the oracle's frame within the same tolerance, every pixel, threshold-sensitive ones two-sidedly — and the instantiations / switches
    # that must not change a frame do not change this one either.
    with forced_fine(drv):
        img_f, st_f = drv.render(cam, cfg, rows)
        st["n_tiles_fine"] = st_f["n_tiles"]
        if st_f["n_tiles"] != st["n_tiles"]:
            assert st_f["n_visible"] == aux["n_visible"], (what, st_f["n_visible"], aux["n_visible"])
            img_fp, st_fp = drv.render(cam, cfg, rows, stats=False)
            assert (img_fp == img_f).all() and st_fp["d_total"] == st_f["d_total"], f"{what}: fine tiles: the frame depends on whether D_f is counted"
            if thorough:
                img_fn, _ = drv.render(cam, cfg, rows, stats=False, deep=False)
                img_fa, st_fa = drv.render(cam, cfg, rows, chunk_cull=False)
                assert (img_fn == img_f).all() and (img_fa == img_f).all() and st_fa["d_total"] == st_f["d_total"], f"{what}: fine tiles: a switch changed the frame"
            worst = max(worst, assert_frame_close(img_f[ya:yb], ref[ya:yb], aux["margin"][ya:yb], aux["recheck"], what=what + " [fine tiles]", y0=ya))
            assert_frame_tight(img_f[ya:yb], ref[ya:yb], aux, y0=ya, what=what + " [fine tiles]")
        else:
            assert (img_f == img).all(), f"{what}: SGS_FLAG_NO_FINE_TILES changed a frame that is not rendered through fine tiles"
    # ... and what the library does with this frame when nobody tells it: one of the tilings above (or the one between them), its own decision
    # (fine_shift_of: the pixel rule and the growth of the record count, estimated from the scene's probe) — the same frame, bit for bit
    img_d, st_d = drv.render(cam, cfg, rows)
    st["n_tiles_default"] = st_d["n_tiles"]
    if st_d["n_tiles"] == st["n_tiles"]:
        assert (img_d == img).all(), f"{what}: the default tiling is 16x16 and the frame is not the 16x16 frame"
    elif st_d["n_tiles"] == st_f["n_tiles"]:
        assert (img_d == img_f).all() and st_d["d_total"] == st_f["d_total"], f"{what}: the default tiling is the forced one and the frame is not"
    else:
        assert st["n_tiles"] < st_d["n_tiles"] < st_f["n_tiles"] and st_d["n_visible"] == aux["n_visible"]
        worst = max(worst, assert_frame_close(img_d[ya:yb], ref[ya:yb], aux["margin"][ya:yb], aux["recheck"], what=what + " [8x8-pixel tiles]", y0=ya))
        assert_frame_tight(img_d[ya:yb], ref[ya:yb], aux, y0=ya, what=what + " [8x8-pixel tiles]")
    return img, st, aux, worst


BG = (0.25, 0.5, 0.75)        # the background of the variant checks, unless a case says otherwise
SENTINEL = -7.0               # what band renders are pre-filled with: no pixel, depth or coverage is ever negative
MAX_SKIPPED = 0.05            # the share of a frame the depth / coverage budget may leave to the flat checks (pixels near a threshold)


def with_background(cfg, bg):
    """`cfg` (None: the defaults) with another background."""
    return dataclasses.replace(onp.Config() if cfg is None else cfg, background=tuple(float(v) for v in bg))


def _aux_against_oracle(aux, o, what):
    """The depth / coverage outputs against the oracle's frame `o` (black background or not: neither depends on it): the flat checks
    (1e-3 of the frame's largest depth, 1e-3 of coverage, off-threshold pixels) and tight_parity's budget, which may leave at most
    MAX_SKIPPED of the frame to the flat checks."""
    assert np.isfinite(aux).all(), f"{what}: non-finite depth / coverage"
    safe = o["margin"] >= 1e-4
    zmax = max(1.0, float(np.max(o["depth_image"], initial=0.0)))
    if safe.any():
        assert np.abs(aux[..., 0] - o["depth_image"])[safe].max() < 1e-3 * zmax, f"{what}: depth"
        assert np.abs(aux[..., 1] - (1.0 - o["final_T"]))[safe].max() < 1e-3, f"{what}: coverage"
    worst, skipped = assert_depth_coverage_tight(aux, o, what=what)
    assert skipped <= MAX_SKIPPED, f"{what}: {100 * skipped:.1f} % of the frame is near a threshold and skipped by the depth / coverage budget (at most {100 * MAX_SKIPPED:.0f} %)"
    return worst, skipped


def check_variants_against_oracle(drv, scene, cam, cfg=None, bg=BG, what="", fine=True, switches=True):
    """The instantiations of the composite that a black-background frame never runs — TF (cfg.bg != 0: the final transmittance of stopped
    pixels, 1 - sum of weights) and AUX (sgs_render_rgbd: expected depth and coverage, built for another occupancy) — on the scene ALREADY
    UPLOADED in `drv` (`scene`: its arrays, for the oracle), whose black-background frame the caller has held against the oracle.
    `cfg`: non-default thresholds (its own background is ignored: black and `bg` are rendered).  Per tiling — 16x16-pixel tiles, and, with
    fine=True and a frame small enough, the fine tiles forced —:
      1. img0, the black-background frame of the instantiation a sweep runs (no SGS_FLAG_STATS);
      2. AUX, black background: RGB == img0 bit for bit; depth and coverage against the oracle (flat checks and the budget; at most
         MAX_SKIPPED of the frame near a threshold); SGS_FLAG_NO_DEEP and SGS_FLAG_STATS change no bit of either; N_v and D are img0's;
      3. TF: the frame over `bg` against the oracle rendered with that background (assert_frame_close, assert_frame_tight);
         SGS_FLAG_NO_DEEP and SGS_FLAG_STATS change no bit;
      4. AUX over `bg`: RGB == 3 bit for bit, depth and coverage == 2 bit for bit (neither depends on the background).
    Between the tilings depth and coverage agree within the budget, not bit for bit (another tile origin, as for RGB): each is held to
    the oracle, so they are within twice the budget of each other — asserted on the pixels away from a threshold.
    switches=False (a few long emulator cases): the SGS_FLAG_NO_DEEP / SGS_FLAG_STATS renders of 2 and 3 are left out under fine tiles.
    Returns a dict: the stats of the AUX and TF renders on 16x16-pixel tiles (both without SGS_FLAG_STATS: the deep-tile path is theirs),
    the worst err / tol_px of the TF frames and of depth / coverage, the skipped share, the frames."""
    t0 = time.time()
    cfg0 = None if cfg is None else with_background(cfg, (0.0, 0.0, 0.0))
    cfg_bg = with_background(cfg, bg)
    _, o = oracle_c.render(*scene, cam, cfg0)
    ref_bg, o_bg = oracle_c.render(*scene, cam, cfg_bg, want="image")
    res = dict(worst_tf=0.0, worst_aux=0.0, skipped=0.0)
    aux_by_tiling = []

    def one_tiling(fine_flag, tag, sw):
        w = f"{what} [{tag}]"
        img0, st0 = drv.render(cam, cfg0, stats=False, fine=fine_flag)
        rgb_a, aux_a, st_a = drv.render_aux(cam, cfg0, fine=fine_flag)
        assert st_a["n_tiles"] == st0["n_tiles"]
        assert (rgb_a == img0).all(), f"{w}: the AUX instantiation changed the colours"
        assert st_a["n_visible"] == st0["n_visible"] == o["n_visible"] and st_a["d_total"] == st0["d_total"], (w, st_a, st0)
        wa, sk = _aux_against_oracle(aux_a, o, w + " AUX")
        img_bg, st_bg = drv.render(cam, cfg_bg, stats=False, fine=fine_flag)
        assert st_bg["n_visible"] == st0["n_visible"] and st_bg["d_total"] == st0["d_total"]
        assert_frame_close(img_bg, ref_bg, o_bg["margin"], o_bg["recheck"], what=w + " TF")
        wt = assert_frame_tight(img_bg, ref_bg, o_bg, what=w + " TF")
        if sw:
            for kw, name in ((dict(deep=False), "SGS_FLAG_NO_DEEP"), (dict(stats=True), "SGS_FLAG_STATS")):
                rgb_s, aux_s, st_s = drv.render_aux(cam, cfg0, fine=fine_flag, **kw)
                assert (rgb_s == img0).all() and (aux_s == aux_a).all(), f"{w}: {name} changed the AUX render"
                assert st_s["n_deep_windows"] == 0, (w, name, st_s["n_deep_windows"])
                img_s, st_s = drv.render(cam, cfg_bg, fine=fine_flag, **{"stats": False, **kw})
                assert (img_s == img_bg).all(), f"{w}: {name} changed the frame over a background"
                assert st_s["n_deep_windows"] == 0, (w, name, st_s["n_deep_windows"])
        rgb_ab, aux_ab, st_ab = drv.render_aux(cam, cfg_bg, fine=fine_flag)
        assert (rgb_ab == img_bg).all(), f"{w}: the AUX instantiation changed the colours over a background"
        assert (aux_ab == aux_a).all(), f"{w}: depth / coverage depend on the background"
        res["worst_tf"] = max(res["worst_tf"], wt); res["worst_aux"] = max(res["worst_aux"], wa); res["skipped"] = max(res["skipped"], sk)
        aux_by_tiling.append(aux_a)
        return dict(st_aux=st_a, st_tf=st_bg, st_aux_bg=st_ab, img0=img0, img_bg=img_bg, aux=aux_a)

    res.update(one_tiling(False, "16x16", True))
    res["n_tiles_fine"] = res["st_aux"]["n_tiles"]
    if fine:
        with forced_fine(drv):
            _, st_f = drv.render(cam, cfg0, stats=False)
            if st_f["n_tiles"] != res["st_aux"]["n_tiles"]:
                f = one_tiling(True, "fine tiles", switches)
                res["n_tiles_fine"] = f["st_aux"]["n_tiles"]
                assert res["n_tiles_fine"] == st_f["n_tiles"]
                res["fine"] = f
                # both tilings are within the budget of the oracle: twice the budget of each other, where no decision is near a threshold
                assert_aux_tilings_agree(aux_by_tiling[0], aux_by_tiling[1], o, what=what)
    o_bg["recheck"].close(); o["recheck"].close()
    res["seconds"] = time.time() - t0
    print(f"[variants] {what}: TF worst err/tol_px {res['worst_tf']:.3f}, depth/coverage {res['worst_aux']:.3f}, skipped {100 * res['skipped']:.2f} %, "
          f"{cam.width}x{cam.height}, tiles {res['st_aux']['n_tiles']} / {res['n_tiles_fine']}, deep windows AUX {res['st_aux']['n_deep_windows']} TF {res['st_tf']['n_deep_windows']}, "
          f"spill tiles AUX {res['st_aux']['n_spill_tiles']} TF {res['st_tf']['n_spill_tiles']}, {res['seconds']:.1f} s")
    return res


def check_aux_bands(drv, cam, cfg, cuts, what="", fine=True):
    """Bands of tile rows through sgs_render_rgbd: into RGB and aux buffers pre-filled with SENTINEL, the band [r0, r1) of 16-pixel rows
    writes its own rows only — bit for bit the rows of the whole-frame render — and leaves every other row of BOTH buffers alone; the
    bands of a partition (cuts: r0 < r1 < ... covering the frame) reassemble the frame.  16x16-pixel tiles and the fine tiles, forced
    (a 16-pixel row is then 2 or 4 rows of tiles)."""
    h, w = cam.height, cam.width
    gy = (h + 15) // 16
    assert cuts[0] == 0 and cuts[-1] == gy and all(a < b for a, b in zip(cuts[:-1], cuts[1:])), cuts
    with forced_fine(drv):
        for fine_flag in ((False, True) if fine else (False,)):
            full, full_aux, st_full = drv.render_aux(cam, cfg, fine=fine_flag)
            union = np.full_like(full, SENTINEL); union_aux = np.full_like(full_aux, SENTINEL)
            d_sum = 0
            for r0, r1 in zip(cuts[:-1], cuts[1:]):
                out = np.full((h, w, 3), SENTINEL, np.float32); out_aux = np.full((h, w, 2), SENTINEL, np.float32)
                img, aux, st = drv.render_aux(cam, cfg, rows=(r0, r1), fine=fine_flag, out=out, out_aux=out_aux)
                y0, y1 = 16 * r0, min(16 * r1, h)
                tag = f"{what}: rows [{r0}, {r1}) (fine {fine_flag})"
                assert (img[:y0] == SENTINEL).all() and (img[y1:] == SENTINEL).all(), f"{tag}: RGB rows outside the band were written"
                assert (aux[:y0] == SENTINEL).all() and (aux[y1:] == SENTINEL).all(), f"{tag}: aux rows outside the band were written"
                assert (img[y0:y1] == full[y0:y1]).all(), f"{tag}: the band's RGB differs from the whole frame's"
                assert (aux[y0:y1] == full_aux[y0:y1]).all(), f"{tag}: the band's depth / coverage differ from the whole frame's"
                union[y0:y1] = img[y0:y1]; union_aux[y0:y1] = aux[y0:y1]
                d_sum += st["d_total"]
            assert (union == full).all() and (union_aux == full_aux).all() and d_sum == st_full["d_total"], f"{what}: the bands do not reassemble the frame (fine {fine_flag})"


# ------------------------------------------------------------------------------------------------
def case_config1(drv, n=10_000):
    scene, cam = onp.config1_scene(n=n, seed=0)
    return check_against_oracle(drv, scene, cam, what=f"config1 n={n}")


def case_sh_degrees(drv, n=1500, thorough=True):
    for deg in (0, 1, 2, 3):
        scene = random_scene(n, 20 + deg, deg, box=((-3, 3), (-2, 2), (-3, 3)))
        view = look_at_view((4.0, 0.5, 5.0), (0.0, 0.0, 0.0))
        cam = onp.Camera(160, 128, 110.0, 105.0, 81.2, 60.7, view)
        check_against_oracle(drv, scene, cam, what=f"sh degree {deg}", thorough=thorough or deg == 3)
        if deg == 3:     # evaluate a degree-3 scene at lower degrees
            for d in (0, 2):
                check_against_oracle(drv, scene, cam, onp.Config(sh_degree=d), what=f"deg3 scene at degree {d}", thorough=thorough)


def case_ragged(drv):
    for n, (w, h) in ((1, (16, 16)), (63, (40, 24)), (65, (100, 70)), (129, (33, 17)), (1000, (250, 130))):
        scene = random_scene(n, 100 + n, 1, scale=(0.05, 0.4))
        cam = onp.Camera(w, h, 0.7 * w, 0.7 * w, w / 2.0, h / 2.0, np.eye(4, dtype=np.float32))
        check_against_oracle(drv, scene, cam, what=f"ragged n={n} {w}x{h}")


def fuzz_frame(seed, max_n=700, max_res=(260, 160), wild=False):
    """The scene, camera and non-default config of fuzz seed `seed` (case_fuzz's generator), and the generator's state for what a case
    draws next: (rng, scene, cam, cfg, n, w, h, deg)."""
    rng = np.random.default_rng(10_000 + seed)
    n = int(rng.integers(1, max_n))
    w, h = int(rng.integers(17, max_res[0])), int(rng.integers(17, max_res[1]))
    deg = int(rng.integers(0, 4))
    lo = float(10 ** rng.uniform(-2.7, -1.0)); hi = lo * float(10 ** rng.uniform(0.3, 2.0))
    if wild:                     # needles and pancakes up to the size of the scene, specks far below a pixel
        lo = float(10 ** rng.uniform(-4.0, -1.0)); hi = lo * float(10 ** rng.uniform(0.3, 4.0))
    scene = random_scene(n, 20_000 + seed, deg, box=((-3, 3), (-2, 2), (-1, 9)), scale=(lo, min(hi, 20.0 if wild else 3.0)),
                         opac_mu=float(rng.uniform(-3.0, 2.0)))
    if wild and seed % 3 == 0:   # opacities at both ends of (0, 1); a tenth of the cloud pushed far away (last depth buckets)
        scene[3][:] = np.clip(np.where(rng.random(n) < 0.5, 1.0 - 10 ** rng.uniform(-7, -2, n), 10 ** rng.uniform(-4, -1, n)), 1e-6, 1.0 - 1e-7).astype(np.float32)
        far = rng.random(n) < 0.1
        scene[0][far, 2] = (scene[0][far, 2] * float(10 ** rng.uniform(1, 3.5))).astype(np.float32)
        scene[1][far] *= np.float32(30.0)
    eye = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(-3, 6)])
    target = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 8)])
    if np.linalg.norm(target - eye) < 0.5:
        target = eye + np.array([0.1, 0.0, 1.0])
    down = np.array([rng.normal(0, 0.3), 1.0, rng.normal(0, 0.3)])
    view = look_at_view(eye, target, down)
    f = float(w * rng.uniform(0.12 if wild else 0.35, 1.6))
    cam = onp.Camera(w, h, f, f * float(rng.uniform(0.9, 1.1)), w / 2.0 + float(rng.uniform(-3, 3)),
                     h / 2.0 + float(rng.uniform(-3, 3)), view)
    cfg = onp.Config(near=float(rng.choice([0.2, 0.05, 0.5])), dilation=float(rng.choice([0.3, 0.1, 0.6])),
                     alpha_min=float(rng.choice([1.0 / 255.0, 0.01, 0.002])), alpha_max=float(rng.choice([0.99, 0.9])),
                     t_min=float(rng.choice([1.0e-4, 1.0e-3])), background=tuple(float(v) for v in rng.uniform(0, 1, 3)),
                     sh_degree=int(rng.integers(0, deg + 1)) if rng.random() < 0.3 else -1)
    return rng, scene, cam, cfg, n, w, h, deg


def case_fuzz(drv, seeds, max_n=700, max_res=(260, 160), wild=False, thorough_every=1):
    """Seeded random small frames through the full comparison: scene size, resolution (ragged tiles), SH degree, splat
    sizes from sub-pixel to screen-filling, opacities down to the cut-off, cameras inside and outside the cloud (Gaussians
    behind the camera, across the near plane, off screen), non-default thresholds / dilation / background, and a band of
    tile rows now and then."""
    for seed in seeds:
        rng, scene, cam, cfg, n, w, h, deg = fuzz_frame(seed, max_n, max_res, wild)
        gy = (h + 15) // 16
        rows = (0, -1)
        if gy >= 3 and rng.random() < 0.3:
            r0 = int(rng.integers(0, gy - 1)); rows = (r0, int(rng.integers(r0 + 1, gy + 1)))
        if seed % 4 == 0:            # default constants and the whole frame: also the depth / coverage outputs (f-4)
            cfg, rows = None, (0, -1)
        check_against_oracle(drv, scene, cam, cfg, rows, what=f"fuzz seed {seed} (n={n} {w}x{h} deg {deg} rows {rows})",
                             thorough=seed % thorough_every == 0)
        if seed % 5 == 1 and rows == (0, -1):      # interleaved tile-row shards reproduce the frame's rows bit for bit
            full, st_full = drv.render(cam, cfg)
            stride = int(rng.integers(2, 5))
            d_sum = 0
            for phase in range(min(stride, gy)):         # (a shard beyond the frame's rows owns nothing and is never rendered)
                part, st_p = drv.render(cam, cfg, interleave=(stride, phase))
                for k, row in enumerate(range(phase, gy, stride)):
                    y0, y1 = 16 * row, min(16 * row + 16, h)
                    assert (part[16 * k: 16 * k + (y1 - y0)] == full[y0:y1]).all(), f"fuzz seed {seed}: stride {stride} phase {phase} row {row}"
                d_sum += st_p["d_total"]
            assert d_sum == st_full["d_total"], f"fuzz seed {seed}: interleaved shards queue {d_sum} records, the frame {st_full['d_total']}"
        if seed % 4 == 0:
            rgb0, _ = drv.render(cam, stats=False)          # (the production instantiation)
            rgb, aux, _ = drv.render_aux(cam)
            assert (rgb == rgb0).all(), f"fuzz seed {seed}: the aux instantiation changed the colours"
            ref, o = oracle_c.render(*scene, cam)
            safe = o["margin"] >= 1e-4
            zmax = max(1.0, float(np.max(o["depth_image"])))
            if safe.any():
                assert np.abs(aux[..., 0] - o["depth_image"])[safe].max() < 1e-3 * zmax, f"fuzz seed {seed}: depth"
                assert np.abs(aux[..., 1] - (1.0 - o["final_T"]))[safe].max() < 1e-3, f"fuzz seed {seed}: coverage"
            assert_depth_coverage_tight(aux, o, what=f"fuzz seed {seed} aux")


def case_fuzz_variants(drv, seeds, max_n=700, max_res=(260, 160)):
    """case_fuzz's generator, seeds of its own, and on EVERY seed what case_fuzz draws now and then: the seed's non-default thresholds,
    dilation, near plane and SH degree, its random background, the depth / coverage outputs, and — wherever the frame has three tile
    rows — a partition into bands.  The black-background frame through check_against_oracle, the TF and AUX instantiations through
    check_variants_against_oracle, the bands through check_aux_bands.  (A driver whose render_aux drops `cfg` fails here on the first
    seed: the oracle is rendered with the seed's thresholds and background.)"""
    for seed in seeds:
        rng, scene, cam, cfg, n, w, h, deg = fuzz_frame(seed, max_n, max_res)
        what = f"fuzz variants seed {seed} (n={n} {w}x{h} deg {deg})"
        check_against_oracle(drv, scene, cam, with_background(cfg, (0.0, 0.0, 0.0)), what=what, thorough=False)
        check_variants_against_oracle(drv, scene, cam, cfg, bg=cfg.background, what=what)
        gy = (h + 15) // 16
        if gy >= 3:
            r0 = int(rng.integers(1, gy - 1)); r1 = int(rng.integers(r0 + 1, gy))
            check_aux_bands(drv, cam, cfg, [0, r0, r1, gy], what=what)


def case_non_finite_gaussians(drv, n=3000, res=(160, 120), seed=3):
    """NaN / +-inf in a Gaussian's mean, scale, rotation or opacity (or an all-zero quaternion): that Gaussian is never
    visible and the frame is, bit for bit, the frame of the scene without it — its chunk neighbours, the Z-order and the
    per-chunk bounds are unaffected."""
    rng = np.random.default_rng(seed)
    means, scales, quats, opac, sh, deg = random_scene(n, 900 + seed, 2, scale=(0.03, 0.4))
    hit = rng.random(n) < 0.05
    bm, bs, bq, bo = means.copy(), scales.copy(), quats.copy(), opac.copy()
    vals = [np.nan, np.inf, -np.inf]
    for i in np.nonzero(hit)[0]:
        f = int(rng.integers(0, 6)); v = vals[int(rng.integers(0, 3))]
        if f == 0: bm[i, int(rng.integers(0, 3))] = v
        elif f == 1: bs[i, int(rng.integers(0, 3))] = v
        elif f == 2: bq[i, int(rng.integers(0, 4))] = v
        elif f == 3: bq[i] = 0.0
        elif f == 4: bo[i] = np.nan
        else: bm[i] = v
    w, h = res
    cam = onp.Camera(w, h, 0.8 * w, 0.8 * w, w / 2.0, h / 2.0, np.eye(4, dtype=np.float32))
    keep = ~hit
    clean = (means[keep], scales[keep], quats[keep], opac[keep], sh[keep], deg)
    cfg_bg = with_background(None, BG)
    drv.upload(*clean)
    ref, st_ref = drv.render(cam)
    # ... and the depth / coverage outputs over a background (the TF and AUX instantiations): held to the oracle on the clean scene
    check_variants_against_oracle(drv, clean, cam, what=f"non-finite Gaussians removed (seed {seed})", switches=False)
    ref_bg, ref_aux, _ = drv.render_aux(cam, cfg_bg)
    drv.upload(bm, bs, bq, bo, sh, deg)
    img, st = drv.render(cam)
    assert np.isfinite(img).all() and (img == ref).all(), "a non-finite Gaussian changed the frame"
    assert st["d_total"] == st_ref["d_total"]
    img_bg, aux, _ = drv.render_aux(cam, cfg_bg)
    assert np.isfinite(img_bg).all() and np.isfinite(aux).all(), "a non-finite Gaussian made depth / coverage or the frame over a background non-finite"
    assert (img_bg == ref_bg).all() and (aux == ref_aux).all(), "a non-finite Gaussian changed depth / coverage or the frame over a background"


def case_padding_lanes(drv):
    """N not a multiple of 64 with a camera looking down -z: the padding lanes of the last chunk must stay
    culled (their placeholder mean projects to a huge POSITIVE depth for such a view)."""
    scene = random_scene(70, 77, 0, box=((-1, 1), (-1, 1), (-6, -2)), scale=(0.05, 0.3))
    view = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)        # rotate pi about y: looks down -z
    cam = onp.Camera(64, 64, 50.0, 50.0, 32.0, 32.0, view)
    img, st, aux, _ = check_against_oracle(drv, scene, cam, what="padding lanes")
    assert st["n_visible"] == aux["n_visible"] <= 70
    check_variants_against_oracle(drv, scene, cam, what="padding lanes")


def case_empty(drv):
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32),
             np.zeros((0,), np.float32), np.zeros((0, 1, 3), np.float32), 0)
    cam = onp.Camera(48, 32, 40.0, 40.0, 24.0, 16.0, np.eye(4, dtype=np.float32))
    drv.upload(*empty)
    img, st = drv.render(cam, onp.Config(background=(0.25, 0.5, 0.75)))
    assert st["n_visible"] == 0 and st["d_total"] == 0
    assert np.allclose(img, [0.25, 0.5, 0.75], atol=1e-7)

    def nothing_to_see(tag):
        """No splat reaches a pixel: T_final is exactly 1 (alpha_max T / alpha_max), so RGB is exactly the background and depth and
        coverage are exactly 0 — in the TF and in the AUX instantiation, on 16x16-pixel and on fine tiles, whole frame and band."""
        bg = np.asarray(BG, np.float32)
        with forced_fine(drv):
            for fine in (False, True):
                for kw in (dict(), dict(stats=True), dict(deep=False)):
                    img, st = drv.render(cam, with_background(None, BG), fine=fine, **kw)
                    assert st["n_visible"] == 0 and (img == bg).all(), f"{tag}: the frame over a background is not the background (fine {fine}, {kw})"
                    rgb, aux, st = drv.render_aux(cam, with_background(None, BG), fine=fine, **kw)
                    assert st["d_total"] == 0 and (rgb == bg).all() and (aux == 0.0).all(), f"{tag}: RGB-D of nothing (fine {fine}, {kw})"
                    rgb, aux, _ = drv.render_aux(cam, None, fine=fine, **kw)
                    assert (rgb == 0.0).all() and (aux == 0.0).all(), f"{tag}: RGB-D of nothing over black (fine {fine}, {kw})"
                out = np.full((cam.height, cam.width, 3), SENTINEL, np.float32); out_aux = np.full((cam.height, cam.width, 2), SENTINEL, np.float32)
                rgb, aux, _ = drv.render_aux(cam, with_background(None, BG), rows=(1, 2), fine=fine, out=out, out_aux=out_aux)
                assert (rgb[16:32] == bg).all() and (aux[16:32] == 0.0).all() and (rgb[:16] == SENTINEL).all() and (aux[:16] == SENTINEL).all() \
                    and (rgb[32:] == SENTINEL).all() and (aux[32:] == SENTINEL).all(), f"{tag}: a band of nothing (fine {fine})"
    nothing_to_see("empty scene")
    # everything culled (all behind the camera)
    scene = random_scene(300, 1, 0, box=((-1, 1), (-1, 1), (-8, -2)))
    drv.upload(*scene)
    img, st = drv.render(cam)
    assert st["n_visible"] == 0 and st["d_total"] == 0 and (img == 0).all()
    nothing_to_see("all culled")


def case_interleaved_rows(drv, stride, n=2500, res=(208, 150)):
    """Interleaved tile-row shards (rank p of `stride` owns frame rows p, p+stride, ...): every shard's compact image
    holds exactly those rows of the full frame, bit for bit, and the shards' queues add up to the frame's — on 16x16-pixel tiles and on
    the fine tiles a frame this small gets by default (a 16-pixel row is then 2 or 4 rows of tiles, owned or not as a whole)."""
    scene = random_scene(n, 7, 2, scale=(0.03, 0.3))
    w, h = res
    cam = onp.Camera(w, h, 0.8 * w, 0.8 * w, w / 2.0, h / 2.0, np.eye(4, dtype=np.float32))
    drv.upload(*scene)
    gy = (h + 15) // 16
    with forced_fine(drv):              # (switches nothing for the fine=False renders and the hooks: those are 16x16 by flag)
        for fine in (False, True):
            full, st_full = drv.render(cam, fine=fine)
            _, st_full_ref = drv.render(cam, loose_cull=True)
            assert (st_full["n_tiles"] != gy * ((w + 15) // 16)) == fine, "this frame is meant to be small enough for fine tiles"
            cp = next(c for c in (16, 8, 4) if -(-w // c) * -(-h // c) == st_full["n_tiles"])          # the tile's side in pixels
            d_sum = d_ref_sum = pix = 0
            seen = np.zeros(gy, bool)
            for phase in range(stride):
                img, st = drv.render(cam, interleave=(stride, phase), fine=fine)
                _, st_ref = drv.render(cam, interleave=(stride, phase), loose_cull=True)
                owned = list(range(phase, gy, stride))
                rows_of_tiles = sum(-(-(min(16 * row + 16, h) - 16 * row) // cp) for row in owned)
                assert img.shape[0] == 16 * len(owned) and st["n_tiles"] == rows_of_tiles * (-(-w // cp)), (st["n_tiles"], rows_of_tiles, cp)
                for k, row in enumerate(owned):
                    y0, y1 = 16 * row, min(16 * row + 16, h)
                    assert (img[16 * k: 16 * k + (y1 - y0)] == full[y0:y1]).all(), f"stride {stride} phase {phase}: frame row {row} (fine {fine})"
                    assert (img[16 * k + (y1 - y0): 16 * k + 16] == -1).all(), "pixels below the frame must stay untouched"
                    seen[row] = True
                    pix += (y1 - y0) * w
                d_sum += st["d_total"]; d_ref_sum += st_ref["d_total"]
                # a sub-range of the owned rows: only those are written
                if len(owned) >= 2:
                    part, st_p = drv.render(cam, rows=(1, 2), interleave=(stride, phase), fine=fine)
                    y0, y1 = 16 * owned[1], min(16 * owned[1] + 16, h)
                    assert (part[16: 16 + (y1 - y0)] == full[y0:y1]).all() and (part[:16] == -1).all() and (part[32:] == -1).all()
            assert seen.all() and pix == w * h
            assert d_sum == st_full["d_total"] and d_ref_sum == st_full_ref["d_total"]


def chunk_bounds_scene(n=6000, res=(208, 150)):
    """case_chunk_bounds' scene and camera: a wall 24 m x 12 m facing the camera at ~6 m (the view covers a tenth of it) and a cloud behind
    the camera, in random order."""
    means, scales, quats, opac, sh, deg = random_scene(n, 17, 1, box=((-12, 12), (-6, 6), (5.9, 6.1)), scale=(0.02, 0.12))
    rng = np.random.default_rng(18)
    back = rng.random(n) < 0.3
    means[back, 2] = rng.uniform(-10.0, -2.0, int(back.sum())).astype(np.float32)
    w, h = res
    view = look_at_view((0.3, -0.2, -1.0), (0.5, 0.4, 6.0))
    return (means, scales, quats, opac, sh, deg), onp.Camera(w, h, 0.9 * w, 0.9 * w, w / 2.0 + 3.3, h / 2.0 - 2.1, view)


def case_chunk_bounds(drv, n=6000, res=(208, 150)):
    """Per-chunk bounds (k_chunk_bounds / chunk_outside): a scene much wider than the view, so most 64-Gaussian chunks
    (Z-ordered at upload) lie outside the image or behind the camera.  The skipped chunks must hold no visible Gaussian
    — N_v, D, queues and frames equal the oracle's and the no-culling run's, for the full frame and for bands of tile
    rows (where chunks above and below the band are skipped too) — and a good share of the chunks must actually be
    skipped, or the test would prove nothing.  (That the bounds are TIGHT, and the order they are cut from, is upload_cases' matter.)"""
    scene, cam = chunk_bounds_scene(n, res)
    w, h = res
    gy = (h + 15) // 16
    n_chunks = (n + 63) // 64
    skipped = {}
    for rows in ((0, -1), (0, 2), (gy // 2, gy // 2 + 1), (gy - 2, gy)):
        check_against_oracle(drv, scene, cam, rows=rows, what=f"chunk bounds rows {rows}")
        drv.render(cam, None, rows)
        sk = drv.chunk_skipped()
        assert len(sk) == n_chunks
        skipped[rows] = int(sk.sum())
        drv.render(cam, None, rows, chunk_cull=False)
        assert int(drv.chunk_skipped().sum()) == 0
    assert skipped[(0, -1)] > 0.4 * n_chunks, skipped              # most of the scene is outside the view
    for rows in list(skipped)[1:]:
        assert skipped[rows] > skipped[(0, -1)], skipped            # a band skips what is above / below it as well


def case_tile_rows(drv, n=2500, res=(208, 150)):
    """Tile-row shards: each band equals the oracle's band; their union equals the full frame bit-exactly (16x16-pixel tiles and the fine
    tiles a frame this small gets by default)."""
    scene = random_scene(n, 7, 2, scale=(0.03, 0.3))
    w, h = res
    cam = onp.Camera(w, h, 0.8 * w, 0.8 * w, w / 2.0, h / 2.0, np.eye(4, dtype=np.float32))
    drv.upload(*scene)
    gy = (h + 15) // 16
    cuts = [0, gy // 3, gy // 3 + 1, gy]
    with forced_fine(drv):              # (switches nothing for the fine=False renders and the hooks: those are 16x16 by flag)
        for fine in (False, True):
            full, st_full = drv.render(cam, fine=fine)
            union = np.full_like(full, -1.0)
            d_sum = 0
            for r0, r1 in zip(cuts[:-1], cuts[1:]):
                out = np.full_like(full, -1.0)
                img, st = drv.render(cam, None, (r0, r1), out=out, fine=fine)
                y0, y1 = r0 * 16, min(r1 * 16, h)
                assert (img[:y0] == -1).all() and (img[y1:] == -1).all(), "rows outside the band must be untouched"
                ref, aux = oracle_c.render(*scene, cam, None, r0, r1)
                _, st_ref = drv.render(cam, None, (r0, r1), loose_cull=True)      # reference binning: the oracle's D
                assert st_ref["d_total"] == aux["D"] and st["n_visible"] == aux["n_visible"] and (fine or st["d_total"] <= aux["D"])
                assert_frame_close(img[y0:y1], ref[y0:y1], aux["margin"][y0:y1], aux["recheck"], what=f"tile rows [{r0}, {r1}) fine={fine}", y0=y0)
                assert_frame_tight(img[y0:y1], ref[y0:y1], aux, y0=y0, what=f"tile rows [{r0}, {r1}) fine={fine}")
                union[y0:y1] = img[y0:y1]
                d_sum += st["d_total"]
            assert (union == full).all(), f"union of tile-row bands != full frame (fine {fine})"
            assert d_sum == st_full["d_total"]


def case_depth_ties(drv):
    """Equal fp32 depths inside a tile must order by Gaussian index: short runs (in-place fix-up) and
    a run longer than SGS_TIE_RUN_MAX (the (index, depth) resort)."""
    rng = np.random.default_rng(5)
    n = 240
    means = np.zeros((n, 3), np.float32)
    means[:, 0] = rng.uniform(-0.15, 0.15, n); means[:, 1] = rng.uniform(-0.15, 0.15, n)
    depth = np.full(n, 3.0, np.float32)
    depth[:60] = 2.5                                   # one run of 60 (> 32) ...
    depth[60:120] = np.repeat(np.linspace(2.6, 2.9, 20, dtype=np.float32), 3)    # ... twenty runs of 3
    depth[120:] = np.linspace(3.0, 4.0, 120, dtype=np.float32)                   # ... and distinct keys
    means[:, 2] = depth
    perm = rng.permutation(n)
    means = means[perm]
    scales = np.full((n, 3), 0.05, np.float32)
    quats = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    opac = np.full(n, 0.05, np.float32)
    sh = rng.normal(size=(n, 1, 3)).astype(np.float32)
    cam = onp.Camera(64, 64, 64.0, 64.0, 32.0, 32.0, np.eye(4, dtype=np.float32))
    check_against_oracle(drv, (means, scales, quats, opac, sh, 0), cam, what="depth ties")
    check_variants_against_oracle(drv, (means, scales, quats, opac, sh, 0), cam, what="depth ties")


def case_sort_classes(drv, sizes=(700, 2500, 6000, 9500), variant_switches=True):
    """Queue lengths that land in each sort class: S (<=1024), M (<=4096), L (<=9216, all in LDS)
    and X (spill: ping-pong in HBM)."""
    for n in sizes:
        rng = np.random.default_rng(n)
        means = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(1.0, 30.0, n)], 1).astype(np.float32)
        scales = np.full((n, 3), 2.0, np.float32) * means[:, 2:3]          # every splat covers all four tiles
        quats = rng.normal(size=(n, 4)).astype(np.float32)
        opac = rng.uniform(0.005, 0.012, n).astype(np.float32)            # faint, but clear of the 1/255 cut-off
        sh = rng.normal(size=(n, 1, 3)).astype(np.float32)
        cam = onp.Camera(32, 32, 32.0, 32.0, 16.0, 16.0, np.eye(4, dtype=np.float32))
        img, st, aux, _ = check_against_oracle(drv, (means, scales, quats, opac, sh, 0), cam, what=f"sort class n={n}")
        assert st["max_tile_len"] == n
        v = check_variants_against_oracle(drv, (means, scales, quats, opac, sh, 0), cam, what=f"sort class n={n}", switches=variant_switches)
        assert v["st_aux"]["max_tile_len"] == n and v["st_tf"]["max_tile_len"] == n


def case_sparse_lists(drv, n=9000, res=(48, 40)):
    """Thousands of faint splats a pixel or two wide over a small image: no pixel saturates, every tile reads its whole queue in many batches,
    and every listed splat reaches a handful of a quadrant's 64 pixels — the shape of a low-resolution frame's slowest tiles (and the case the
    per-pixel-mask walk of round 6 was built for, profiles/r06n).  A second scene mixes in splats that cover whole quadrants and a few opaque
    ones (pixels that end in the middle of a list)."""
    w, h = res
    f = 40.0
    for seed, big in ((33, 0.0), (34, 0.05)):
        rng = np.random.default_rng(seed)
        z = rng.uniform(2.0, 30.0, n)
        means = np.stack([rng.uniform(-0.5 * w, 0.5 * w, n) * z / f, rng.uniform(-0.5 * h, 0.5 * h, n) * z / f, z], 1).astype(np.float32)
        s_px = np.where(rng.random(n) < big, rng.uniform(3.0, 12.0, n), rng.uniform(0.15, 0.7, n))          # sigma in pixels
        scales = (np.repeat((s_px * z / f)[:, None], 3, 1) * rng.uniform(0.6, 1.0, (n, 3))).astype(np.float32)
        quats = rng.normal(size=(n, 4)).astype(np.float32)
        opac = rng.uniform(0.02, 0.25, n).astype(np.float32)
        if big:
            opac[(rng.random(n) < 0.03) & (s_px < 1.0)] = 0.995                  # (a pixel here and there ends inside a chunk)
            opac[s_px >= 3.0] *= 0.2
        sh = rng.normal(size=(n, 1, 3)).astype(np.float32)
        cam = onp.Camera(w, h, f, f, w / 2.0, h / 2.0, np.eye(4, dtype=np.float32))
        img, st, aux, _ = check_against_oracle(drv, (means, scales, quats, opac, sh, 0), cam, what=f"sparse lists (seed {seed})")
        assert st["max_tile_len"] > 512, st["max_tile_len"]
        assert float((aux["final_T"] > 0.05).mean()) > 0.5 or big
        check_variants_against_oracle(drv, (means, scales, quats, opac, sh, 0), cam, what=f"sparse lists (seed {seed})")


def deep_tile_scene(n_back=6000):
    """(scene, camera) of case_deep_tile."""
    rng = np.random.default_rng(21)
    ys, xs = np.mgrid[0:32, 0:32]
    hole = ((xs % 16 >= 8) & (xs % 16 <= 12) & (ys % 16 >= 3) & (ys % 16 <= 7))
    px, py = xs[~hole].astype(np.float64), ys[~hole].astype(np.float64)
    f, c = 32.0, 16.0
    front = []
    for z in (1.0, 1.05, 1.1):
        front.append(np.stack([(px - c + 0.5) * z / f, (py - c + 0.5) * z / f, np.full(px.shape, z)], 1))
    nb = n_back
    zb = rng.uniform(2.0, 40.0, nb)
    back = np.stack([rng.uniform(-15.5, 15.5, nb) * zb / f, rng.uniform(-15.5, 15.5, nb) * zb / f, zb], 1)
    means = np.concatenate(front + [back]).astype(np.float32)
    nf = means.shape[0] - nb
    scales = np.concatenate([np.repeat((0.55 * means[:nf, 2] / f)[:, None], 3, 1),                # ~0.55 px: covers its own pixel
                             np.repeat((rng.uniform(0.6, 2.5, nb) * zb / f)[:, None], 3, 1)]).astype(np.float32)
    quats = rng.normal(size=(means.shape[0], 4)).astype(np.float32)
    opac = np.concatenate([np.full(nf, 0.999), rng.uniform(0.05, 0.6, nb)]).astype(np.float32)
    sh = rng.normal(size=(means.shape[0], 1, 3)).astype(np.float32)
    perm = rng.permutation(means.shape[0])
    scene = (means[perm], scales[perm], quats[perm], opac[perm], sh[perm], 0)
    return scene, onp.Camera(32, 32, f, f, c, c, np.eye(4, dtype=np.float32))


def case_deep_tile(drv, n_back=6000):
    """Tiles that keep consuming batches for a few pixels: three opaque layers saturate every pixel of a 32x32 image except a 5x5 hole
    per tile, and thousands of splats behind them are visible only through the holes.  After SGS_DEEP_AFTER batches such a tile culls every
    resident window of its queue against the live pixels BEFORE ranking / staging (k_tile_render, deep tiles) and blends the survivors as one
    batch: the frame must equal the oracle's AND the frame of the ordinary path (the D_f-counting instantiation) bit for bit — both
    checked by check_against_oracle — and the path must actually have run."""
    scene, cam = deep_tile_scene(n_back)
    img, st, aux, _ = check_against_oracle(drv, scene, cam, what="deep tile")
    assert st["max_tile_len"] > 1024 and st["n_deep_windows_plain"] >= 4, (st["max_tile_len"], st["n_deep_windows_plain"])
    # most pixels stopped inside the front layers, the holes read on deep into the queue
    stopped = float((aux["final_T"] < 1e-3).mean())
    assert stopped > 0.5 and st["d_fetched"] > 0.1 * st["d_total"], (stopped, st["d_fetched"], st["d_total"], st["n_deep_windows_plain"])
    # the same frame through the TF and AUX instantiations, which take the deep-tile path too (their renders without SGS_FLAG_STATS): the
    # windows culled against the live pixels must not lose or repeat a record's share of sum w (coverage, T_final bg) or of sum w z
    v = check_variants_against_oracle(drv, scene, cam, what="deep tile")
    assert v["st_aux"]["n_deep_windows"] >= 4 and v["st_tf"]["n_deep_windows"] >= 4 and v["st_aux_bg"]["n_deep_windows"] >= 4, \
        (v["st_aux"]["n_deep_windows"], v["st_tf"]["n_deep_windows"], v["st_aux_bg"]["n_deep_windows"])
    print(f"[deep tile] {st['n_deep_windows_plain']} windows culled first; {100 * stopped:.0f} % of the pixels stopped; D_f / D = {st['d_fetched'] / st['d_total']:.2f}")


def big_depth_bucket_scene(n_slab=3000):
    """(scene, camera) of case_big_depth_bucket."""
    rng = np.random.default_rng(8)
    n = n_slab + 500
    means = np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n), rng.uniform(1.0, 12.0, n)], 1).astype(np.float32)
    means[:n_slab, 2] = rng.uniform(3.0, 3.02, n_slab).astype(np.float32)
    means[100:100 + (4 * n_slab) // 5, 2] = 3.01               # four fifths of the slab at one depth (the tight bin rects drop some per tile)
    perm = rng.permutation(n); means = means[perm]
    scales = np.full((n, 3), 2.0, np.float32) * means[:, 2:3]      # broad: alpha stays clear of the 1/255 cut-off
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    opac = rng.uniform(0.005, 0.012, n).astype(np.float32)
    sh = rng.normal(size=(n, 1, 3)).astype(np.float32)
    return (means, scales, quats, opac, sh, 0), onp.Camera(32, 32, 32.0, 32.0, 16.0, 16.0, np.eye(4, dtype=np.float32))


def case_big_depth_bucket(drv, n_slab=3000):
    """Thousands of splats of one tile inside a 2-cm slab of a queue that spans 1-12 m (a wall facing the camera), four fifths
    of them at EXACTLY the same depth.  The composite cuts 256 depth buckets from the queue's own range (~3 cm each here), finds
    the slab's bucket longer than one batch and partitions the queue again over that bucket's key range (refinement) — which
    separates everything but the equal depths: that bucket exceeds the LDS capacity, cannot be refined and is sorted through
    HBM, its run of equal keys ordered by index."""
    scene, cam = big_depth_bucket_scene(n_slab)
    img, st, aux, _ = check_against_oracle(drv, scene, cam, what="big depth bucket")
    assert st["n_spill_tiles"] >= 1
    # the long-sum case of the TF / AUX instantiations: every pixel adds thousands of weights of ~0.01 T into 1 - T_final and sum w z
    # (each add rounds to half an ulp of a sum below 1: n 2^-25, inside B n of tight_parity's budget)
    v = check_variants_against_oracle(drv, scene, cam, what="big depth bucket")
    assert v["st_aux"]["n_spill_tiles"] >= 1 and v["st_tf"]["n_spill_tiles"] >= 1, (v["st_aux"]["n_spill_tiles"], v["st_tf"]["n_spill_tiles"])
    assert int(aux["n_contrib"].max()) > 700, int(aux["n_contrib"].max())      # (alpha <= 0.012: a pixel blends ln(1 / t_min) / 0.012 = 767 records before it may stop)


def case_full_grid_splat(drv, res=(1920, 1080), thorough=True, variants=False):
    """One huge splat covering every tile of a 1080p grid (120x68 = 8160 records from one lane) plus
    small ones: exercises the balanced duplication's row-major expansion over a wide rect."""
    w, h = res
    rng = np.random.default_rng(3)
    n = 40
    means = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.5, 0.5, n), rng.uniform(2, 4, n)], 1).astype(np.float32)
    scales = np.full((n, 3), 0.01, np.float32)
    means[17] = [0.0, 0.0, 1.0]; scales[17] = [4.0, 4.0, 0.5]
    quats = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    opac = np.full(n, 0.3, np.float32); opac[17] = 0.003             # below 1/255 everywhere: binned but never blended
    sh = rng.normal(size=(n, 1, 3)).astype(np.float32)
    cam = onp.Camera(w, h, 0.38 * w, 0.38 * w, w / 2.0, h / 2.0, np.eye(4, dtype=np.float32))
    img, st, aux, _ = check_against_oracle(drv, (means, scales, quats, opac, sh, 0), cam, what="full-grid splat", thorough=thorough)
    assert aux["tiles"][17] == ((w + 15) // 16) * ((h + 15) // 16)
    if variants:
        check_variants_against_oracle(drv, (means, scales, quats, opac, sh, 0), cam, what=f"full-grid splat {w}x{h}", switches=thorough)


def case_overflow_retry(drv):
    scene = random_scene(1200, 9, 0, scale=(0.1, 0.5))
    cam = onp.Camera(96, 96, 80.0, 80.0, 48.0, 48.0, np.eye(4, dtype=np.float32))
    drv.set_record_capacity(1024)
    img, st, aux, _ = check_against_oracle(drv, scene, cam, what="overflow -> grow -> retry")
    assert st["d_total"] > 1024 and st["retries"] >= 1
    # and once grown, no more retries
    img2, st2 = drv.render(cam, fine=False)
    assert st2["retries"] == 0 and (img2 == img).all()
    # the same entered through sgs_render_rgbd over a background: the frame that overflowed, grew the queues and was rendered again is
    # the frame (and the depth / coverage) of the context that never overflowed — which is held against the oracle
    cfg_bg = with_background(None, BG)
    got = {}
    with forced_fine(drv):
        for fine in (False, True):
            drv.set_record_capacity(1024)
            out = np.full((cam.height, cam.width, 3), SENTINEL, np.float32); out_aux = np.full((cam.height, cam.width, 2), SENTINEL, np.float32)
            rgb1, aux1, st1 = drv.render_aux(cam, cfg_bg, fine=fine, out=out, out_aux=out_aux)
            assert st1["d_total"] > 1024 and st1["retries"] >= 1, (fine, st1["d_total"], st1["retries"])
            rgb2, aux2, st2 = drv.render_aux(cam, cfg_bg, fine=fine)
            assert st2["retries"] == 0 and (rgb2 == rgb1).all() and (aux2 == aux1).all(), f"the retried RGB-D frame differs from the un-overflowed one (fine {fine})"
            got[fine] = (rgb1, aux1)
    v = check_variants_against_oracle(drv, scene, cam, what="overflow -> grow -> retry")
    assert (got[False][0] == v["img_bg"]).all() and (got[False][1] == v["aux"]).all()
    assert (got[True][0] == v["fine"]["img_bg"]).all() and (got[True][1] == v["fine"]["aux"]).all()


def case_depth_aux(drv, n=1500, res=(96, 80)):
    """f-4: expected view depth sum(T alpha z) and coverage 1 - T_final, against the oracle; the RGB of the
    aux kernel instantiation must equal the RGB-only kernel's bit for bit."""
    scene = random_scene(n, 55, 1, scale=(0.03, 0.3))
    w, h = res
    cam = onp.Camera(w, h, 0.8 * w, 0.8 * w, w / 2.0, h / 2.0, np.eye(4, dtype=np.float32))
    drv.upload(*scene)
    rgb0, _ = drv.render(cam, stats=False)
    rgb, aux, _ = drv.render_aux(cam)
    assert (rgb == rgb0).all()
    ref, o = oracle_c.render(*scene, cam)
    safe = o["margin"] >= 1e-4
    zmax = float(np.max(scene[0][:, 2]))
    assert np.abs(aux[..., 0] - o["depth_image"])[safe].max() < 1e-3 * zmax
    assert np.abs(aux[..., 1] - (1.0 - o["final_T"]))[safe].max() < 1e-3
    assert np.abs(aux[..., 0] - o["depth_image"]).max() < zmax / 255.0 + 1e-3 * zmax
    assert_depth_coverage_tight(aux, o, what="depth aux")


def case_determinism(drv, n=4000):
    scene = random_scene(n, 31, 1, scale=(0.03, 0.3))
    cam = onp.Camera(176, 144, 120.0, 120.0, 88.0, 72.0, np.eye(4, dtype=np.float32))
    drv.upload(*scene)
    a, st = drv.render(cam, full_sort=True)
    ids_a = drv.intermediates()[1].copy()
    b, _ = drv.render(cam, full_sort=True)
    ids_b = drv.intermediates()[1]
    c, _ = drv.render(cam, fine=False)
    assert (c == a).all()
    p1, _ = drv.render(cam, stats=False, fine=False); p2, _ = drv.render(cam, stats=False, fine=False)      # the production instantiation twice
    assert (p1 == p2).all() and (p1 == a).all(), "two production renders of the same frame differ"
    assert (a == b).all() and (ids_a == ids_b).all(), "two renders of the same frame differ"
    with forced_fine(drv):
        f1, st1 = drv.render(cam, stats=False); f2, st2 = drv.render(cam, stats=False)  # ... and through fine tiles
    assert st1["n_tiles"] > st["n_tiles"] and (f1 == f2).all() and st1 == st2, "two fine-tile renders of the same frame differ"
    assert float(np.mean(np.abs(f1 - a).max(axis=-1) > 1e-5)) < 2e-3 and float(np.median(np.abs(f1 - a))) < 1e-6, "fine tiles moved the frame by more than rounding"
    d1, sd1 = drv.render(cam, stats=False); d2, sd2 = drv.render(cam, stats=False)      # ... and as the library decides by itself
    assert (d1 == d2).all() and sd1 == sd2 and ((d1 == f1).all() or (d1 == a).all() or sd1["n_tiles"] not in (st["n_tiles"], st1["n_tiles"]))


def case_batch_shares_scene_reads(drv, n=4000, res=(160, 112), quick=False):
    """sgs_render_batch*: the full frames of a group are projected by ONE launch whose waves take the group's work list — (chunk, frame)
    pairs, chunk-major (k_chunk_cull_group / k_preprocess_shared: the frames that want a chunk run side by side, the group reads the scene
    once).  That must not show: every frame of a batch equals the frame rendered alone, bit for bit — for nearly identical views (every
    chunk wanted by all frames), for views turned a quarter circle apart (hardly a chunk wanted twice), for a batch that mixes them
    (groups of four: the kinds alternate), with fine tiles and without."""
    scene = random_scene(n, 77, 2, box=((-4, 4), (-2, 2), (-4, 4)), scale=(0.02, 0.2))
    drv.upload(*scene)
    w, h = res

    def cam_at(yaw_deg, dx=0.0):
        a = np.deg2rad(yaw_deg)
        eye = (0.3 + dx, 0.1, 0.2)
        return onp.Camera(w, h, 0.7 * w, 0.7 * w, w / 2.0, h / 2.0, look_at_view(eye, (eye[0] + np.sin(a), eye[1], eye[2] + np.cos(a))))
    near = [cam_at(10.0 + 2.0 * k, 0.02 * k) for k in range(6)]                  # consecutive frames of a path
    far = [cam_at(90.0 * k) for k in range(4)] + [cam_at(45.0), cam_at(225.0)]   # views that share next to nothing
    mixed = near[:4] + far[:4] + near[4:] + far[4:]
    for cams in ((mixed,) if quick else (near, far, mixed)):       # (quick — the CPU emulator: the mixed batch holds both kinds of group)
        for fine in (False, True):
            with forced_fine(drv):
                alone = [drv.render(c, stats=False, fine=fine)[0] for c in cams]
                batch = drv.render_batch(cams, fine=fine)
            for i, a in enumerate(alone):
                assert (batch[i] == a).all(), f"frame {i} of a batch of {len(cams)} differs from the frame rendered alone (fine {fine})"
            if cams is mixed:        # ... and over a background: the batch launches the TF instantiation with one frame per blockIdx.y
                cfg_bg = with_background(None, BG)
                with forced_fine(drv):
                    alone_bg = [drv.render(c, cfg_bg, stats=False, fine=fine)[0] for c in cams]
                    batch_bg = drv.render_batch(cams, fine=fine, cfg=cfg_bg)
                for i, a in enumerate(alone_bg):
                    assert (batch_bg[i] == a).all(), f"frame {i} of a batch over a background differs from the frame rendered alone (fine {fine})"
                assert any((a != b).any() for a, b in zip(alone_bg, alone)), "the background shows in no frame"
    assert any(a.max() > 0.05 for a in alone)


def case_fine_tile_decision(drv, n=500):
    """fine_shift_of (sgs_api.hip): a frame small enough for fine tiles is split while halving the tiles multiplies its (Gaussian, tile)
    records by no more than sgs_tuning.fine_tile_growth — a ratio the library ESTIMATES on the host from the scene's probe (here the
    whole scene: fewer Gaussians than a probe holds).  Scenes of splats from far below a tile to several tiles wide, at two resolutions:
    the decision must agree with the frame's REAL record counts wherever those are clear of the threshold, the frame must be the frame of
    the tiling it chose (bit for bit), a batch and a band must make the same choice as the single frame."""
    g = drv.tuning()["fine_tile_growth"]
    assert g == 2.2
    seen = set()
    for seed, scale in ((1, (0.004, 0.02)), (2, (0.01, 0.05)), (3, (0.03, 0.15)), (4, (0.1, 0.5)), (5, (0.3, 1.2))):
        scene = random_scene(n, 300 + seed, 1, scale=scale, opac_mu=1.0)
        drv.upload(*scene)
        for (w, h) in ((96, 64), (200, 152)):
            cam = onp.Camera(w, h, 0.9 * w, 0.9 * w, w / 2.0, h / 2.0, np.eye(4, dtype=np.float32))
            tiles = lambda c: -(-w // c) * -(-h // c)
            # the three tilings, each forced (the pixel rule alone: fine_tile_pixels = 0 / W H / 4 W H under a growth limit that never binds)
            keep = drv.tuning()
            D, img = {}, {}
            for side, fp in ((16, 0), (8, w * h), (4, 4 * w * h)):
                drv.set_tuning(fine_tile_pixels=fp, fine_tile_growth=1.0e9)
                img[side], st = drv.render(cam, stats=False)
                assert st["n_tiles"] == tiles(side)
                D[side] = st["d_total"]
            drv.set_tuning(fine_tile_pixels=4 * w * h, fine_tile_growth=keep["fine_tile_growth"])     # (both splits allowed by the pixel rule)
            got, st = drv.render(cam, stats=False)
            side = next(c for c in (16, 8, 4) if tiles(c) == st["n_tiles"])
            assert (got == img[side]).all() and st["d_total"] == D[side], f"seed {seed} {w}x{h}: the frame is not the frame of the tiling it chose"
            g1, g2 = D[8] / max(1, D[16]), D[4] / max(1, D[8])
            want = 16 if g1 > g else 8 if g2 > g else 4
            clear = abs(g1 - g) > 0.12 * g and (g1 > g or abs(g2 - g) > 0.12 * g)        # (the estimate bins extents, not the exact rects: a few per cent)
            assert side == want or not clear, f"seed {seed} {w}x{h}: records grow by {g1:.2f}, {g2:.2f} per split, the library chose {side}x{side}"
            seen.add(side)
            gy = (h + 15) // 16
            band, st_b = drv.render(cam, rows=(1, gy - 1), stats=False, out=np.full((h, w, 3), -1.0, np.float32))
            assert (band[16:16 * (gy - 1)] == got[16:16 * (gy - 1)]).all(), f"seed {seed} {w}x{h}: a band chose another tiling than its frame"
            drv.set_tuning(fine_tile_pixels=keep["fine_tile_pixels"], fine_tile_growth=keep["fine_tile_growth"])
    assert seen == {16, 8, 4}, seen          # (the five scenes span the three outcomes)


# Scenes whose splats straddle sgs_tuning.fine_tile_growth at small resolutions: random_scene(n, 700 + i, 0, scale=(s / 2, 2 s),
# opac_mu=1.0) for s = LAYOUT_SCALES[i], seen by an identity camera with f = 0.9 w.  While the probe was drawn at even strides through the
# LAYOUT, four of them (i = 12, 15, 17, 19) got another tiling — and another frame — with morton = 0 than with morton = 1 (4000 Gaussians:
# 1900 against 475 tiles at 200x152, 192 against 768 / 48 against 192 / 130 against 475 at 128x96 and 200x152).
LAYOUT_SCALES = np.geomspace(0.004, 0.3, 28)
LAYOUT_FLIPS = (12, 15, 17, 19)


def layout_scene(i, n=4000):
    s = float(LAYOUT_SCALES[i])
    return random_scene(n, 700 + i, 0, scale=(s / 2, 2 * s), opac_mu=1.0)


def layout_cameras(res=((128, 96), (200, 152))):
    return [onp.Camera(w, h, 0.9 * w, 0.9 * w, w / 2.0, h / 2.0, np.eye(4, dtype=np.float32)) for w, h in res]


def frames_of(drv, cams):
    """The frames of `cams` on the driver's scene as the library renders them by itself (its own tiling), with (n_tiles, n_visible, d_total)."""
    out = []
    for cam in cams:
        img, st = drv.render(cam, stats=False)
        out.append((img, (st["n_tiles"], st["n_visible"], st["d_total"])))
    return out


def case_tiling_does_not_depend_on_the_layout(drv, picks=range(28), n=4000, cams=None):
    """The tiling a small frame gets (fine_shift_of) is estimated from the scene's probe of 512 Gaussians; the probe is drawn by the Gaussians'
    indices in the caller's order, so the layout of the scene on the device — Z-order (sgs_tuning.morton = 1) or the caller's order
    (morton = 0) — must not change the tiling, nor, therefore, a pixel: same n_tiles / N_v / D, frames bit for bit.  The scales sweep across
    the growth threshold (every tiling is chosen somewhere) and take in the scenes that flipped with the layout (LAYOUT_FLIPS).
    Returns the frames (morton = 1) by scene for further comparisons (the GPU's compressed upload)."""
    cams = layout_cameras() if cams is None else cams
    keep = drv.tuning()["morton"]
    tilings, frames = set(), {}
    try:
        for i in picks:
            scene = layout_scene(i, n)
            got = {}
            for morton in (1, 0):
                drv.set_tuning(morton=morton)
                drv.upload(*scene)
                got[morton] = frames_of(drv, cams)
            for cam, (a, sa), (b, sb) in zip(cams, got[1], got[0]):
                what = f"scene {i} (seed {700 + i}, s {LAYOUT_SCALES[i]:.4f}, n {n}) at {cam.width}x{cam.height}"
                assert sa == sb, f"{what}: (n_tiles, N_v, D) {sa} with the scene in Z-order, {sb} in the caller's order"
                assert (a == b).all(), f"{what}: the frame depends on the scene's layout"
                tilings.add((cam.width, sa[0]))
            frames[i] = got[1]
    finally:
        drv.set_tuning(morton=keep)
    return frames, tilings


def case_refused_capacity_changes_nothing(drv):
    """A record capacity the library refuses (2^33: more than its 32-bit tile offsets can address; validation refuses it, nothing is allocated)
    must leave the context as it was: the tuning reads back unchanged and the next frame renders, the same frame as before.  The same for
    sgs_set_tuning carrying that capacity: SGS_ERR_INVALID, and none of its other fields applied either."""
    from sage_gs import _capi
    scene = random_scene(900, 43, 1, scale=(0.05, 0.3))
    cam = onp.Camera(96, 64, 70.0, 70.0, 48.0, 32.0, np.eye(4, dtype=np.float32))
    drv.upload(*scene)
    want, st0 = drv.render(cam, stats=False)
    keep = drv.tuning()
    assert keep["lanes"] != 5 and keep["morton"] == 1
    for what, attempt in (("sgs_set_record_capacity", lambda: drv.set_record_capacity(1 << 33)),
                          ("sgs_set_tuning", lambda: drv.set_tuning(lanes=5, group=2, group_lanes=3, morton=0, record_capacity=1 << 33))):
        try:
            attempt()
        except _capi.SgsError as e:
            assert e.code == -1 and "2^32" in str(e), (what, e.code, str(e))        # SGS_ERR_INVALID
        else:
            raise AssertionError(f"{what}: a record capacity of 2^33 was accepted")
        assert drv.tuning() == keep, (what, drv.tuning(), keep)
        got, st = drv.render(cam, stats=False)
        assert (got == want).all() and (st["n_visible"], st["d_total"]) == (st0["n_visible"], st0["d_total"]), f"{what}: the next frame differs"
    # ... and once more: still refused (a refused value that had been stored would now compare as "unchanged")
    try:
        drv.set_tuning(lanes=5, group=2, group_lanes=3, morton=0, record_capacity=1 << 33)
    except _capi.SgsError as e:
        assert e.code == -1                                  # SGS_ERR_INVALID
    else:
        raise AssertionError("sgs_set_tuning: a record capacity of 2^33 was accepted the second time")
    assert drv.tuning() == keep
    # the capacity the context already holds (unchanged, no reallocation) with the other fields: applied
    drv.set_tuning(lanes=5, group=2, group_lanes=3, morton=0)
    t = drv.tuning()
    assert (t["lanes"], t["group"], t["group_lanes"], t["morton"], t["record_capacity"]) == (5, 2, 3, 0, keep["record_capacity"]), t
    got, st = drv.render(cam, stats=False)
    assert (got == want).all()
    drv.set_tuning(**{k: keep[k] for k in ("lanes", "group", "group_lanes", "morton")})
    assert drv.tuning() == keep


def stats_without_times(st):
    """What a frame's sgs_stats says of the FRAME: every field but the stage times and the number of renders it took."""
    return {k: v for k, v in st.items() if k not in ("ms", "ms_total", "retries")}


RING_SHIFTS = (-0.35, -0.1, 0.1, 0.15)
RING_FRAMES = 260            # more frames than the status ring has slots (256): a batch of them is two chunks, the second of 4 frames


def ring_scene_and_cameras():
    """32x32 frames (four tiles) of 300 Gaussians from four cameras a step apart: D = 1 000 ... 1 035 per frame, on both sides of 1024."""
    cams = []
    for k in range(4):
        V = np.eye(4, dtype=np.float32); V[0, 3] = RING_SHIFTS[k]
        cams.append(onp.Camera(32, 32, 28.0, 28.0, 16.0, 16.0, V))
    return random_scene(300, 9, 0, scale=(0.1, 0.4)), cams


def case_status_ring(drv):
    """The host's bookkeeping of the frames in flight (sgs_api.hip StatusRing, FrameRec), at frames so small that nothing else is tested.
    A `drv` offers frames_in_flight(cams) -> the frames of SGS_FLAG_ASYNC | SGS_FLAG_PIPELINED renders, each into its own buffer, with
    nothing but ONE sgs_frame_sync after the last; and render_batch_stats(cams) -> (frames, one stats dict per frame).
    (a) 260 frames in flight — the ring wraps, the library has to drain it by itself: every buffer is the synchronous frame of its camera.
    (b) one batch of 260 cameras under a record capacity of 1024, which some frames overflow and some do not: every frame is the frame
        rendered alone, and its N_v, D and tile count are the single render's."""
    scene, cams = ring_scene_and_cameras()
    drv.upload(*scene)
    alone = [drv.render(c, stats=False) for c in cams]
    d = [st["d_total"] for _, st in alone]
    assert max(d) > 1024 and min(d) <= 1024, d           # (the case's own precondition: both verdicts occur in the batch)
    many = [cams[i % 4] for i in range(RING_FRAMES)]
    for i, img in enumerate(drv.frames_in_flight(many)):
        assert (img == alone[i % 4][0]).all(), f"frame {i} of {RING_FRAMES} in flight differs from the synchronous frame"
    drv.set_record_capacity(1024)
    batch, stats = drv.render_batch_stats(many)
    for i in range(RING_FRAMES):
        img, st = alone[i % 4]
        assert (batch[i] == img).all(), f"frame {i} of a batch of {RING_FRAMES} differs from the frame rendered alone"
        got = {k: stats[i][k] for k in ("n_visible", "d_total", "n_tiles")}
        assert got == {k: st[k] for k in got}, (i, got, st)


def case_batch_stats_of_mixed_tilings(drv, n=500, res=(96, 64)):
    """A batch whose frames choose different tilings (a lens that zooms in and out: fine_shift_of decides per camera, a launch group ends
    where the choice changes): every frame is the frame rendered alone and its sgs_stats — bytes[] too, which count the frame's OWN grid
    of tiles — are the single render's, the stage times and `retries` aside."""
    scene = random_scene(n, 303, 1, scale=(0.03, 0.15), opac_mu=1.0)
    drv.upload(*scene)
    w, h = res
    cams = [onp.Camera(w, h, k * w, k * w, w / 2.0, h / 2.0, np.eye(4, dtype=np.float32)) for k in (0.9, 0.2, 3.0, 0.25, 0.9, 4.0, 0.3, 0.2, 2.5)]
    alone = [drv.render(c, stats=False) for c in cams]
    assert len({st["n_tiles"] for _, st in alone}) > 1, [st["n_tiles"] for _, st in alone]      # (or the case proves nothing)
    batch, stats = drv.render_batch_stats(cams)
    for i, (img, st) in enumerate(alone):
        assert (batch[i] == img).all(), f"frame {i} of the batch differs from the frame rendered alone"
        assert stats_without_times(stats[i]) == stats_without_times(st), (i, stats[i], st)
