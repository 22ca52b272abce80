"""GPU campaigns beside the parity tests proper (test_gpu_parity.py): trained-like scenes at every resolution the product renders, the 4K
sweep as batches, the batch overflow redo on real streams, the big-splat list past its capacity, the tiling's independence of the scene's
layout and upload path, refused capacities, and fixed slices of the fuzz campaigns (tests/fuzz_cases.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle_c
import oracle_np as onp
import parity_cases as pc
import fuzz_cases
from conftest import assert_frame_close
from tight_parity import assert_frame_tight
from test_gpu_parity import GpuDriver, BANDS_4K_8, _ocam


@pytest.fixture(scope="module")
def drv():
    d = GpuDriver()
    yield d
    d.close()


def _cam(oc):
    """sage_gs.Camera of an oracle camera (whose view already holds the scene's model transform)."""
    from sage_gs import Camera
    return Camera(oc.width, oc.height, oc.fx, oc.fy, oc.cx, oc.cy, np.asarray(oc.view, np.float64))


def _upload(r, scene):
    """A scene tuple (means, scales, quats, opacities, sh, degree) uploaded without a model transform: cameras come from _ocam."""
    import torch
    from sage_gs import Gaussians
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(r.device)
    return r.upload(Gaussians(*(t(a) for a in scene[:5]), scene[5]))


def _batch_equals_frames_alone(r, scene, cams, rows=None):
    """render_batch of `cams` (default group / group_lanes) against every frame rendered alone: bit for bit, N_v / D / n_tiles equal.
    Returns the frames alone and their stats."""
    import torch
    alone, st1 = [], []
    for c in cams:
        alone.append(r.render(c, scene, tile_rows=rows).clone()); st1.append(dict(r.last_stats))
    batch, bst = r.render_batch(cams, scene, tile_rows=rows, want_stats=True)
    h = cams[0].height
    y0, y1 = (0, h) if rows is None else (16 * rows[0], min(h, 16 * rows[1]))
    for i in range(len(cams)):
        assert torch.equal(batch[i, y0:y1], alone[i][y0:y1]), \
            f"frame {i} of a batch of {len(cams)} (rows {rows}): {int((batch[i, y0:y1] != alone[i][y0:y1]).any(dim=-1).sum())} pixels differ from the frame alone"
        for k in ("n_visible", "d_total", "n_tiles"):
            assert bst[i][k] == st1[i][k], (i, k, bst[i][k], st1[i][k])
    return alone, st1


# ---- A. trained-like statistics (scenes.make_trained_like: what InteriorGS assets look like) --------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """make_trained_like(3 000 000, seed 2), uploaded ONCE on a renderer of its own (D is ~29 M records at 1080p: capacity 96 Mi)."""
    from sage_gs import scenes
    sc = scenes.make_trained_like(3_000_000, seed=2)
    d = GpuDriver()
    d.set_record_capacity(96 << 20)
    d.upload(*sc.as_tuple())
    yield sc, d
    d.close()


@pytest.mark.parametrize("pose", [129, 0, 52, 206])
def test_trained_like_3m_1080p_full_frames_vs_oracle(trained, pose):
    """More whole 1080p frames of the trained-like scene through check_against_oracle (pose 77 is test_gpu_parity's; 129 is the bench's
    slowest pose of room_cameras(n_positions=4, n_yaw=64, seed=2))."""
    from sage_gs import scenes
    sc, d = trained
    cam = scenes.room_cameras(sc, 1920, 1080, n_positions=4, n_yaw=64, seed=2)[pose]
    _, st, aux, _ = pc.check_against_oracle(d, sc.as_tuple(), _ocam(cam, sc), what=f"trained-like 3M @1080p pose {pose} (full frame)", upload=False)
    assert st["d_total"] > 10_000_000
    aux["recheck"].close()


@pytest.mark.parametrize("res", [(320, 240), (640, 480), (1024, 768)], ids=lambda r: f"{r[0]}x{r[1]}")
def test_trained_like_3m_at_the_reference_resolutions_vs_oracle(trained, res):
    """The trained-like scene at the reference's resolutions, the bench's slowest pose: forced fine tiles and the library's own choice
    (fine_shift_of on these statistics), each held against the oracle by the checker (the chosen tiling bit-equal to the forced one it is)."""
    from sage_gs import scenes
    sc, d = trained
    w, h = res
    cam = scenes.room_cameras(sc, w, h, n_positions=4, n_yaw=64, seed=2)[129]
    _, st, aux, _ = pc.check_against_oracle(d, sc.as_tuple(), _ocam(cam, sc), what=f"trained-like 3M @{w}x{h} pose 129 (full frame)", upload=False)
    tiles = {s: -(-w // s) * -(-h // s) for s in (16, 8, 4)}
    print(f"[tiling] trained-like 3M @{w}x{h} pose 129: the library chose {st['n_tiles_default']} tiles "
          f"(16x16: {tiles[16]}, 8x8: {tiles[8]}, 4x4: {tiles[4]}); forced fine: {st['n_tiles_fine']}")
    assert st["n_tiles_default"] in tiles.values()
    aux["recheck"].close()


def test_trained_like_3m_640x480_batch_equals_frames_alone(trained):
    """A render_batch of 16 consecutive headings at 640x480 (two groups of 8 on both group lanes) against the frames rendered alone.
    Record capacity 32 Mi here: the batch's 16 lanes hold 16 x 24 B x 32 Mi = 12.9 GB of queues (an overflowing frame grows them)."""
    from sage_gs import scenes
    sc, d = trained
    d.set_record_capacity(32 << 20)
    cams = [_cam(_ocam(c, sc)) for c in scenes.room_cameras(sc, 640, 480, n_positions=4, n_yaw=64, seed=2)[128:144]]
    alone, st = _batch_equals_frames_alone(d.r, d.scene, cams)
    assert min(s["d_total"] for s in st) > 100_000 and max(float(a.max()) for a in alone) > 0.1
    print(f"[batch] trained-like 3M @640x480: 16 frames bit-equal to the frames alone, tilings {sorted(set(s['n_tiles'] for s in st))}")


# ---- B. BASELINE configs[4] (3840x2160, the 3 M room's 360-pose sweep) as batches ---------------------------------------------------------
@pytest.fixture(scope="module")
def room4k():
    """make_room(3 000 000, seed 2) on a renderer of its own with a record capacity of 32 Mi: 16 lanes (group 8 x group_lanes 2) x 24 B x
    32 Mi = 12.9 GB of queues at most (D of a 4K frame of this scene: ~10-20 M)."""
    from sage_gs import Renderer, scenes
    sc = scenes.make_room(3_000_000, seed=2)
    r = Renderer("cuda:0", record_capacity=32 << 20)
    gs = _upload(r, sc.as_tuple())
    cams = scenes.sweep_cameras(sc, 3840, 2160, n=360, seed=2)
    yield sc, r, gs, cams
    gs.free()
    r.close()


def test_4k_batch_of_consecutive_poses(room4k):
    """16 consecutive poses of the sweep (the shared projection path: k_chunk_cull_group / k_preprocess_shared) against the frames alone;
    one of them (pose 85: not test_gpu_parity's pose 77) held against the oracle, image and counts."""
    sc, r, gs, cams = room4k
    pids = list(range(78, 94))
    ocams = [_ocam(cams[p], sc) for p in pids]
    alone, st = _batch_equals_frames_alone(r, gs, [_cam(c) for c in ocams])
    k = pids.index(85)
    img_ref = r.render(_cam(ocams[k]), gs, loose_cull=True).cpu().numpy()
    st_ref = dict(r.last_stats)
    img = alone[k].cpu().numpy()
    ref, aux = oracle_c.render(*sc.as_tuple(), ocams[k], want="image")
    assert (img_ref == img).all() and st[k]["n_visible"] == aux["n_visible"] and st_ref["d_total"] == aux["D"] and st[k]["d_total"] <= aux["D"]
    assert_frame_close(img, ref, aux["margin"], aux["recheck"], what="3M @ 3840x2160 sweep pose 85 (image + counts)")
    assert_frame_tight(img, ref, aux, what="3M @ 3840x2160 sweep pose 85 (image + counts)")
    aux["recheck"].close()
    print(f"[batch] 3M @4K poses 78-93: 16 frames bit-equal to the frames alone (D {min(s['d_total'] for s in st)}-{max(s['d_total'] for s in st)})")


def test_4k_batch_of_poses_at_stride_23(room4k):
    """16 poses 23 degrees apart (hardly a chunk wanted twice: every frame its own live list) against the frames alone."""
    sc, r, gs, cams = room4k
    pids = [(23 * k + 5) % 360 for k in range(16)]
    _, st = _batch_equals_frames_alone(r, gs, [_cam(_ocam(cams[p], sc)) for p in pids])
    assert min(s["n_visible"] for s in st) > 0
    print(f"[batch] 3M @4K 16 poses at stride 23: bit-equal to the frames alone")


@pytest.mark.parametrize("rows", [BANDS_4K_8[1], BANDS_4K_8[2], (30, 38)], ids=lambda r: f"rows{r[0]}-{r[1]}")
def test_4k_batch_of_a_band(room4k, rows):
    """The call a sharded rank makes: a batch of 16 poses restricted to one band of tile rows of the 8-rank partition (BANDS_4K_8: the bands
    that end and begin at the first binning-window boundary, tile row 34), and a band that straddles it, against the same band alone."""
    sc, r, gs, cams = room4k
    _batch_equals_frames_alone(r, gs, [_cam(_ocam(cams[p], sc)) for p in range(200, 216)], rows=rows)


# ---- C. the batch overflow redo on real streams -----------------------------------------------------------------------------------
def test_batch_on_a_fresh_context_survives_overflowing_frames_on_real_streams():
    """test_emu_parity's overflow test on the GPU, where the group lanes run at once: a batch of 24 frames (three groups of 8 over both group
    lanes) on a fresh context with a record capacity of 1024, some frames overflowing it and some not.  Every frame equals the frame
    rendered alone, bit for bit, with the same N_v / D."""
    import torch
    from sage_gs import Renderer
    scene = pc.random_scene(1200, 9, 0, scale=(0.1, 0.5))
    ocams = []
    for k in range(24):
        V = np.eye(4, dtype=np.float32); V[0, 3] = 0.45 * (k % 12) - 2.5 + (7.0 if k % 3 == 2 else 0.0)      # (16 of 24 overflow)
        ocams.append(onp.Camera(96, 96, 80.0, 80.0, 48.0, 48.0, V))
    cams = [_cam(c) for c in ocams]
    r = Renderer("cuda:0", record_capacity=1024)
    try:
        assert r.tuning()["record_capacity"] == 1024
        gs = _upload(r, scene)
        batch, bst = r.render_batch(cams, gs, want_stats=True)
        batch = batch.clone()
        over = 0
        for i, c in enumerate(cams):
            single = r.render(c, gs, stats=False)
            st = r.last_stats
            over += st["d_total"] > 1024
            assert torch.equal(batch[i], single), f"frame {i} of the batch differs from the frame rendered alone"
            assert (bst[i]["d_total"], bst[i]["n_visible"]) == (st["d_total"], st["n_visible"]), (i, bst[i], st)
        assert 4 <= over <= 20, f"{over} of 24 frames overflow: the batch must mix both kinds"
        print(f"[batch] overflow redo: 24 frames bit-equal to the frames alone, {over} of them overflowing 1024 records")
        gs.free()
    finally:
        r.close()


# ---- E. the tiling does not depend on the layout or the upload path ---------------------------------------------------------------------
def test_tiling_does_not_depend_on_the_layout(drv):
    """parity_cases.case_tiling_does_not_depend_on_the_layout at two sizes (4000: every scene of the sweep; 20 000)."""
    _, tilings = pc.case_tiling_does_not_depend_on_the_layout(drv)
    assert {t for w, t in tilings if w == 128} == {48, 192, 768}, tilings
    pc.case_tiling_does_not_depend_on_the_layout(drv, picks=range(0, 28, 3), n=20_000)


def test_tiling_does_not_depend_on_the_upload_path(drv, tmp_path):
    """The sweep's scenes from the compressed payload and as the fp32 arrays the device decoded from it (SGS_BUF_SCENE_GEOM): same n_tiles,
    N_v, D, and frames bit for bit."""
    import torch
    from sage_gs import Gaussians, _capi, ply
    r = drv.r
    cams = pc.layout_cameras()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    for i in range(0, 28, 2):
        m, s_, q, o, sh, deg = pc.layout_scene(i)
        path = str(tmp_path / f"layout_{i}.ply")
        ply.save_compressed_ply(path, m, s_, q, o, sh, deg)
        chunks, packed, shb, _ = ply.read_compressed_payload(path)
        sc_c = r.upload_compressed(chunks, packed, shb, deg)
        got_c = [(r.render(_cam(c), sc_c, stats=False).clone(), (r.last_stats["n_tiles"], r.last_stats["n_visible"], r.last_stats["d_total"])) for c in cams]
        g = r.debug_buffer(_capi.BUF_SCENE_GEOM, np.float32).reshape(-1, 11)
        shd = r.debug_buffer(_capi.BUF_SCENE_SH, np.float32).reshape(len(m), -1, 3)
        sc_c.free()
        sc_f = r.upload(Gaussians(t(g[:, 0:3]), t(g[:, 4:7]), t(g[:, 7:11]), t(g[:, 3]), t(shd), deg))
        for c, (a, sa) in zip(cams, got_c):
            b = r.render(_cam(c), sc_f, stats=False)
            sb = (r.last_stats["n_tiles"], r.last_stats["n_visible"], r.last_stats["d_total"])
            assert sa == sb and torch.equal(a, b), f"scene {i} at {c.width}x{c.height}: compressed {sa}, fp32 {sb}"
        sc_f.free()


# ---- F. a refused capacity or tuning changes nothing ---------------------------------------------------------------------------------
def test_refused_record_capacity_changes_nothing(drv):
    pc.case_refused_capacity_changes_nothing(drv)


# ---- G. fixed slices of the fuzz campaigns (seeds 434 and 415: the two round-6 tolerances in parity_cases.check_against_oracle) -------
@pytest.mark.parametrize("seed", list(range(400, 416)) + [434])
def test_fuzz_rooms(drv, seed):
    fuzz_cases.room_seed(drv, seed)


@pytest.mark.parametrize("seed", list(range(400, 410)) + [415])
def test_fuzz_trained(drv, seed):
    fuzz_cases.trained_seed(drv, seed)


def test_fuzz_batches(drv):
    """Batch seeds 5000-5029 against the frames alone."""
    frames = sum(fuzz_cases.batch_seed(drv.r, seed) for seed in range(5000, 5030))
    print(f"[batch] fuzz seeds 5000-5029: {frames} frames bit-equal to the frames alone")


# ---- D. the big-splat list past its capacity ------------------------------------------------------------------------------------------
def test_big_splat_list_overflow():
    """More than SGS_BIG_CAP (65 536) splats whose rects span more than SGS_BIG_RECT super-tiles (sgs_common.h): the wave that straddles
    the cap puts some lanes in the list and sends the rest down the per-chunk wave path.  768x768 (48 x 48 tiles, 144 super-tiles):
    66 000 isotropic splats about 2000 px wide at opacity 0.02 (alpha >= 1/255 at the corners: every tile, under the tight ellipse too),
    distinct depths in [2, 20], with 3000 small splats, in random order.  ~150 M records on a renderer of its own (capacity 160 Mi, 3.8 GB
    of queues).  The production frame equals the reference-binning frame and itself; under reference binning D is the sum of the rect
    areas; two tile-row bands of the full frame (rendered whole: a band render clamps the rects, nothing would be big) match the oracle."""
    import torch
    from sage_gs import Renderer, _capi
    W = H = 768
    f = 0.9 * W
    n_big, n_small = 66_000, 3000
    rng = np.random.default_rng(2024)
    z_big = rng.permutation(np.linspace(2.0, 20.0, n_big))
    m_big = np.stack([rng.uniform(-0.05, 0.05, n_big) * z_big, rng.uniform(-0.05, 0.05, n_big) * z_big, z_big], 1)
    s_big = np.repeat((2000.0 * z_big / f)[:, None], 3, 1)
    z_s = rng.uniform(2.0, 20.0, n_small)
    m_s = np.stack([rng.uniform(-0.4, 0.4, n_small) * z_s, rng.uniform(-0.4, 0.4, n_small) * z_s, z_s], 1)
    s_s = np.exp(rng.uniform(np.log(0.005), np.log(0.05), (n_small, 3)))
    means = np.concatenate([m_big, m_s]); scales = np.concatenate([s_big, s_s])
    quats = np.concatenate([np.tile([1.0, 0.0, 0.0, 0.0], (n_big, 1)), rng.normal(size=(n_small, 4)) + 1e-3])
    opac = np.concatenate([np.full(n_big, 0.02), rng.uniform(0.1, 0.9, n_small)])
    sh = 0.5 * rng.normal(size=(n_big + n_small, 1, 3))
    perm = rng.permutation(n_big + n_small)
    f32 = lambda a: np.ascontiguousarray(a[perm], np.float32)
    scene = (f32(means), f32(scales), f32(quats), f32(opac), f32(sh), 0)
    ocam = onp.Camera(W, H, f, f, W / 2.0, H / 2.0, np.eye(4, dtype=np.float32))
    cam = _cam(ocam)
    r = Renderer("cuda:0", record_capacity=160 << 20)
    try:
        gs = _upload(r, scene)
        img = r.render(cam, gs, stats=False).clone(); st = dict(r.last_stats)
        img2 = r.render(cam, gs, stats=False); st2 = dict(r.last_stats)
        img_ref = r.render(cam, gs, full_sort=True, loose_cull=True); st_ref = dict(r.last_stats)
        assert torch.equal(img, img2) and st["d_total"] == st2["d_total"], "two renders of the frame differ"
        assert torch.equal(img, img_ref), "the production frame differs from the reference-binning frame"
        # (the splat table of the reference-binning render: S3's rect of every visible splat)
        ids = r.debug_buffer(_capi.BUF_SLOT_IDS, np.uint32)
        sp = r.debug_buffer(_capi.BUF_SPLATS, np.uint32).reshape(-1, 12)[ids != 0xFFFFFFFF]
        x0, y0, x1, y1 = sp[:, 10] & 0xffff, sp[:, 10] >> 16, sp[:, 11] & 0xffff, sp[:, 11] >> 16
        whole = int(((x0 == 0) & (y0 == 0) & (x1 == 48) & (y1 == 48)).sum())
        print(f"[big] {whole} splats cover the whole 48 x 48 grid (SGS_BIG_CAP 65536); D {st['d_total']} (tight), {st_ref['d_total']} (reference)")
        assert whole > 65_536, whole
        assert st_ref["d_total"] == int(((x1 - x0).astype(np.int64) * (y1 - y0)).sum())
        assert st["d_total"] >= whole * 48 * 48, "the tight bin rects dropped tiles of a splat that reaches every tile"
        full = img.cpu().numpy()
        gs.free()
    finally:
        r.close()
    for r0, r1 in ((0, 2), (23, 25)):
        ref, aux = oracle_c.render(*scene, ocam, None, r0, r1, want="image")
        sl = slice(16 * r0, 16 * r1)
        assert_frame_close(full[sl], ref[sl], aux["margin"][sl], aux["recheck"], what=f"big-splat list overflow, tile rows {r0}-{r1}", y0=sl.start)
        assert_frame_tight(full[sl], ref[sl], aux, y0=sl.start, what=f"big-splat list overflow, tile rows {r0}-{r1}")
        aux["recheck"].close()
