"""Splat records live at the Gaussian's LAYOUT position (preprocess_chunk stores the chunk's visible lanes as one contiguous run) while
everything that NAMES a splat — the tile records, the depth ties, the debug buffers — keeps the Gaussian's original index; the composite
finds a record through the scene's inverse permutation (sgs_kernels.h splat_at).  These cases hold that against the layout that needs no
lookup at all: the same arrays uploaded with sgs_tuning.morton = 0 (layout position = original index).  Every comparison is bit for bit.

Written once and run twice, like parity_cases: under the wave64 emulator (test_emu_layout_records.py, which also seeds the fault — a
gather without the lookup) and on the MI355X (test_gpu_layout_records.py).  A `drv` is a parity_cases driver with upload_compressed and
the debug buffers (frontend_cases.debug_buffer)."""
import functools
import os
import tempfile

import numpy as np

import frontend_cases as fc
import oracle_np as onp
import parity_cases as pc
from sage_gs import _capi, ply

EYE = np.eye(4, dtype=np.float32)
DEAD_ID = 0xFFFFFFFF


class layout:
    """with layout(drv, morton): scenes uploaded inside lie in Z-order (1) or in the caller's order (0)."""

    def __init__(self, drv, morton):
        self.drv, self.morton = drv, morton

    def __enter__(self):
        self.keep = self.drv.tuning()["morton"]
        self.drv.set_tuning(morton=self.morton)
        return self

    def __exit__(self, *exc):
        self.drv.set_tuning(morton=self.keep)
        return False


def scene_perm(drv):
    """SGS_BUF_SCENE_PERM of the last frame's scene: layout position -> original index."""
    return fc.debug_buffer(drv, _capi.BUF_SCENE_PERM, np.uint32).astype(np.int64)


def shots(drv, cam, before=None):
    """What every case compares between the two layouts, of the scene uploaded in drv: the production frame (the instantiation a sweep
    runs: no D_f, the deep-tile cull), the same without the deep-tile cull, the D_f-counting instantiation, the fully sorted queues, the
    debug buffers by index.  before: a camera rendered first, so that the slots dead in `cam` hold another frame's records."""
    s = {}
    if before is not None:
        drv.render(before, stats=False, fine=False)
    s["plain"], s["st_plain"] = drv.render(cam, stats=False, fine=False)
    s["nodeep"], _ = drv.render(cam, stats=False, deep=False, fine=False)
    s["stats"], s["st"] = drv.render(cam, fine=False)
    s["perm"] = scene_perm(drv)
    s["splats_raw"] = fc.debug_buffer(drv, _capi.BUF_SPLATS, np.uint32).reshape(-1, 12)
    s["slot_ids_raw"] = fc.debug_buffer(drv, _capi.BUF_SLOT_IDS, np.uint32)
    s["default"], _ = drv.render(cam, stats=False)                 # (the library's own tiling for this frame)
    s["full"], s["st_full"] = drv.render(cam, full_sort=True, fine=False)
    s["off"], s["ids"], s["live_ids"], s["splats"] = drv.intermediates()
    return s


def both_layouts(drv, scene, cam, before=None):
    """shots() of `scene` uploaded in Z-order and in the caller's order: {1: ..., 0: ...}.  The Z-order must be a real permutation."""
    got = {}
    for morton in (1, 0):
        with layout(drv, morton):
            drv.upload(*scene)
            got[morton] = shots(drv, cam, before)
    n = len(scene[0])
    assert (np.sort(got[1]["perm"]) == np.arange(n)).all() and (got[0]["perm"] == np.arange(n)).all()
    return got


def assert_same_frames(got, what, deep=True):
    a, b = got[1], got[0]
    for k in ("plain", "stats", "default", "full") + (("nodeep",) if deep else ()):
        bad = (a[k] != b[k]).any(axis=-1)
        assert not bad.any(), (f"{what}: the Z-ordered scene's frame '{k}' differs from the frame of the caller's order in {int(bad.sum())} pixels "
                               f"(first at {tuple(int(v) for v in np.argwhere(bad)[0])})")
    assert (a["ids"] == b["ids"]).all(), f"{what}: the fully sorted queues differ between the two layouts"
    for g, name in ((a, "Z-order"), (b, "caller's order")):
        assert (g["nodeep"] == g["plain"]).all(), f"{what}: {name}: SGS_FLAG_NO_DEEP changed the frame"
        assert (g["stats"] == g["plain"]).all() and (g["full"] == g["plain"]).all(), f"{what}: {name}: the frame depends on the instantiation"
    assert a["plain"].max() > 0.05, f"{what}: nothing is drawn"


def assert_strict_queue_order(s, n, what):
    """SGS_BUF_SORTED_SLOTS under SGS_FLAG_FULL_SORT: every queue strictly ordered by (depth bits, original index).  Returns the number
    of adjacent pairs with EQUAL depth bits."""
    key_of = np.zeros(n, np.uint64); key_of[s["live_ids"]] = s["splats"][:, 9].astype(np.uint64)
    ids = s["ids"]
    comp = (key_of[ids] << np.uint64(32)) | ids.astype(np.uint64)
    tile_of = np.repeat(np.arange(len(s["off"]) - 1), np.diff(s["off"]))
    same = tile_of[1:] == tile_of[:-1]
    assert (comp[1:][same] > comp[:-1][same]).all(), f"{what}: a queue is not strictly ordered by (depth bits, index)"
    return int((key_of[ids][1:][same] == key_of[ids][:-1][same]).sum())


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1 / 2.  Ties against the layout; the export by index
PLANES_Z = (2.0, 2.5, 3.0, 4.0)


@functools.lru_cache(maxsize=None)
def tie_planes_scene():
    """192 Gaussians (three chunks) at 48x48 (3x3 tiles of 16 pixels) under the identity view, in four planes facing the camera: tz is the
    stored z, so a plane's Gaussians share their depth bits exactly.  Gaussian i lies in plane i % 4, at a pixel column that DEcreases with
    i // 4 — the original indices run against the Z-order — except every twelfth column, which lies far left of the frame: sixteen
    Gaussians that this camera never sees (dead slots), and that `wide` does see.  Returns (scene, camera, wide)."""
    w = 48
    cam = onp.Camera(w, w, 48.0, 48.0, 24.0, 24.0, EYE.copy())
    wide = onp.Camera(w, w, 10.0, 10.0, 24.0, 24.0, EYE.copy())
    i = np.arange(192)
    k, z = i // 4, np.array(PLANES_Z)[i % 4]
    dead = k % 12 == 5
    px = np.where(dead, -60.0 - k, 47.0 - k)
    py = (k * 11) % 48 + 0.25 * (i % 4)
    means = np.stack([fc.at_pixel(cam, x, y, d) for x, y, d in zip(px, py, z)]).astype(np.float32)
    means[:, 2] = z
    scales = np.repeat((2.5 * z / cam.fx)[:, None], 3, 1)
    return fc.make_scene(means, scales, opac=0.35, seed=61), cam, wide, np.nonzero(dead)[0]


def tie_planes(drv):
    scene, cam, wide, dead = tie_planes_scene()
    return scene, cam, dead, both_layouts(drv, scene, cam, before=wide)


def case_ties_against_the_layout(drv):
    """Whole groups of equal depth bits whose original indices run against the Z-order: the frame, the queues and their tie order must be
    those of the caller's order (where index and layout position coincide), and the oracle's."""
    scene, cam, dead, got = tie_planes(drv)
    what = "ties against the layout"
    n = len(scene[0])
    assert (np.diff(got[1]["perm"]) < 0).any(), f"{what}: SGS_BUF_SCENE_PERM is monotone: the Z-order left the scene in the caller's order"
    bits = scene[0][:, 2].view(np.uint32)
    assert len(np.unique(bits)) == len(PLANES_Z)
    assert_same_frames(got, what)
    for morton in (1, 0):
        ties = assert_strict_queue_order(got[morton], n, f"{what} [morton {morton}]")
        assert ties > 100, f"{what}: only {ties} adjacent records of equal depth bits"
    with layout(drv, 1):
        pc.check_against_oracle(drv, scene, cam, what=what)


def case_export_by_index(drv):
    """SGS_BUF_SPLATS and SGS_BUF_SLOT_IDS present the records by ORIGINAL index whatever the layout, word for word, with dead slots
    blanked — the device holds another frame's records in them (the wide camera's, rendered first)."""
    scene, cam, dead, got = tie_planes(drv)
    what = "export by index"
    a, b = got[1], got[0]
    assert (a["slot_ids_raw"] == b["slot_ids_raw"]).all(), f"{what}: SGS_BUF_SLOT_IDS differs between the two layouts"
    bad = np.nonzero((a["splats_raw"] != b["splats_raw"]).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: SGS_BUF_SPLATS differs between the two layouts at {len(bad)} indices, first {bad[:8]}"
    is_dead = a["slot_ids_raw"] == DEAD_ID
    assert (np.nonzero(is_dead)[0] == dead).all(), f"{what}: dead slots {np.nonzero(is_dead)[0]}, the scene's {dead}"
    assert (a["slot_ids_raw"][~is_dead] == np.nonzero(~is_dead)[0]).all()
    assert (a["splats_raw"][is_dead] == 0).all(), f"{what}: a dead slot is not zero"
    live = a["splats_raw"][~is_dead]
    assert (live[:, 9] == scene[0][~is_dead, 2].view(np.uint32)).all(), f"{what}: a record's depth bits are not its Gaussian's"


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3.  Every gather site, with a non-trivial permutation
GATHER_RES = (160, 112)
TILE_TIES, TILE_LONG, TILE_MULTI, TILE_SINGLE = (1, 1), (5, 3), (8, 5), (3, 5)
SIGMA_PX = 1.6                  # 3-sigma radius 6 px: a splat within 1.5 px of a tile's centre stays inside the tile


@functools.lru_cache(maxsize=None)
def gather_scene():
    """4000 faint specks at 160x112 (no pixel saturates: every queue is read to its end), input arrays reversed.  Four tiles hold a heap each:
      TILE_SINGLE  150 records: one batch (the single-batch gather);
      TILE_MULTI   500 records, 380 of them in a slab of one depth bucket: a group of more than one batch (the multi-batch gather);
      TILE_LONG    1300 records over five octaves: more than the LDS holds, a second window;
      TILE_TIES    the depths of frontend_cases.tie_run_scene(resort=True): a cluster of 1100-odd consecutive bit patterns with runs of
                   2 .. 33 equal ones that stays one oversized bucket — radix-sorted through HBM, the run of 33 through the (index, depth)
                   resort, which reads the keys back from the records (the HBM radix path's gather);
    the rest are spread over the frame.  Returns (scene, camera)."""
    w, h = GATHER_RES
    f = 112.0
    cam = onp.Camera(w, h, f, f, w / 2.0, h / 2.0, EYE.copy())
    rng = np.random.default_rng(71)
    (tie_scene, _, runs) = fc.tie_run_scene(resort=True)
    z_t = tie_scene[0][:, 2].astype(np.float64)
    z_long = np.exp(rng.uniform(0.0, np.log(30.0), 1300))
    z_multi = np.concatenate([np.exp(rng.uniform(0.0, np.log(30.0), 120)), np.linspace(3.0, 3.001, 380)])
    z_single = rng.uniform(1.0, 30.0, 150)
    n_rest = 4000 - len(z_t) - 1300 - 500 - 150
    assert n_rest > 300
    z_rest = rng.uniform(1.0, 30.0, n_rest)
    px, py, z = [], [], []
    for tile, zs in ((TILE_TIES, z_t), (TILE_LONG, z_long), (TILE_MULTI, z_multi), (TILE_SINGLE, z_single)):
        px.append(16 * tile[0] + 7.5 + rng.uniform(-1.5, 1.5, len(zs))); py.append(16 * tile[1] + 7.5 + rng.uniform(-1.5, 1.5, len(zs))); z.append(zs)
    px.append(rng.uniform(0.0, w, n_rest)); py.append(rng.uniform(0.0, h, n_rest)); z.append(z_rest)
    px, py, z = (np.concatenate(a)[::-1].copy() for a in (px, py, z))           # the input arrays reversed
    n = len(z)
    for idx in runs:                     # inside a run of equal depth bits x decreases with the (final) index: the layout holds it last-index-first
        j = np.sort(n - 1 - idx)
        px[j] = 16 * TILE_TIES[0] + 7.5 + np.linspace(1.5, -1.5, len(j)); py[j] = py[j[0]]
    z32 = z.astype(np.float32)
    z32[n - 1 - np.arange(len(z_t))] = tie_scene[0][:, 2]                       # (the tie tile's depths bit for bit)
    means = np.stack([(px - cam.cx + 0.5) * z32 / f, (py - cam.cy + 0.5) * z32 / f, z32], 1).astype(np.float32)
    means[:, 2] = z32
    scales = np.repeat((SIGMA_PX * z32.astype(np.float64) / f)[:, None], 3, 1)
    opac = rng.uniform(0.005, 0.012, n)
    return fc.make_scene(means, scales, opac=opac, seed=72), cam


def gather_sites(drv):
    scene, cam = gather_scene()
    return scene, cam, both_layouts(drv, scene, cam)


def case_every_gather_site(drv):
    """One frame whose tiles take the single-batch gather, the multi-batch gather, a long queue's second window and the HBM radix path with
    its resort, under a Z-order that is far from the identity: the frame, in every instantiation, and the queues are those of the caller's
    order; SGS_FLAG_NO_DEEP changes nothing; the frame is the oracle's."""
    scene, cam, got = gather_sites(drv)
    what = "every gather site"
    n = len(scene[0])
    assert (got[1]["perm"] != np.arange(n)).mean() > 0.9, f"{what}: the Z-order is (nearly) the identity"
    gx = (cam.width + 15) // 16
    lens = np.diff(got[1]["off"])
    at = lambda t: int(lens[t[1] * gx + t[0]])
    assert 0 < at(TILE_SINGLE) <= 256 and 256 < at(TILE_MULTI) <= 1024 and at(TILE_LONG) > 1024 and at(TILE_TIES) > 1024, \
        f"{what}: queue lengths {at(TILE_SINGLE)}, {at(TILE_MULTI)}, {at(TILE_LONG)}, {at(TILE_TIES)}"
    assert got[1]["st"]["n_spill_tiles"] >= 1 and got[1]["st_plain"]["n_spill_tiles"] >= 1, f"{what}: no depth bucket was sorted through HBM"
    assert_same_frames(got, what)
    assert assert_strict_queue_order(got[1], n, what) >= 2 + 3 + 31 + 32 + 33 + 2 + 3 - 7
    with layout(drv, 1):
        pc.check_against_oracle(drv, scene, cam, what=what, thorough=False)


@functools.lru_cache(maxsize=None)
def deep_scene():
    """parity_cases.deep_tile_scene — opaque layers with 5x5 holes in front of a few thousand splats — with the input arrays reversed."""
    scene, cam = pc.deep_tile_scene(n_back=3000)
    return tuple(np.ascontiguousarray(a[::-1]) for a in scene[:5]) + (scene[5],), cam


def case_deep_tile_gather(drv):
    """The deep-tile cull reads 32 bytes of every record of a window: the same frame as in the caller's order, and as without the cull."""
    scene, cam = deep_scene()
    got = both_layouts(drv, scene, cam)
    what = "deep-tile gather"
    assert (got[1]["perm"] != np.arange(len(scene[0]))).mean() > 0.9, f"{what}: the Z-order is (nearly) the identity"
    assert got[1]["st_plain"]["n_deep_windows"] >= 4 and got[0]["st_plain"]["n_deep_windows"] >= 4, f"{what}: no window was culled against the live pixels"
    assert_same_frames(got, what)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 4.  The group path
def group_cameras():
    """Five poses of a short path through gather_scene's frame."""
    w, h = GATHER_RES
    cams = []
    for k, deg in enumerate((-4.0, -2.0, 0.0, 2.0, 4.0)):
        a = np.deg2rad(deg)
        eye = (0.01 * k, 0.0, 0.0)
        cams.append(onp.Camera(w, h, 112.0, 112.0, w / 2.0, h / 2.0, pc.look_at_view(eye, (eye[0] + np.sin(a), 0.0, np.cos(a)))))
    return cams


def case_group_path(drv):
    """sgs_render_batch of five poses (one launch group: k_preprocess_shared writes the records of five frames) equals the five frames
    rendered one at a time — for the fp32 upload and for the compressed one (the quantised scene: another Z-order, the same property)."""
    scene, _ = gather_scene()
    cams = group_cameras()
    means, scales, quats, opac, sh, deg = scene
    with layout(drv, 1), tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "gather.ply")
        ply.save_compressed_ply(path, means, scales, quats, opac, sh, deg)
        payload = ply.read_compressed_payload(path)
        for kind in ("fp32", "compressed"):
            if kind == "fp32":
                drv.upload(*scene)
            else:
                drv.upload_compressed(*payload)
            alone = [drv.render(c, stats=False, fine=False)[0] for c in cams]
            perm = scene_perm(drv)
            assert (perm != np.arange(len(perm))).mean() > 0.9, f"group path [{kind}]: the Z-order is (nearly) the identity"
            batch = drv.render_batch(cams, fine=False)
            for i, a in enumerate(alone):
                bad = (batch[i] != a).any(axis=-1)
                assert not bad.any(), f"group path [{kind}]: frame {i} of the batch differs from the frame rendered alone in {int(bad.sum())} pixels"
            assert all(a.max() > 0.05 for a in alone) and all((alone[i] != alone[j]).any() for i in range(5) for j in range(i))
