"""The visible-object table's checks (sgs_object_table), shared by the CPU-emulator tests (test_emu_objects.py, its mutants) and the GPU
tests (test_gpu_objects.py): the pictures, a driver of the C ABI over plain buffers, and the assertions against tests/object_table_ref.py.
Every comparison is exact equality of every field, z_min by bits: there is no tolerance anywhere in this feature."""
from __future__ import annotations

import numpy as np

import jpeg_cases
import object_table_ref as ref
from abi_driver import POISON, SENTINEL, AbiDriver, GpuBuffers          # POISON: out_rows and out_counts before every call

NONE = ref.ID_NONE
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
# restated from sage-3d_official_amd/csrc/sgs_objects.h (SGS_OBJ_REGION, SGS_OBJ_SLOT_BITS, SGS_OBJ_SLOTS, SGS_OBJ_HASH, obj_slot)
REGION, SLOT_BITS, SLOTS, HASH = 2048, 7, 128, 0x9E3779B1


def slot_of(label):
    return ((int(label) * HASH) & 0xFFFFFFFF) >> (32 - SLOT_BITS)


def chunk_edit(chunk):
    """The edit that makes sgs_object_table cut its frames into launches of `chunk` (SGS_OBJ_MAX_FRAMES, csrc/sgs_objects.h)."""
    return ("#define SGS_OBJ_MAX_FRAMES 65535 ", f"#define SGS_OBJ_MAX_FRAMES {int(chunk)} ")


# ---- pictures: name -> [(ids int32 [H,W], depth fp32 [H,W] or None, n_labels)] ------------------------------------------------------------
def _depth(H, W, seed):
    """Positive depths with plateaus, so that a label's minimum is met at several pixels."""
    d = (np.random.RandomState(seed).randint(8, 70, (H, W)) * 0.125).astype(np.float32)
    return d


def one_pixel():
    return [(np.array([[1]], np.int32), np.array([[2.5]], np.float32), 3), (np.array([[NONE]], np.int32), np.array([[2.5]], np.float32), 3)]


def one_label_ragged():
    """67 x 5, all label 2: image rows end in the middle of a wave."""
    return [(np.full((5, 67), 2, np.int32), _depth(5, 67, 1), 4)]


def bands_and_stripes():
    bands = np.repeat(np.array([0, 0, 1, 1, 0], np.int32)[:, None], 67, 1)         # the same label ends row y and starts row y + 1
    stripes = np.zeros((3, 130), np.int32)
    k = 0
    for y, widths in enumerate(((1, 2, 63, 64), (65, 1, 64), (2, 63, 65))):         # 130 each: runs of 1, 2, 63, 64 and 65 pixels
        x = 0
        for wd in widths:
            stripes[y, x:x + wd] = k % 3
            x += wd; k += 1
        assert x == 130
    shifted = np.roll(stripes.reshape(-1), 17).reshape(3, 130).copy()               # ... and again, begun at other lanes
    return [(bands, _depth(5, 67, 2), 2), (stripes, _depth(3, 130, 3), 3), (shifted, _depth(3, 130, 4), 3)]


def checker_with_holes():
    yy, xx = np.mgrid[0:11, 0:37]
    ids = ((xx + yy) & 1).astype(np.int32)
    ids[np.random.RandomState(5).rand(11, 37) < 0.1] = NONE
    return [(ids, _depth(11, 37, 5), 2)]


def sum_over_2_32():
    """40000 x 6, one label: sum_x = 6 * 40000 * 39999 / 2 = 4.8e9 needs the 64-bit sum; every region updates the one row."""
    return [(np.zeros((6, 40000), np.int32), None, 1)]


def own_label():
    """97 x 53, every pixel its own label: 2048 labels meet in a region's 128 slots — all but the slots' owners take the no-slot path."""
    H, W = 53, 97
    assert min(H * W, REGION) >= 4 * SLOTS and H * W > 2 * REGION
    return [(np.arange(H * W, dtype=np.int32).reshape(H, W), _depth(H, W, 6), H * W)]


def colliding():
    """Five labels that obj_slot sends to one slot, interleaved pixel by pixel: the largest owns the slot, the others have none."""
    same = [k for k in range(1, 20000) if slot_of(k) == slot_of(1)][:5]
    assert len(same) == 5 and len({slot_of(k) for k in same}) == 1
    ids = np.array(same, np.int32)[np.arange(9 * 40) % 5].reshape(9, 40)
    return [(ids, _depth(9, 40, 7), max(same) + 1)]


def edge_labels():
    a = np.array([[0, 1, INT32_MAX - 1, -2, INT32_MIN, NONE, 0, 0]], np.int32)      # n_labels = 1: the id 1 == n_labels is no label
    b = np.array([[0, 6, 7, INT32_MAX - 1, -2, INT32_MIN, 6, 0, NONE, 3]], np.int32).repeat(3, 0)
    return [(a, _depth(1, 8, 8), 1), (b, _depth(3, 10, 9), 7)]


def depth_specials():
    """Label 0 (two image rows): the minimum +0 at several pixels among +inf, -0, a denormal, negatives and NaNs of both signs — every
    run holds patterns with the sign bit.  Label 1: excluded samples only, z_min stays +inf.  Label 2: ordinary depths.  Also without depth."""
    nan_p, nan_n = np.uint32(0x7FC00000).view(np.float32), np.uint32(0xFFC00000).view(np.float32)
    den = np.uint32(1).view(np.float32)
    ids = np.full((4, 16), 2, np.int32)
    d = _depth(4, 16, 10)
    ids[0:2, 0:12] = 0
    d[0, 0:12] = [0.0, 5.0, np.inf, -0.0, den, -3.0, nan_p, nan_n, 0.0, 1.0, 2.0, -1.0]
    d[1, 0:12] = [2.0, 0.0, -0.0, den, np.inf, nan_n, 7.0, -np.inf, 0.0, nan_p, 1.5, 3.0]
    ids[2:4, 0:8] = 1
    d[2, 0:8] = [-1.0, -0.0, nan_p, nan_n, -np.inf, -2.0, -0.0, nan_p]
    d[3, 0:8] = d[2, 0:8][::-1]
    ids[3, 15] = NONE
    return [(ids, d, 3), (ids, None, 3)]


def _collider_labels():
    """(a, b, c): a < b in one slot (the search of colliding()), c in another."""
    same = [k for k in range(1, 20000) if slot_of(k) == slot_of(1)]
    a, b = same[0], same[1]
    c = next(k for k in range(2, 20000) if slot_of(k) != slot_of(a))
    assert a < b and slot_of(a) == slot_of(b) != slot_of(c)
    return a, b, c


MIXED_W, MIXED_H, MIXED_ROWS = 64, 96, REGION // 64          # three regions of 32 image rows each


def mixed_paths():
    """64 x 96, three regions of 32 rows; a < b share a slot, c has another.  Label a changes path from region to region, so its row
    receives the slot's flush of one workgroup and the no-slot sends of two others:
      region 0   a (columns 10..49 of rows 3..28) in c: a owns its slot
      region 1   a and b interleaved in runs of 1 to 5 pixels: b owns the slot, every run of a goes straight to the global row
      region 2   b in the left half, a in the right half but for the last column (c): a has no slot here either
    a touches column 0 and column 63 in region 1 alone and its least depth (0.5, at three pixels) lies there, so x_min, x_end and
    z_min are attained only in region 1; y_min comes from region 0 alone.  y_end is that of a's last image row, which is in region
    2 whatever the placement: no slot there either, so y_end too comes from the no-slot path alone.  Variant [1] moves the least depth
    to region 0 (the slot path)."""
    a, b, c = _collider_labels()
    W, H, R = MIXED_W, MIXED_H, MIXED_ROWS
    ids = np.full((H, W), c, np.int32)
    ids[3:29, 10:50] = a
    rs = np.random.RandomState(12)
    runs = rs.randint(1, 6, REGION)                                               # more runs than the region can hold
    ids[R:2 * R] = np.repeat(np.resize(np.array([a, b], np.int32), REGION), runs)[:REGION].reshape(R, W)
    ids[2 * R:, :W // 2] = b
    ids[2 * R:, W // 2:W - 1] = a
    out = []
    for region in (1, 0):
        d = _depth(H, W, 30 + region)                                             # 1.0 .. 8.625
        ys, xs = np.nonzero(ids[region * R:(region + 1) * R] == a)
        pick = rs.choice(len(ys), 3, replace=False)
        d[ys[pick] + region * R, xs[pick]] = 0.5
        out.append((ids, d, max(a, b, c) + 1))
    return out


NARROW_SIZES = ((1, 2500), (2, 1500), (3, 1000), (5, 700))


def narrow():
    """Frames 1, 2, 3 and 5 pixels wide that cross a region (2500, 3000, 3000 and 3500 pixels): dozens of image rows per wave, a head
    with x == 0 at every few lanes (W = 1: at every lane), x wrapping at every k.  Per size one frame in vertical bands (label = x:
    the label that ends row y differs from the one that starts row y + 1 unless W = 1, where the one label continues across every row
    start) and one in horizontal bands of 1 to 9 rows (the label continues across the row starts inside a band and changes at a
    band's first row); 4 % SGS_ID_NONE sprinkled in, a depth with each."""
    out = []
    for k, (W, H) in enumerate(NARROW_SIZES):
        assert W * H > REGION and (W * H) % REGION != 0
        rs = np.random.RandomState(40 + k)
        yy, xx = np.mgrid[0:H, 0:W]
        band_of_row = np.repeat(np.arange(H), rs.randint(1, 10, H))[:H] % 6
        for ids in (xx.astype(np.int32), np.repeat(band_of_row[:, None], W, 1).astype(np.int32)):
            ids = ids.copy()
            ids[rs.rand(H, W) < 0.04] = NONE
            out.append((ids, _depth(H, W, 50 + len(out)), 6))
    return out


SMALL = (one_pixel, one_label_ragged, bands_and_stripes, checker_with_holes, colliding, edge_labels, depth_specials)
LARGE = (sum_over_2_32, own_label)             # the emulator's largest: one run each there
PATHS = (mixed_paths, narrow)                  # a label that changes path between regions; very narrow frames across regions


def check_picture_properties():
    """What the pictures are built for, from the restatement alone."""
    rows, _ = ref.table(*one_label_ragged()[0])
    r = rows[2]
    assert (r["x_min"], r["y_min"], r["x_end"], r["y_end"], r["n_pixels"]) == (0, 0, 67, 5, 335)
    rows, _ = ref.table(*sum_over_2_32()[0])
    assert int(rows["sum_x"][0]) == 6 * 40000 * 39999 // 2 > 2 ** 32
    ids, d, n = depth_specials()[0]
    rows, counts = ref.table(ids, d, n)
    assert ref.z_bits(rows)[0] == 0 and ref.z_bits(rows)[1] == ref.Z_INF and (d[ids == 0] == 0).sum() >= 4 and counts.tolist() == [1, 0]
    for ids, d, n in edge_labels():
        rows, counts = ref.table(ids, d, n)
        assert counts[1] == 4 * ids.shape[0] and rows["n_pixels"][0] > 0 and rows["n_pixels"][n - 1] > 0
    check_mixed_paths_properties()
    pictures = narrow()
    for k, (W, H) in enumerate(NARROW_SIZES):
        frames = pictures[2 * k:2 * k + 2]                                         # vertical bands, horizontal bands
        for ids, d, n in frames:
            rows, counts = ref.table(ids, d, n)
            assert ids.shape == (H, W) and d is not None and counts[0] > 0 and counts[1] == 0 and (rows["n_pixels"][:min(W, n)] > 0).all()
        across = [(f[0][1:, 0] == f[0][:-1, -1]) & (f[0][1:, 0] != NONE) for f in frames]       # row y's last label starts row y + 1
        assert across[1].any() and not across[1].all() and (across[0].any() if W == 1 else not across[0].any())


def check_mixed_paths_properties():
    """The condition under which mixed_paths can catch a fault of one path alone, from the restatement of each region by itself."""
    a, b, c = _collider_labels()
    R = MIXED_ROWS
    for variant, (ids, d, n) in enumerate(mixed_paths()):
        assert ids.shape == (MIXED_H, MIXED_W) and MIXED_W * R == REGION and MIXED_H == 3 * R
        part = [ref.table(ids[k * R:(k + 1) * R], d[k * R:(k + 1) * R], n)[0] for k in range(3)]     # y counts from the region's first row
        whole = ref.table(ids, d, n)[0]
        labels = [set(np.flatnonzero(p["n_pixels"]).tolist()) for p in part]
        assert labels == [{a, c}, {a, b}, {a, b, c}]             # a owns its slot in region 0 alone: b, the larger, takes it in 1 and 2
        runs = np.diff(np.flatnonzero(np.diff(ids[R:2 * R].reshape(-1)) != 0))
        assert runs.min() == 1 and runs.max() == 5
        pa, wa = [p[a] for p in part], whole[a]
        assert wa["x_min"] == pa[1]["x_min"] == 0 < min(pa[0]["x_min"], pa[2]["x_min"])
        assert wa["x_end"] == pa[1]["x_end"] == MIXED_W > max(pa[0]["x_end"], pa[2]["x_end"])
        assert wa["y_min"] == pa[0]["y_min"] and wa["y_end"] == 2 * R + pa[2]["y_end"] == MIXED_H    # the first row from the slot, the last without one
        z = [int(ref.z_bits(p)[a]) for p in part]
        low = 1 if variant == 0 else 0
        assert int(ref.z_bits(whole)[a]) == z[low] and all(z[low] < z[k] for k in range(3) if k != low)
        assert (d[ids == a] == d[ids == a].min()).sum() == 3


# ---- the C ABI over plain buffers ---------------------------------------------------------------------------------------------------------
class AbiObjects(AbiDriver):
    """sgs_object_table over host buffers; a GPU driver overrides the buffer hooks (GpuObjects)."""

    def _ints(self, a):
        a = np.ascontiguousarray(a, np.int32)
        return a, a.ctypes.data

    def call(self, ids_ptr, depth_ptr, n, H, W, stride, n_labels, rows_ptr, counts_ptr):
        return int(self.lib.sgs_object_table(self.ctx, ids_ptr, depth_ptr, int(n), int(H), int(W), int(stride), int(n_labels), rows_ptr, counts_ptr, None))

    def tables(self, ids, depth, n_labels, stride=None, slack=64):
        """ids int32 [n,H,W], depth fp32 [n,H,W] or None -> (rows ROW_DTYPE [n, n_labels], counts uint32 [n, 2]).  Both outputs hold
        0xA5 bytes before the call, with `slack` bytes behind them that must stay so.  stride: elements from frame to frame (default: a
        frame); the ids between frames are label 0 and the depths NaN and 1e30 in turn."""
        ids = np.asarray(ids, np.int32)
        n, H, W = ids.shape
        st = H * W if stride is None else int(stride)
        ibuf = np.zeros((n, st), np.int32)
        ibuf[:, :H * W] = ids.reshape(n, -1)
        keep_i, i_ptr = self._ints(ibuf.reshape(-1))
        keep_d, d_ptr = (None, None) if depth is None else self._frames(jpeg_cases.strided(np.asarray(depth, np.float32), st))
        row_bytes, cnt_bytes = n * n_labels * ref.ROW_DTYPE.itemsize, n * 8
        keep_r, r_ptr, r_get = self._bytes(row_bytes + slack)
        keep_c, c_ptr, c_get = self._bytes(cnt_bytes + slack)
        self.lib.check(self.call(i_ptr, d_ptr, n, H, W, st, n_labels, r_ptr, c_ptr), self.ctx)
        self._sync()
        rb, cb = np.array(r_get()), np.array(c_get())
        assert (rb[row_bytes:] == SENTINEL).all() and (cb[cnt_bytes:] == SENTINEL).all(), "bytes were written behind the outputs"
        return rb[:row_bytes].view(ref.ROW_DTYPE).reshape(n, n_labels), cb[:cnt_bytes].view(np.uint32).reshape(n, 2)


class GpuObjects(GpuBuffers, AbiObjects):
    """AbiObjects over torch device buffers, on a Renderer's context."""

    def _ints(self, a):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(self.r.device)
        return t, t.data_ptr()


def check_frame(name, rows, counts, ids, depth, n_labels):
    """One frame's table against the restatement; the assertions name the picture, the label and the field."""
    want, want_counts = ref.table(ids, depth, n_labels)
    words = np.ascontiguousarray(rows).view(np.uint32).reshape(n_labels, 10)
    left = (words == POISON).any(1) & (want["n_pixels"] == 0)
    assert not left.any(), f"{name}: the empty row of label {int(np.argmax(left))} was not written (0xA5 bytes are left in it)"
    d = None if rows.tobytes() == want.tobytes() else ref.first_difference(rows, want)
    assert d is None, f"{name}: label {d[0]}: {d[1]} is {d[2]}, the restatement has {d[3]}"
    assert counts.tolist() == want_counts.tolist(), f"{name}: counts are {counts.tolist()}, the restatement has {want_counts.tolist()}"
    total = int(rows["n_pixels"].astype(np.int64).sum()) + int(counts[0]) + int(counts[1])
    assert total == ids.size, f"{name}: rows and counts hold {total} pixels of {ids.size}"


def check_pictures(drv, makers):
    for make in makers:
        for i, (ids, depth, n_labels) in enumerate(make()):
            name = f"{make.__name__}[{i}] {ids.shape[1]}x{ids.shape[0]}"
            rows, counts = drv.tables(ids[None], None if depth is None else depth[None], n_labels)
            check_frame(name, rows[0], counts[0], ids, depth, n_labels)


# ---- rendered frames ----------------------------------------------------------------------------------------------------------------------
def room_cams(w, h, poses=None):
    import mesh_depth_ref
    import mesh_id_cases as ic
    from sage_gs import scenes
    cams = scenes.room_cameras(ic.room(2000)[3], w, h, n_positions=4, n_yaw=4, seed=0)
    return [mesh_depth_ref.of_camera(cams[p]) for p in (ic.ROOM_POSES if poses is None else poses)]


def check_rendered(drv, ids_drv, sizes=((80, 60), (160, 120))):
    """make_room_mesh_parts(2000) from mesh_id_cases' room poses through sgs_render_mesh_ids: the table of those ids and that depth."""
    import mesh_id_cases as ic
    V, T, part, _ = ic.room(2000)
    m = ids_drv.mesh(V, T, part)
    try:
        for w, h in sizes:
            for k, cam in enumerate(room_cams(w, h)):
                ids, z, _ = ids_drv.ids(m, cam)
                assert len(np.unique(ids)) >= 3
                rows, counts = drv.tables(ids[None], z[None], 12)
                check_frame(f"rendered {w}x{h} pose {ic.ROOM_POSES[k]}", rows[0], counts[0], ids, z, 12)
    finally:
        ids_drv.free(m)


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
def batch_frames():
    """Nine different 67 x 5 frames (n_labels 335) with their depths."""
    H, W, n = 5, 67, 335
    rs = np.random.RandomState(11)
    yy, xx = np.mgrid[0:H, 0:W]
    edge = np.resize(edge_labels()[1][0].reshape(-1), H * W).reshape(H, W)
    frames = [np.full((H, W), 2, np.int32), np.repeat(np.array([0, 0, 1, 1, 0], np.int32)[:, None], W, 1), ((xx + yy) & 1).astype(np.int32),
              np.arange(H * W, dtype=np.int32).reshape(H, W), (xx // 9 + 3 * (yy // 2)).astype(np.int32), edge.astype(np.int32),
              rs.randint(-1, 6, (H, W)).astype(np.int32), np.full((H, W), NONE, np.int32), (xx % 7 * 40).astype(np.int32)]
    depth = np.stack([_depth(H, W, 20 + k) for k in range(9)])
    depth[6, 2, 10:20] = -1.0
    return np.stack(frames), depth, n


def check_batches(drv):
    """B = 1, 3 and 9 frames with a padded frame_stride: each frame's table is that of the frame alone, bit for bit."""
    ids, depth, n = batch_frames()
    assert len({f.tobytes() for f in ids}) == 9
    alone = [drv.tables(ids[k:k + 1], depth[k:k + 1], n) for k in range(9)]
    for k in range(9):
        check_frame(f"batch frame {k} alone", alone[k][0][0], alone[k][1][0], ids[k], depth[k], n)
    for B in (1, 3, 9):
        for sel in (slice(0, B), slice(9 - B, 9)):
            rows, counts = drv.tables(ids[sel], depth[sel], n, stride=5 * 67 + 37)
            for j, k in enumerate(range(9)[sel]):
                assert rows[j].tobytes() == alone[k][0][0].tobytes() and counts[j].tolist() == alone[k][1][0].tolist(), \
                    f"B = {B}: the table of frame {k} depends on the batch it is issued in"
            nd, _ = drv.tables(ids[sel], None, n, stride=5 * 67 + 37)
            assert (ref.z_bits(nd.reshape(-1)) == ref.Z_INF).all() and np.array_equal(nd["sum_x"], rows["sum_x"])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def check_refusals(drv):
    """Every refusal of the header returns SGS_ERR_INVALID with a message and leaves the poisoned outputs untouched."""
    keep_i, i_ptr = drv._ints(np.zeros(4 * 64 + 64, np.int32))
    keep_r, r_ptr, r_get = drv._bytes(4 * 3 * 40)
    keep_c, c_ptr, c_get = drv._bytes(4 * 8)

    def call(ids=i_ptr, n=2, H=8, W=8, stride=64, n_labels=3, rows=r_ptr, counts=c_ptr):
        return drv.call(ids, None, n, H, W, stride, n_labels, rows, counts)

    bad = [(b"null ids", dict(ids=None)), (b"null out_rows", dict(rows=None)), (b"null out_counts", dict(counts=None)),
           (b"n_frames = 0", dict(n=0)), (b"n_frames = -1", dict(n=-1)), (b"frame 8 x 0", dict(H=0)), (b"frame 0 x 8", dict(W=0)),
           (b"frame -8 x 8", dict(W=-8)), (b"more than 2^31 - 1 pixels", dict(H=65536, W=32768, stride=2 ** 31)),
           (b"frames overlap", dict(stride=63)), (b"frames overlap", dict(n=1, stride=63)), (b"n_labels = 0", dict(n_labels=0)),
           (b"n_labels = -3", dict(n_labels=-3))]
    for word, kw in bad:
        assert call(**kw) == -1, word
        assert word in drv.lib.sgs_last_error(drv.ctx), (word, drv.lib.sgs_last_error(drv.ctx))
    drv._sync()
    assert (np.array(r_get()) == SENTINEL).all() and (np.array(c_get()) == SENTINEL).all(), "a refused call wrote to its outputs"
    assert call() == 0 and call(n=1, H=46340, W=1, stride=46340 * 4, ids=None) == -1          # the context still works
    drv._sync()
    assert (np.array(r_get())[:2 * 3 * 40].view(ref.ROW_DTYPE)["n_pixels"] == [64, 0, 0, 64, 0, 0]).all()


def check_misaligned(drv):
    """out_rows 4 bytes off its 8-byte alignment, ids, depth and out_counts 1 and 2 bytes off their 4: each is refused with
    SGS_ERR_INVALID and a message that names the argument, before anything is enqueued — the poisoned outputs stay untouched."""
    pad = 16                                                                        # room behind every buffer for the offsets tried
    keep_i, i_ptr = drv._ints(np.zeros(2 * 64 + pad, np.int32))
    keep_d, d_ptr = drv._frames(np.ones(2 * 64 + pad, np.float32))
    keep_r, r_ptr, r_get = drv._bytes(2 * 3 * 40 + 4 * pad)
    keep_c, c_ptr, c_get = drv._bytes(2 * 8 + 4 * pad)
    assert i_ptr % 8 == 0 and d_ptr % 8 == 0 and r_ptr % 8 == 0 and c_ptr % 8 == 0

    def call(ids=0, depth=0, rows=0, counts=0):
        return drv.call(i_ptr + ids, d_ptr + depth, 2, 8, 8, 64, 3, r_ptr + rows, c_ptr + counts)

    bad = [(b"out_rows", dict(rows=4))] + [(word, {arg: off}) for word, arg in ((b"ids", "ids"), (b"depth", "depth"), (b"out_counts", "counts"))
                                           for off in (1, 2)]
    for word, kw in bad:
        assert call(**kw) == -1, f"{word.decode()} off by {kw} bytes was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"aligned" in msg, (word, msg)
    drv._sync()
    assert (np.array(r_get()) == SENTINEL).all() and (np.array(c_get()) == SENTINEL).all(), "a refused call wrote to its outputs"
    assert call() == 0 and call(rows=8, counts=4, ids=4, depth=4) == 0               # aligned, and aligned again: the context still works
    drv._sync()
    assert (np.array(r_get())[8:8 + 2 * 3 * 40].view(ref.ROW_DTYPE)["n_pixels"] == [64, 0, 0, 64, 0, 0]).all()


def check_split(drv, chunk, n_frames=None):
    """2 * chunk + 3 frames of 1 x 1 in one call (chunk: SGS_OBJ_MAX_FRAMES of the library driven): two full launches and a short one,
    each with ids, depth, rows and counts re-based.  n_labels = 2, ids 0, 1, SGS_ID_NONE, 7 in turn, depth 1 + (f % 13) / 8,
    frame_stride 3: every frame's two rows and its counters are the restatement's, and (tables) nothing is written behind either output."""
    n = 2 * chunk + 3 if n_frames is None else int(n_frames)
    assert n > chunk
    f = np.arange(n)
    ids = np.array([0, 1, NONE, 7], np.int32)[f % 4].reshape(n, 1, 1)
    depth = (1 + (f % 13) / 8).astype(np.float32).reshape(n, 1, 1)
    rows, counts = drv.tables(ids, depth, 2, stride=3)
    period = [ref.table(ids[k], depth[k], 2) for k in range(min(n, 52))]             # (id, depth) repeats every lcm(4, 13) frames
    want = np.stack([p[0] for p in period])[f % 52]
    want_counts = np.stack([p[1] for p in period])[f % 52]
    same = (rows.view(np.uint32).reshape(n, 20) == want.view(np.uint32).reshape(n, 20)).all(1) & (counts == want_counts).all(1)
    if not same.all():
        k = int(np.argmin(same))
        check_frame(f"split: frame {k} of {n} (launches of {chunk})", rows[k], counts[k], ids[k], depth[k], 2)
        raise AssertionError(f"split: frame {k} of {n} differs from the restatement")
    return n
