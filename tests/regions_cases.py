"""The checks of the connected regions (sgs_regions_label), shared by the CPU-emulator tests (test_emu_regions.py, its mutants) and
the GPU tests (test_gpu_regions.py): the pictures, a driver of the C ABI over plain buffers, and the assertions against
tests/regions_ref.py.  Every comparison is exact equality: labels, every field of every row and every counter are integers that
depend on the map and the params alone.  Shapes derive from T = sgs_regions_tile(); nothing is larger than (2T+5) x (2T+3), the
smallest size with 3 x 3 tiles and partial tiles on both edges."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

import regions_ref as ref
from abi_driver import SENTINEL, AbiDriver, GpuBuffers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regions_golden.json")
ROW_BYTES = ref.ROW_DTYPE.itemsize


def c_params(nx, ny, source=ref.SRC_MASK8, connectivity=8, lo=1, hi=255, flags=0, reserved=0):
    from sage_gs import _capi
    return _capi.SgsRegionsParams(int(nx), int(ny), int(source), int(connectivity), int(lo), int(hi), int(flags), int(reserved))


# ---- the C ABI over plain buffers -----------------------------------------------------------------------------------------------------
class AbiRegions(AbiDriver):
    """sgs_regions_label over host buffers; a GPU driver overrides the buffer hooks (GpuRegions)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.T = int(self.lib.sgs_regions_tile())

    def call(self, src, n_maps, stride, params, work, labels, rows, max_regions, counts, stream=None):
        return int(self.lib.sgs_regions_label(self.ctx, src, int(n_maps), int(stride), None if params is None else C.byref(params), work, labels, rows,
                                              int(max_regions), counts, stream))

    def _source(self, maps, source, stride):
        maps = np.asarray(maps)
        src = maps.astype(np.uint32) if source == ref.SRC_D2 else maps.astype(np.uint8)
        n, ny, nx = src.shape
        st = ny * nx if stride is None else int(stride)
        assert st >= ny * nx
        buf = np.full((n, st), 0xA5A5A5A5 if source == ref.SRC_D2 else SENTINEL, src.dtype)      # the padding holds sentinel bytes
        buf[:, :ny * nx] = src.reshape(n, ny * nx)
        return self._put(buf) + (n, ny, nx, st)

    def label(self, maps, connectivity=8, source=ref.SRC_MASK8, lo=1, hi=255, max_regions=8, stride=None, slack=64, null_rows=False):
        """maps [n, ny, nx] (bytes, or d2 words with source SRC_D2) -> (labels int32 [n, ny, nx], rows ROW_DTYPE [n, max_regions],
        counts uint32 [n, 4]).  work, labels, rows and counts hold 0xA5 bytes before the call, each with `slack` bytes behind it
        that must stay so.  null_rows: out_rows = NULL (max_regions must be 0)."""
        keep_s, s_ptr, _, n, ny, nx, st = self._source(maps, source, stride)
        words = int(self.lib.sgs_regions_work_words(nx, ny, n))
        chunks = -(-nx * ny // 1024)
        assert words == 2 * n * (nx * ny + chunks), words
        lab_bytes, row_bytes = 4 * n * ny * nx, ROW_BYTES * n * max_regions
        keep_w, w_ptr, w_get = self._bytes(4 * words + slack)
        keep_l, l_ptr, l_get = self._bytes(lab_bytes + slack)
        keep_r, r_ptr, r_get = self._bytes(row_bytes + slack)
        keep_c, c_ptr, c_get = self._bytes(16 * n + slack)
        assert r_ptr % 8 == 0
        self.lib.check(self.call(s_ptr, n, st, c_params(nx, ny, source, connectivity, lo, hi), w_ptr, l_ptr, None if null_rows else r_ptr, max_regions, c_ptr), self.ctx)
        self._sync()
        lb, rb, cb = np.array(l_get()), np.array(r_get()), np.array(c_get())
        assert (np.array(w_get())[4 * words:] == SENTINEL).all(), "bytes were written behind work"
        assert (lb[lab_bytes:] == SENTINEL).all(), "bytes were written behind labels"
        assert (rb[row_bytes:] == SENTINEL).all(), "bytes were written behind out_rows"
        assert (cb[16 * n:] == SENTINEL).all(), "bytes were written behind out_counts"
        return (lb[:lab_bytes].view(np.int32).reshape(n, ny, nx).copy(), rb[:row_bytes].view(ref.ROW_DTYPE).reshape(n, max_regions).copy(),
                cb[:16 * n].view(np.uint32).reshape(n, 4).copy())


class GpuRegions(GpuBuffers, AbiRegions):
    """AbiRegions over torch device buffers, on a Renderer's context."""


# ---- one map against the restatement ------------------------------------------------------------------------------------------------------
_REF = {}


def want_regions(cells, connectivity):
    """ref.label of a picture, computed once: (labels, n)."""
    cells = np.ascontiguousarray(cells, bool)
    key = (cells.shape, cells.tobytes(), connectivity)
    if key not in _REF:
        _REF[key] = ref.label(cells, connectivity)
    return _REF[key]


def check_map(name, labels, rows, counts, cells, connectivity):
    """Labels, then counters, then every field of every row (max_regions = len(rows)) of one map, each on its own assertion."""
    want, n = want_regions(cells, connectivity)
    if not np.array_equal(labels, want):
        j, i = (int(v[0]) for v in np.nonzero(labels != want))
        raise AssertionError(f"{name}: cell ({i}, {j}) has label {int(labels[j, i])}, the restatement has {int(want[j, i])}")
    want_counts = ref.counts_of(want, n)
    assert counts.tolist() == want_counts.tolist(), f"{name}: counters {counts.tolist()}, the restatement has {want_counts.tolist()}"
    want_rows = ref.rows_of(want, n, len(rows))
    for field in ref.ROW_DTYPE.names:
        bad = np.nonzero(rows[field] != want_rows[field])[0]
        assert len(bad) == 0, f"{name}: row {int(bad[0])} has {field} = {int(rows[field][bad[0]])}, the restatement has {int(want_rows[field][bad[0]])}"


def check_pictures(drv, pics, label="", slack_rows=2):
    """pics = {name: (cells bool [ny, nx], connectivity[, max_regions])}: each alone, with `slack_rows` rows more than it has regions
    (they must come back empty) unless the picture says how many."""
    for name, pic in pics.items():
        cells, conn = pic[0], pic[1]
        n = want_regions(cells, conn)[1]
        cap = pic[2] if len(pic) > 2 else n + slack_rows
        labels, rows, counts = drv.label(cells[None], connectivity=conn, max_regions=cap)
        check_map(f"{label}{name} {cells.shape[1]}x{cells.shape[0]} under {conn}", labels[0], rows[0], counts[0], cells, conn)


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------
DENSITIES = (0.3, 0.45, 0.6, 0.8)


def sizes(T):
    edge = (1, 2, T - 1, T, T + 1, 2 * T + 3)
    return [(nx, ny) for nx in edge for ny in edge]


def size_maps(nx, ny):
    rs = np.random.RandomState(1000 * nx + ny)
    return np.stack([rs.rand(ny, nx) < d for d in DENSITIES])


def check_sizes(drv, which=None):
    """Every width x height of the edge set; the four seeded densities as one call of four maps, under both connectivities."""
    for nx, ny in (sizes(drv.T) if which is None else which):
        maps = size_maps(nx, ny)
        for conn in (8, 4):
            cap = max(want_regions(m, conn)[1] for m in maps) + 1
            labels, rows, counts = drv.label(maps, connectivity=conn, max_regions=cap)
            for k, d in enumerate(DENSITIES):
                check_map(f"{nx}x{ny} density {d} under {conn}", labels[k], rows[k], counts[k], maps[k], conn)


# ---- pictures: nx = 2T + 5, ny = 2T + 3 ---------------------------------------------------------------------------------------------------
def shape(T):
    return 2 * T + 3, 2 * T + 5                                                   # (ny, nx)


def blank(T):
    return np.zeros(shape(T), bool)


def corner_diagonal(T):
    """(k, k) for k = T-3 .. T+2 alone: the step (T-1, T-1) -> (T, T) passes the corner four tiles share."""
    a = blank(T)
    for k in range(T - 3, T + 3):
        a[k, k] = True
    return a


def corner_anti_diagonal(T):
    """(x, y) = (T+k, T-1-k) for k = -3 .. 2: the step (T, T-1) -> (T-1, T) passes the same corner the other way."""
    a = blank(T)
    for k in range(-3, 3):
        a[T - 1 - k, T + k] = True
    return a


def comb(T):
    """Teeth in every other column that join only in the last row of the map — the last row of the last tile row."""
    a = blank(T)
    a[:, ::2] = True
    a[-1, :] = True
    return a


def rings(T):
    """Concentric square rings two cells apart round the middle: one region each, cut by every tile border."""
    ny, nx = shape(T)
    j, i = np.mgrid[:ny, :nx]
    return np.maximum(np.abs(j - ny // 2), np.abs(i - nx // 2)) % 2 == 0


def serpentine(T):
    """Every other row, joined at alternating ends: one region that passes all nine tiles."""
    a = blank(T)
    a[::2, :] = True
    for k, j in enumerate(range(1, a.shape[0], 2)):
        a[j, -1 if k % 2 == 0 else 0] = True
    return a


def checkerboard(T):
    ny, nx = shape(T)
    j, i = np.mgrid[:ny, :nx]
    return (i + j) % 2 == 0


def raster_before_tile(T):
    """Region A starts at (T+2, 0), in the second tile; region B at (0, 1), in the first: A is label 1."""
    a = blank(T)
    a[0:2, T + 2] = True
    a[1:3, 0] = True
    return a


def edge_hooks(T):
    """Pieces that touch the map's right and lower edges inside the partial tiles without touching each other: were the cells beyond
    the edge in the set, they would join there."""
    a = blank(T)
    ny, nx = a.shape
    for y0 in (0, T, 2 * T):
        a[y0, 2 * T:] = True
        a[y0 + 2, nx - 1] = True
    a[ny - 1, 3], a[ny - 1, 6], a[ny - 1, T + 4] = True, True, True
    return a


def pictures(T):
    ny, nx = shape(T)
    one = blank(T)
    one[T, T + 1] = True
    row = np.zeros((1, ny), bool)
    row[0, ::2] = True
    board = checkerboard(T)
    return {"empty": (blank(T), 8), "full": (~blank(T), 8), "full under 4": (~blank(T), 4), "single_cell": (one, 8),
            "row_alternating": (row, 8), "column_alternating": (np.ascontiguousarray(row.T), 8),
            "corner_diagonal": (corner_diagonal(T), 8), "corner_diagonal under 4": (corner_diagonal(T), 4),
            "corner_anti_diagonal": (corner_anti_diagonal(T), 8), "corner_anti_diagonal under 4": (corner_anti_diagonal(T), 4),
            "comb": (comb(T), 4), "comb under 8": (comb(T), 8), "rings": (rings(T), 8), "rings under 4": (rings(T), 4),
            "serpentine": (serpentine(T), 4), "checkerboard": (board, 8), "checkerboard under 4": (board, 4, 50),
            "raster_before_tile": (raster_before_tile(T), 8), "edge_hooks": (edge_hooks(T), 8)}


def check_picture_properties(T):
    """The pictures show what they are there for (by the restatement)."""
    ny, nx = shape(T)
    n_of = lambda a, c: want_regions(a, c)[1]                                      # noqa: E731
    assert n_of(corner_diagonal(T), 8) == 1 and n_of(corner_diagonal(T), 4) == 6 and corner_diagonal(T)[T - 1, T - 1] and corner_diagonal(T)[T, T]
    assert n_of(corner_anti_diagonal(T), 8) == 1 and corner_anti_diagonal(T)[T - 1, T] and corner_anti_diagonal(T)[T, T - 1]
    assert n_of(comb(T), 4) == 1 and n_of(comb(T)[:-1], 4) == (nx + 1) // 2
    assert n_of(rings(T), 8) == n_of(rings(T), 4) >= min(ny, nx) // 4 + 1 > 4
    assert n_of(serpentine(T), 4) == 1 and n_of(checkerboard(T), 8) == 1 and n_of(checkerboard(T), 4) == (nx * ny + 1) // 2 > 50
    lab, n = want_regions(raster_before_tile(T), 8)
    assert n == 2 and lab[0, T + 2] == 1 and lab[1, 0] == 2
    assert n_of(edge_hooks(T), 8) == 9


def check_capacity(drv):
    """The checkerboard under 4-connectivity has far more regions than rows: counts[0] stays true, the rows that exist are right, no
    row is written past capacity (the driver's sentinels), and the labels above capacity are still right."""
    check_pictures(drv, {"checkerboard under 4": pictures(drv.T)["checkerboard under 4"]})


# ---- sources ----------------------------------------------------------------------------------------------------------------------------
def check_sources(drv):
    """lo and hi at their ends on a mask of seeded bytes; a d2 map of the clearance restatement with lo = max_d2 + 1."""
    import clearance_ref
    T = drv.T
    nx, ny = T + 3, 9
    rs = np.random.RandomState(11)
    mask = rs.choice(np.array([0, 1, 2, 100, 254, 255], np.uint8), (ny, nx))
    for lo, hi in ((1, 255), (0, 0), (255, 255), (0, 255), (100, 100), (2, 254), (1, 1)):
        cells = ref.in_set(mask, lo, hi)
        assert (mask == lo).any() and (mask == hi).any()
        cap = want_regions(cells, 8)[1] + 1
        labels, rows, counts = drv.label(mask[None], lo=lo, hi=hi, max_regions=cap)
        check_map(f"mask, lo = {lo}, hi = {hi}", labels[0], rows[0], counts[0], cells, 8)
    ob = rs.rand(2 * T + 3, T + 6) < 0.08
    d2 = clearance_ref.d2_two_pass(ob)
    seen = set()
    for max_d2 in (0, 1, 4, 8):
        assert (d2 == max_d2).any() and (d2 == max_d2 + 1).any()
        cells = ref.in_set(d2, max_d2 + 1, 0xFFFFFFFF)
        cap = want_regions(cells, 8)[1] + 1
        labels, rows, counts = drv.label(d2[None], source=ref.SRC_D2, lo=max_d2 + 1, hi=0xFFFFFFFF, max_regions=cap)
        check_map(f"d2 source, lo = {max_d2 + 1}", labels[0], rows[0], counts[0], cells, 8)
        seen.add(labels.tobytes())
    assert len(seen) == 4
    none = np.full((3, 5), 0xFFFFFFFF, np.uint32)                                  # a map without obstacles: every cell free
    labels, rows, counts = drv.label(none[None], source=ref.SRC_D2, lo=1, hi=0xFFFFFFFF, max_regions=2)
    check_map("d2 source, no obstacle", labels[0], rows[0], counts[0], np.ones((3, 5), bool), 8)


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
def batch_maps(T):
    nx, ny = T + 5, T + 2
    rs = np.random.RandomState(7)
    maps = rs.rand(5, ny, nx) < np.array([0.2, 0.35, 0.5, 0.65, 0.9])[:, None, None]
    maps[:, 0, 0] = True                                                           # every map has a region
    return maps


def check_batches(drv):
    """Five different maps in one call, against the restatement and against each map alone, bit for bit; then the same call with a
    padded map_stride and sentinel bytes between the maps."""
    maps = batch_maps(drv.T)
    for conn in (8, 4):
        cap = max(want_regions(m, conn)[1] for m in maps) + 1
        labels, rows, counts = drv.label(maps, connectivity=conn, max_regions=cap)
        for k, m in enumerate(maps):
            check_map(f"batch map {k} under {conn}", labels[k], rows[k], counts[k], m, conn)
            l1, r1, c1 = drv.label(m[None], connectivity=conn, max_regions=cap)
            assert np.array_equal(l1[0], labels[k]) and r1[0].tobytes() == rows[k].tobytes() and np.array_equal(c1[0], counts[k]), f"map {k} depends on the batch"
        padded = drv.label(maps, connectivity=conn, max_regions=cap, stride=maps[0].size + 37)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(padded, (labels, rows, counts))), "the output depends on map_stride"
    assert len({labels[k].tobytes() for k in range(5)}) == 5


# ---- rows -------------------------------------------------------------------------------------------------------------------------------
def rows_picture(T):
    """Three regions of 12 cells (a bar through a tile border, a block, an L through a tile corner), one of 5 and one of 1: the
    largest area is tied between labels 1, 2 and 4."""
    a = blank(T)
    a[1, T - 6:T + 6] = True                                                       # label 1: 12 cells
    a[3:6, 2:6] = True                                                             # label 2: 12 cells
    a[4, T + 9:T + 14] = True                                                      # label 3: 5 cells
    a[T - 6:T + 1, T + 3] = True                                                   # label 4: an L of 7 + 5 = 12 cells
    a[T, T + 3:T + 9] = True
    a[2 * T + 1, 2 * T + 4] = True                                                 # label 5: the last cell of a partial corner tile
    return a


def check_rows(drv):
    """Every field of every row and counter on a picture whose rows are known; the largest-area tie goes to the least label;
    max_regions below, at and above the number of regions; max_regions = 0 with a null out_rows."""
    T = drv.T
    a = rows_picture(T)
    want, n = want_regions(a, 8)
    assert n == 5 and np.bincount(want.reshape(-1))[1:].tolist() == [12, 12, 5, 12, 1]
    for cap in (7, 5, 3, 1):
        labels, rows, counts = drv.label(a[None], max_regions=cap)
        check_map(f"rows picture, max_regions = {cap}", labels[0], rows[0], counts[0], a, 8)
        assert counts[0].tolist() == [5, 42, 12, 1], f"rows picture: counters {counts[0].tolist()}: three regions tie at 12 cells and label 1 is the least"
    labels, rows, counts = drv.label(a[None], max_regions=7)
    r = rows[0]
    assert (int(r["x_min"][0]), int(r["y_min"][0]), int(r["x_end"][0]), int(r["y_end"][0]), int(r["first"][0])) == (T - 6, 1, T + 6, 2, a.shape[1] + T - 6)
    assert (int(r["x_min"][3]), int(r["y_min"][3]), int(r["x_end"][3]), int(r["y_end"][3])) == (T + 3, T - 6, T + 9, T + 1)
    assert int(r["sum_x"][1]) == 3 * (2 + 3 + 4 + 5) and int(r["sum_y"][1]) == 4 * (3 + 4 + 5)
    assert r[5:].tobytes() == ref.empty_rows(2).tobytes(), "the rows past the number of regions are not empty rows"
    labels, rows, counts = drv.label(a[None], max_regions=0, null_rows=True)
    check_map("rows picture, labels only", labels[0], rows[0], counts[0], a, 8)
    flipped = np.ascontiguousarray(a[::-1])                                        # the tie in another order: the L comes first
    labels, rows, counts = drv.label(flipped[None], max_regions=5)
    check_map("rows picture upside down", labels[0], rows[0], counts[0], flipped, 8)


# ---- the reference's own answers ------------------------------------------------------------------------------------------------------------
def geodesic_golden_grids():
    import geodesic_cases
    return {e["name"]: e for e in geodesic_cases.golden()["grids"]}


def check_reachability(label_of):
    """On the closet room and the diagonal gap of geodesic_golden.json: two free cells share a label iff the reference's astar_pixel
    found a path between them.  label_of(free bool [ny, nx]) -> labels."""
    import geodesic_cases
    n_path = n_none = 0
    for name in ("closet_room", "diagonal_gap"):
        e = geodesic_golden_grids()[name]
        free = ~geodesic_cases.golden_grid(e)
        labels = label_of(free)
        want = want_regions(free, 8)[0]
        assert np.array_equal(labels, want), f"{name}: the labels differ from the restatement"
        for g in e["goals"]:
            gi, gj = g["goal"]
            for p in g["pairs"]:
                si, sj = p["start"]
                assert labels[sj, si] != 0 and labels[gj, gi] != 0
                same = labels[sj, si] == labels[gj, gi]
                assert same == (p["path"] is not None), f"{name}: {(si, sj)} -> {(gi, gj)}: one region is {bool(same)}, the reference's path is {p['path'] is not None}"
                n_path += p["path"] is not None
                n_none += p["path"] is None
    assert n_path > 100 and n_none > 20, (n_path, n_none)


def check_reachability_drv(drv):
    check_reachability(lambda free: drv.label(free[None], max_regions=0, null_rows=True)[0][0])


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def golden_occupancy(scene):
    return np.array([list(bytes.fromhex(row)) for row in scene["occupancy"]], np.uint8)


def check_golden(items_of):
    """items_of(occupancy uint8 [h, w], scale, x_min, y_min) equals the items the reference wrote, dict for dict, on every scene."""
    n_items = 0
    for s in golden()["scenes"]:
        occ = golden_occupancy(s)
        assert occ.shape == (s["height"], s["width"])
        got = items_of(occ, s["scale"], s["min"][0], s["min"][1])
        assert len(got) == len(s["items"]), f"{s['name']}: {len(got)} items, the reference wrote {len(s['items'])}"
        for k, (mine, theirs) in enumerate(zip(got, s["items"])):
            for key in theirs:
                assert mine.get(key) == theirs[key], f"{s['name']}: item {k} ({theirs['instance_id']}): {key} differs from the reference's"
            assert mine == theirs
            n_items += 1
    assert n_items > 20


def check_golden_drv(drv):
    from sage_gs import regions
    check_golden(lambda occ, scale, x_min, y_min: regions.semantic_map_items(
        occ, scale, x_min, y_min, label_fn=lambda cells: (lambda out: (out[0][0], int(out[2][0, 0])))(drv.label(cells[None], max_regions=0, null_rows=True))))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def check_refusals(drv):
    """Every refusal of the header returns SGS_ERR_INVALID with a message that names the argument and leaves the poisoned outputs
    untouched; then the context still works."""
    nx, ny, n = 8, 4, 2
    cells = nx * ny
    keep_s, s_ptr, _ = drv._put(np.zeros(2 * cells + 16, np.uint32))
    words = int(drv.lib.sgs_regions_work_words(nx, ny, n))
    keep_w, w_ptr, w_get = drv._bytes(4 * words + 64)
    keep_l, l_ptr, l_get = drv._bytes(4 * n * cells + 64)
    keep_r, r_ptr, r_get = drv._bytes(ROW_BYTES * n * 3 + 64)
    keep_c, c_ptr, c_get = drv._bytes(16 * n + 64)
    # one buffer that holds labels and work side by side, for the overlap cases
    keep_b, b_ptr, b_get = drv._bytes(4 * n * cells + 4 * words + 64)

    def call(src=s_ptr, n_maps=n, stride=cells, work=w_ptr, labels=l_ptr, rows=r_ptr, max_regions=3, counts=c_ptr, null_params=False, **kw):
        return drv.call(src, n_maps, stride, None if null_params else c_params(**{**dict(nx=nx, ny=ny), **kw}), work, labels, rows, max_regions, counts)

    D = ref.SRC_D2
    bad = [(b"null src", dict(src=None)), (b"null params", dict(null_params=True)), (b"null work", dict(work=None)), (b"null labels", dict(labels=None)),
           (b"null out_counts", dict(counts=None)), (b"null out_rows", dict(rows=None)), (b"max_regions = -1", dict(max_regions=-1)),
           (b"max_regions = -1", dict(max_regions=-1, rows=None)), (b"n_maps = 0", dict(n_maps=0)), (b"n_maps = -2", dict(n_maps=-2)),
           (b"n_maps = 65536", dict(n_maps=65536)), (b"nx = 0", dict(nx=0)), (b"ny = 0", dict(ny=0)), (b"nx = 4097", dict(nx=4097, stride=2 ** 40)),
           (b"ny = 4097", dict(ny=4097, stride=2 ** 40)), (b"unknown source 2", dict(source=2)), (b"unknown source -1", dict(source=-1)),
           (b"unknown connectivity 6", dict(connectivity=6)), (b"unknown connectivity 0", dict(connectivity=0)), (b"unknown connectivity -8", dict(connectivity=-8)),
           (b"lo = 9 > hi = 8", dict(lo=9, hi=8)), (b"hi = 256 with a mask", dict(hi=256)), (b"hi = 4294967295 with a mask", dict(hi=0xFFFFFFFF)),
           (b"unknown flags 0x1", dict(flags=1)), (b"unknown flags 0x80000000", dict(flags=0x80000000)), (b"reserved = 7", dict(reserved=7)),
           (b"reserved = -1", dict(reserved=-1)), (b"map_stride", dict(stride=cells - 1)), (b"map_stride", dict(n_maps=1, stride=0)),
           (b"work 0x", dict(work=w_ptr + 2)), (b"labels 0x", dict(labels=l_ptr + 1)), (b"out_counts 0x", dict(counts=c_ptr + 2)),
           (b"src 0x", dict(src=s_ptr + 2, source=D, hi=0xFFFFFFFF)), (b"out_rows 0x", dict(rows=r_ptr + 4)),
           (b"overlap", dict(labels=b_ptr, work=b_ptr)), (b"overlap", dict(labels=b_ptr, work=b_ptr + 4 * n * cells - 4)),
           (b"overlap", dict(work=b_ptr, labels=b_ptr + 4 * words - 4))]
    for word, kw in bad:
        assert call(**kw) == -1, f"{word.decode()} with {kw} was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"sgs_regions_label" in msg, (word, msg)
    drv._sync()
    for get, what in ((w_get, "work"), (l_get, "labels"), (r_get, "out_rows"), (c_get, "out_counts"), (b_get, "labels or work")):
        assert (np.array(get()) == SENTINEL).all(), f"a refused call wrote to {what}"
    W = drv.lib.sgs_regions_work_words
    assert W(0, 4, 1) == -1 and W(4, 4097, 1) == -1 and W(4, 4, 0) == -1 and W(4, 4, 65536) == -1 and W(4096, 4096, 1) == 2 * (4096 * 4096 + 16384)
    # the context still works: labels right behind work is fine, a mask may start at any byte, rows may be null with max_regions = 0
    assert call() == 0 and call(src=s_ptr + 1, labels=b_ptr + 4 * words, work=b_ptr, rows=None, max_regions=0) == 0
    drv._sync()
    assert np.array(c_get())[:16 * n].view(np.uint32).tolist() == [0, 0, 0, 0] * n          # (a map of zero bytes: nothing is in the set)
    assert (np.array(l_get())[:4 * n * cells] == 0).all() and np.array(r_get())[:ROW_BYTES * n * 3].tobytes() == ref.empty_rows(n * 3).tobytes()
