"""The clearance map's checks (sgs_clearance_map, sgs_clearance_query), shared by the CPU-emulator tests (test_emu_clearance.py, its
mutants) and the GPU tests (test_gpu_clearance.py): the pictures, a driver of the C ABI over plain buffers, and the assertions against
tests/clearance_ref.py.  Every comparison is exact equality: there is no tolerance anywhere in this feature."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

import clearance_ref as ref
from abi_driver import POISON, SENTINEL, AbiDriver, GpuBuffers      # POISON: work, d2, out_counts and out before every call

NONE = ref.NONE
INF, NAN = float("inf"), float("nan")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clearance_golden.json")


# ---- pictures: {name: bool [ny, nx]} ---------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (1, 7), (7, 1), (63, 3), (64, 3), (65, 3), (129, 5), (3, 257), (130, 97))      # nx x ny: wave, word and row ends
DENSITIES = (0.002, 0.01, 0.3)


def _single(nx, ny, i, j):
    ob = np.zeros((ny, nx), bool)
    ob[j, i] = True
    return ob


def size_pictures(nx, ny, seed=0):
    """No obstacle, all obstacles, one obstacle in each corner, seeded random maps at 0.2 %, 1 % and 30 %."""
    pics = {"none": np.zeros((ny, nx), bool), "all": np.ones((ny, nx), bool)}
    for name, (i, j) in (("corner_nw", (0, 0)), ("corner_ne", (nx - 1, 0)), ("corner_sw", (0, ny - 1)), ("corner_se", (nx - 1, ny - 1))):
        pics[name] = _single(nx, ny, i, j)
    rs = np.random.RandomState(1000 * nx + ny + seed)
    for d in DENSITIES:
        pics[f"random_{d}"] = rs.rand(ny, nx) < d
    return pics


def lane_pictures():
    """One obstacle at lane 0, 63 and 64 of a row (and the row's last cell) in rows of 65, 129 and 130 cells: every other cell's
    nearest obstacle of its row lies in another word, to its left for one picture and to its right for another."""
    pics = {}
    for nx, ny in ((65, 3), (129, 5), (130, 5)):
        for i in (0, 63, 64, nx - 1):
            pics[f"lane_{i}_of_{nx}x{ny}"] = _single(nx, ny, i, 1)
    return pics


def shape_pictures():
    pics = {}
    ob = np.zeros((5, 130), bool)                                                  # rows 1..3 hold nothing, between rows that do
    ob[0, 3] = ob[4, 100] = True
    pics["empty_rows_between"] = ob
    ob = np.zeros((7, 130), bool)                                                  # (100, 3): 100 cells along its own row, 1 cell up
    ob[3, 0] = ob[2, 100] = True
    pics["one_up_beats_the_own_row"] = ob
    pics["only_below"] = _single(3, 257, 1, 256)                                   # every cell's nearest obstacle is below it
    pics["only_above"] = _single(3, 257, 1, 0)
    ob = np.zeros((9, 12), bool)                                                   # cell (3, 4): (0, 0) at 9 + 16 and (8, 4) at 25 + 0
    ob[0, 0] = ob[4, 8] = True
    pics["ties"] = ob
    ob = np.zeros((40, 70), bool)                                                  # a cell of lane 0 that walks far beside lanes that stop at once
    ob[:, 1:] = True
    ob[39, 0] = True
    pics["first_lane_walks_alone"] = ob.copy()
    ob = np.zeros((40, 70), bool)
    ob[:, 0] = True
    ob[39, 69] = True
    pics["last_lanes_walk_on"] = ob
    return pics


def check_picture_properties():
    p = shape_pictures()
    d = ref.d2_two_pass(p["ties"])
    assert d[4, 3] == 25 and ref.row_distance(p["ties"])[4, 3] == 5
    g = ref.row_distance(p["one_up_beats_the_own_row"])
    assert g[3, 100] == 100 and ref.d2_two_pass(p["one_up_beats_the_own_row"])[3, 100] == 1
    g = ref.row_distance(p["empty_rows_between"])
    assert (g[1:4] == -1).all() and (g[0] >= 0).all() and (g[4] >= 0).all()
    d = ref.d2_two_pass(p["last_lanes_walk_on"])
    assert d[0, 69] == 39 * 39 and d[0, 1] == 1                                     # lane 0 stops at once, lane 69 - 64 = 5 of word 1 walks 38 rows
    for name, ob in lane_pictures().items():
        g = ref.row_distance(ob)
        assert ob.shape[1] > 64 and ob.sum() == 1 and (g[1] >= 0).all() and (g[0] == -1).all(), name      # cells of another word than the obstacle's
    assert any(not ob.any() for ob in size_pictures(1, 7).values()) and size_pictures(130, 97)["random_0.002"].sum() > 5


# ---- the C ABI over plain buffers ---------------------------------------------------------------------------------------------------------
def c_params(nx, ny, source=ref.SRC_MASK8, flags=0, min_hits=0, max_d2=0, reserved=0):
    from sage_gs import _capi
    return _capi.SgsClearanceParams(int(nx), int(ny), int(source), int(flags), int(min_hits), int(max_d2), int(reserved))


def c_frame(f: ref.Frame):
    from sage_gs import _capi
    return _capi.SgsClearanceFrame(f.min_x, f.min_y, f.sum_x, f.sum_y, f.scale, f.flags, f.margin, f.max_d2, f.n_samples, f.reserved)


class AbiClearance(AbiDriver):
    """sgs_clearance_map and sgs_clearance_query over host buffers; a GPU driver overrides the buffer hooks (GpuClearance)."""

    def call(self, src, n, stride, params, work, d2, counts, stream=None):
        return int(self.lib.sgs_clearance_map(self.ctx, src, int(n), int(stride), None if params is None else C.byref(params), work, d2, counts, stream))

    def call_query(self, d2, nx, ny, segs, n, frame, out, stream=None):
        cf = None if frame is None else C.byref(c_frame(frame) if isinstance(frame, ref.Frame) else frame)
        return int(self.lib.sgs_clearance_query(self.ctx, d2, int(nx), int(ny), segs, int(n), cf, out, stream))

    def map(self, maps, min_hits=1, unseen_blocks=False, max_d2=0, stride=None, slack=64, stream=None):
        """maps: bool / uint8 [n,ny,nx] (a mask) or uint32 [n,ny,nx,2] (a seen map) -> (d2 uint32 [n,ny,nx], counts uint32 [n,4]).
        work, d2 and out_counts hold 0xA5 bytes before the call, each with `slack` bytes behind it that must stay so.  stride:
        elements from map to map (default: a map); the elements between maps are 0xA5 bytes — obstacles, and hits without number."""
        maps = np.asarray(maps)
        topdown = maps.ndim == 4
        src = maps.astype(np.uint32) if topdown else maps.astype(np.uint8)
        n, ny, nx = src.shape[:3]
        per_map = ny * nx * (2 if topdown else 1)
        st = per_map if stride is None else int(stride)
        assert st >= per_map
        buf = np.full((n, st), POISON if topdown else SENTINEL, src.dtype)
        buf[:, :per_map] = src.reshape(n, per_map)
        keep_s, s_ptr, _ = self._put(buf)
        out_bytes = 4 * n * ny * nx
        keep_w, w_ptr, w_get = self._bytes(out_bytes + slack)
        keep_d, d_ptr, d_get = self._bytes(out_bytes + slack)
        keep_c, c_ptr, c_get = self._bytes(16 * n + slack)
        p = c_params(nx, ny, ref.SRC_TOPDOWN if topdown else ref.SRC_MASK8, ref.UNSEEN_BLOCKS if unseen_blocks else 0, min_hits if topdown else 0, max_d2)
        self.lib.check(self.call(s_ptr, n, st, p, w_ptr, d_ptr, c_ptr, stream), self.ctx)
        self._sync()
        wb, db, cb = np.array(w_get()), np.array(d_get()), np.array(c_get())
        assert (wb[out_bytes:] == SENTINEL).all(), "bytes were written behind work"
        assert (db[out_bytes:] == SENTINEL).all(), "bytes were written behind d2"
        assert (cb[16 * n:] == SENTINEL).all(), "bytes were written behind out_counts"
        return db[:out_bytes].view(np.uint32).reshape(n, ny, nx), cb[:16 * n].view(np.uint32).reshape(n, 4)

    def query(self, d2, frame: ref.Frame, segs, slack=64, stream=None):
        """d2 uint32 [ny,nx], segs float64 [n,4] -> int64 [n,2]."""
        d2 = np.ascontiguousarray(d2, np.uint32)
        segs = np.ascontiguousarray(segs, np.float64).reshape(-1, 4)
        n = len(segs)
        keep_d, d_ptr, _ = self._put(d2)
        keep_s, s_ptr, _ = self._put(segs)
        keep_o, o_ptr, o_get = self._bytes(8 * n + slack)
        self.lib.check(self.call_query(d_ptr, d2.shape[1], d2.shape[0], s_ptr, n, frame, o_ptr, stream), self.ctx)
        self._sync()
        ob = np.array(o_get())
        assert (ob[8 * n:] == SENTINEL).all(), "bytes were written behind out"
        return ob[:8 * n].view(np.uint32).reshape(n, 2).astype(np.int64)


class GpuClearance(GpuBuffers, AbiClearance):
    """AbiClearance over torch device buffers, on a Renderer's context."""


def check_map(name, d2, counts, ob, max_d2=0):
    """One map's d2 and counters against the restatement; the assertion names the picture and the cell."""
    want = ref.d2_two_pass(ob)
    if not np.array_equal(d2, want):
        j, i = (int(v[0]) for v in np.nonzero(d2 != want))
        left = " (0xA5 bytes are left in it)" if int(d2[j, i]) == POISON else ""
        raise AssertionError(f"{name}: d2 of cell ({i}, {j}) is {int(d2[j, i])}{left}, the restatement has {int(want[j, i])}")
    want_counts = ref.counts(want, max_d2)
    assert counts.tolist() == want_counts, f"{name}: counts are {counts.tolist()}, the restatement has {want_counts}"
    assert int(counts.astype(np.int64).sum()) == ob.size, f"{name}: the counters do not sum to the cells"


def check_pictures(drv, pics, label=""):
    for name, ob in pics.items():
        d2, counts = drv.map(ob[None])
        check_map(f"{label}{name} {ob.shape[1]}x{ob.shape[0]}", d2[0], counts[0], ob)


def check_sizes(drv, sizes=SIZES):
    for nx, ny in sizes:
        check_pictures(drv, size_pictures(nx, ny), f"{nx}x{ny} ")


# ---- batches, counters, the seen map --------------------------------------------------------------------------------------------------------
def batch_maps():
    """Nine different maps of 67 x 9, the fifth without an obstacle."""
    rs = np.random.RandomState(5)
    maps = rs.rand(9, 9, 67) < np.array([0.01, 0.3, 0.05, 0.002, 0.0, 0.02, 0.5, 0.01, 0.1])[:, None, None]
    assert len({m.tobytes() for m in maps}) == 9 and not maps[4].any() and maps[3].any()
    return maps


def check_batches(drv):
    """1, 3 and 9 maps with a padded map_stride whose padding is 0xA5 bytes (obstacles, if they were read): every map's d2 and
    counters are those of the map alone."""
    maps = batch_maps()
    alone = [drv.map(maps[k:k + 1], max_d2=4) for k in range(9)]
    for k in range(9):
        check_map(f"batch map {k} alone", alone[k][0][0], alone[k][1][0], maps[k], 4)
    for B in (1, 3, 9):
        for sel in (slice(0, B), slice(9 - B, 9)):
            d2, counts = drv.map(maps[sel], max_d2=4, stride=9 * 67 + 37)
            for j, k in enumerate(range(9)[sel]):
                check_map(f"B = {B}, map {k}", d2[j], counts[j], maps[k], 4)
                assert np.array_equal(d2[j], alone[k][0][0]) and counts[j].tolist() == alone[k][1][0].tolist(), f"B = {B}: map {k} depends on the batch"


def check_counters(drv):
    """max_d2 at 0, at a value the map holds, just below and above it, and at NONE - 1; a map without obstacles beside one with."""
    ob = size_pictures(130, 97)["random_0.002"]
    want = ref.d2_two_pass(ob)
    present = int(np.median(want))
    assert 0 < present < NONE and (want == present).any()
    both = np.stack([ob, np.zeros_like(ob)])
    for max_d2 in (0, present, present - 1, present + 1, NONE - 1):
        d2, counts = drv.map(both, max_d2=max_d2)
        check_map(f"max_d2 = {max_d2}", d2[0], counts[0], ob, max_d2)
        assert counts[1].tolist() == [0, 0, 0, ob.size] and (d2[1] == NONE).all(), f"max_d2 = {max_d2}: a map without obstacles: {counts[1].tolist()}"
    assert ref.counts(want, present)[1] > ref.counts(want, present - 1)[1] and ref.counts(want, NONE - 1)[2] == 0


def seen_maps():
    """uint32 [2, 11, 70, 2]: hits 0 .. 5 in both channels (cells on both sides of min_hits 1 and 3, seen and unseen), then a map
    whose occupied hits are all below 3 while its free hits are not."""
    rs = np.random.RandomState(8)
    a = (rs.randint(0, 6, (11, 70, 2)) * (rs.rand(11, 70, 2) < 0.25)).astype(np.uint32)
    b = np.stack([rs.randint(0, 6, (11, 70)), rs.randint(0, 3, (11, 70)) * (rs.rand(11, 70) < 0.1)], -1).astype(np.uint32)
    return np.stack([a, b])


def check_seen_maps(drv, grids=None, label="seen map"):
    grids = seen_maps() if grids is None else grids
    for min_hits in (1, 3):
        for unseen in (False, True):
            d2, counts = drv.map(grids, min_hits=min_hits, unseen_blocks=unseen, max_d2=2, stride=grids[0].size + 10)
            for k in range(len(grids)):
                ob = ref.obstacles(grids[k], ref.SRC_TOPDOWN, min_hits, unseen)
                check_map(f"{label} {k}, min_hits = {min_hits}, unseen_blocks = {unseen}", d2[k], counts[k], ob, 2)


def check_seen_map_properties():
    g = seen_maps()
    ob = [[ref.obstacles(g[0], None, m, u) for u in (False, True)] for m in (1, 3)]
    assert ob[0][0].sum() > ob[1][0].sum() > 0 and ob[0][1].sum() > ob[0][0].sum() and ob[1][1].sum() > ob[0][1].sum()
    assert ((g[0][..., 1] == 3).sum() > 0) and ((g[0][..., 1] == 1).sum() > 0)      # hits exactly at min_hits
    assert not ref.obstacles(g[1], None, 3).any() and (g[1][..., 0] >= 3).any()     # the free channel would make obstacles, the occupied does not
    assert ref.obstacles(seen_maps()[1], None, 3, True).any()


# ---- queries --------------------------------------------------------------------------------------------------------------------------------
def id_map(nx=9, ny=7):
    """A d2 map that names its cells: d2[j][i] = 100 j + i + 1."""
    return (100 * np.arange(ny)[:, None] + np.arange(nx)[None, :] + 1).astype(np.uint32)


PLAIN = ref.Frame(min_x=1.0, min_y=-2.0, sum_x=0.0, sum_y=0.0, scale=0.25, flags=0, margin=2, max_d2=305, n_samples=1)      # k + 0.5 is exact at 0.25


def check_query(name, drv, d2, frame, segs):
    got, want = drv.query(d2, frame, segs), ref.query(d2, frame, segs)
    if not np.array_equal(got, want):
        k = int(np.nonzero((got != want).any(1))[0][0])
        raise AssertionError(f"{name}: segment {k} {np.asarray(segs, np.float64).reshape(-1, 4)[k].tolist()} gives {got[k].tolist()}, the restatement has {want[k].tolist()}")
    return got


def half_way_points(nx=9):
    """End points whose (x - min_x) / scale is exactly k + 0.5, k = -4 .. nx + 2, in row 3."""
    ks = np.arange(-4, nx + 3)
    x = 1.0 + 0.25 * (ks + 0.5)
    return ks, np.stack([x, np.full_like(x, -2.0 + 0.75), x, np.full_like(x, -2.0 + 0.75)], 1)


def check_rounding(drv):
    """rint is ties-to-even: k + 0.5 goes to k for even k and to k + 1 for odd k; -2.5 goes to -2 (inside the margin, clamped to 0)
    and -3.5 to -4 (outside); nx + 1.5 = 10.5 goes to 10 (inside the margin of 2), nx + 2.5 to 12 (outside)."""
    d2 = id_map()
    ks, segs = half_way_points()
    got = check_query("half-way points", drv, d2, PLAIN, segs)
    cell = {int(k): int(v) for k, v in zip(ks, got[:, 1])}
    assert cell[2] == 303 and cell[3] == 305 and cell[0] == 301 and cell[1] == 303 and cell[-1] == 301 and cell[-3] == 301, cell
    assert cell[-4] == NONE and cell[8] == 309 and cell[9] == 309 and cell[10] == 309 and cell[11] == NONE, cell
    assert got[:, 0].tolist() == [1 if v == NONE or v <= 305 else 0 for v in got[:, 1]]
    ys = np.stack([np.full(5, 1.0), -2.0 + 0.25 * (np.arange(5) + 0.5), np.full(5, 1.0), -2.0 + 0.25 * (np.arange(5) + 0.5)], 1)
    assert check_query("half-way rows", drv, d2, PLAIN, ys)[:, 1].tolist() == [1, 201, 201, 401, 401]


def query_segments(seed=3, n=200):
    """Seeded segments over and around a 9 x 7 map of cells of 0.25 from (1, -2), some ending far outside."""
    rs = np.random.RandomState(seed)
    s = np.stack([rs.uniform(0.0, 4.0, n), rs.uniform(-3.0, 0.5, n), rs.uniform(0.0, 4.0, n), rs.uniform(-3.0, 0.5, n)], 1)
    s[::17, 2] = 50.0
    return s


def check_flags_margins_samples(drv):
    d2 = id_map()
    segs = query_segments()
    base = PLAIN.but(sum_x=1.0 + 3.0, sum_y=-2.0 - 0.5, max_d2=250, n_samples=10)
    mirrored = np.concatenate([segs, -segs, np.stack([4.0 - segs[:, 0], segs[:, 1], 4.0 - segs[:, 2], segs[:, 3]], 1)])
    seen = set()
    for flags in (0, ref.NEGATE, ref.FLIP_X, ref.FLIP_Y, ref.NEGATE | ref.FLIP_X | ref.FLIP_Y):
        for margin in (0, 2):
            for n_samples in (0, 1, 2, 10):
                got = check_query(f"flags = {flags}, margin = {margin}, n_samples = {n_samples}", drv, d2, base.but(flags=flags, margin=margin, n_samples=n_samples), mirrored)
                seen |= set(got[:, 0].tolist())
    assert seen == set(range(11)), seen                                             # every sample index is some segment's first hit
    f0, f2 = base.but(margin=0, n_samples=1), base.but(margin=2, n_samples=1)
    edge = np.array([[0, 0, 1.0 - 0.5, -1.0], [0, 0, 1.0 - 0.75, -1.0], [0, 0, 1.0 + 2.5, -1.0]])      # px = -2, -3, 10
    assert drv.query(d2, f0, edge)[:, 1].tolist() == [NONE, NONE, NONE] and drv.query(d2, f2, edge)[:, 1].tolist() == [401, NONE, 409]
    # a start that collides does not count: the samples run from 1
    start_only = np.array([[1.0, -2.0, 1.0 + 8 * 0.25, -2.0 + 6 * 0.25]])
    want = ref.query(d2, base.but(max_d2=1), start_only)
    assert want[0].tolist() == [0, 609], want                                       # only the start point lies on the one colliding cell
    assert drv.query(d2, base.but(max_d2=1), start_only).tolist() == want.tolist()


def check_non_finite(drv):
    """NaN and +-inf coordinates collide, and the end point's d2 is NONE — the stated departure from the reference."""
    d2 = id_map()
    f = PLAIN.but(max_d2=0, n_samples=10)
    ok = [2.0, -1.0]
    segs = np.array([ok + [NAN, -1.0], ok + [2.0, INF], ok + [-INF, -1.0], [NAN, -1.0] + ok, [INF, -1.0] + ok, ok + ok])
    got = check_query("non-finite", drv, d2, f, segs)
    assert got.tolist() == [[1, NONE], [1, NONE], [1, NONE], [1, NONE], [1, NONE], [0, 405]], got.tolist()
    got = check_query("non-finite end points", drv, d2, f.but(n_samples=1), segs)
    assert got.tolist() == [[1, NONE], [1, NONE], [1, NONE], [0, 405], [0, 405], [0, 405]], got.tolist()


# ---- the reference's own answers ------------------------------------------------------------------------------------------------------------
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def write_golden_map(entry, tmp_dir):
    path = os.path.join(str(tmp_dir), entry["name"] + ".json")
    with open(path, "w") as fh:
        json.dump(entry["instances"], fh)
    return path


def check_golden(drv, tmp_dir):
    """The host load reproduces the reference's bounds and size; d2 <= inflation_limit reproduces its obstacle_map at every radius; the
    query reproduces every recorded check_collision_3d and check_path_collision_3d answer."""
    from sage_gs import clearance
    g = golden()
    for e in g["maps"]:
        mask, (min_x, max_x, min_y, max_y) = clearance.load_semantic_map(write_golden_map(e, tmp_dir), e["scale"])
        assert [min_x, max_x, min_y, max_y] == e["bounds"] and list(mask.shape) == e["size"], e["name"]
        d2, counts = drv.map(mask[None])
        raw = np.array([[c == "1" for c in row] for row in e["obstacle_map"]["0.0"]])
        assert np.array_equal(mask != 0, raw), f"{e['name']}: the raw mask differs from the reference's"
        pos = np.array(e["positions"])[:, :2]
        segs = np.array(e["segments"])
        for radius in g["radii"]:
            key = repr(radius)
            L = max(0, clearance.inflation_limit(radius, e["scale"]))
            assert L == ref.inflation_limit(radius, e["scale"])
            want = np.array([[c == "1" for c in row] for row in e["obstacle_map"][key]])
            grown = d2[0] <= L
            assert np.array_equal(grown, want), f"{e['name']} at radius {radius}: {int((grown != want).sum())} cells differ from the reference's obstacle_map"
            assert int(grown.sum()) == e["obstacle_pixels"][key]
            f = ref.Frame(min_x, min_y, min_x + max_x, min_y + max_y, e["scale"], max_d2=L, n_samples=1)
            hits = drv.query(d2[0], f, np.concatenate([pos, pos], 1))[:, 0] != 0
            want_hits = np.array([c == "1" for c in e["position_hits"][key]])
            assert np.array_equal(hits, want_hits), f"{e['name']} at radius {radius}: positions {np.nonzero(hits != want_hits)[0].tolist()} differ from check_collision_3d"
            for ns in sorted(set(int(v) for v in segs[:, 6])):
                sel = segs[:, 6] == ns
                got = drv.query(d2[0], f.but(n_samples=ns), segs[sel][:, [0, 1, 3, 4]])[:, 0] != 0
                want_s = np.array([c == "1" for c in e["segment_hits"][key]])[sel]
                assert np.array_equal(got, want_s), f"{e['name']} at radius {radius}, {ns} samples: segments {np.nonzero(got != want_s)[0].tolist()} differ from check_path_collision_3d"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def check_refusals(drv):
    """Every refusal of the header returns SGS_ERR_INVALID with a message that names the argument and leaves the poisoned outputs
    untouched; then the context still works."""
    nx, ny = 8, 4
    keep_s, s_ptr, _ = drv._put(np.zeros(2 * 2 * nx * ny + 16, np.uint32))
    keep_w, w_ptr, w_get = drv._bytes(4 * 2 * nx * ny + 64)
    keep_d, d_ptr, d_get = drv._bytes(4 * 2 * nx * ny + 64)
    keep_c, c_ptr, c_get = drv._bytes(32 + 64)
    keep_g, g_ptr, _ = drv._put(np.zeros(8, np.float64))
    keep_o, o_ptr, o_get = drv._bytes(16 + 64)

    def call(src=s_ptr, n=2, stride=nx * ny, work=w_ptr, d2=d_ptr, counts=c_ptr, null_params=False, **kw):
        return drv.call(src, n, stride, None if null_params else c_params(**{**dict(nx=nx, ny=ny), **kw}), work, d2, counts)

    T = ref.SRC_TOPDOWN
    bad = [(b"null src", dict(src=None)), (b"null params", dict(null_params=True)), (b"null work", dict(work=None)), (b"null d2", dict(d2=None)),
           (b"null out_counts", dict(counts=None)), (b"n_maps = 0", dict(n=0)), (b"n_maps = -2", dict(n=-2)), (b"nx = 0", dict(nx=0)), (b"ny = -1", dict(ny=-1)),
           (b"nx = 32769", dict(nx=32769, stride=2 ** 40)), (b"ny = 32769", dict(ny=32769, stride=2 ** 40)), (b"map_stride", dict(stride=nx * ny - 1)),
           (b"map_stride", dict(n=1, stride=0)), (b"map_stride", dict(source=T, min_hits=1, stride=2 * nx * ny - 1)), (b"unknown source", dict(source=2)),
           (b"unknown source", dict(source=-1)), (b"unknown flags", dict(source=T, min_hits=1, stride=2 * nx * ny, flags=2)),
           (b"unknown flags", dict(flags=1)), (b"min_hits = 0", dict(source=T, min_hits=0, stride=2 * nx * ny)), (b"reserved", dict(reserved=7)),
           (b"overlap", dict(work=d_ptr)), (b"overlap", dict(work=d_ptr + 4 * nx * ny)), (b"overlap", dict(d2=w_ptr + 4 * (2 * nx * ny - 1)))]
    for word, kw in bad:
        assert call(**kw) == -1, f"{word.decode()} with {kw} was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"sgs_clearance_map" in msg, (word, msg)

    def call_q(d2=d_ptr, qx=nx, qy=ny, segs=g_ptr, n=2, out=o_ptr, null_frame=False, **kw):
        return drv.call_query(d2, qx, qy, segs, n, None if null_frame else PLAIN.but(**kw), out)

    bad = [(b"null d2", dict(d2=None)), (b"null segs", dict(segs=None)), (b"null frame", dict(null_frame=True)), (b"null out", dict(out=None)), (b"n = 0", dict(n=0)),
           (b"n = -1", dict(n=-1)), (b"nx = 0", dict(qx=0)), (b"ny = 32769", dict(qy=32769)), (b"scale", dict(scale=0.0)), (b"scale", dict(scale=-0.05)),
           (b"scale", dict(scale=NAN)), (b"scale", dict(scale=INF)), (b"min", dict(min_x=NAN)), (b"min", dict(min_y=INF)), (b"sum", dict(sum_x=-INF)),
           (b"sum", dict(sum_y=NAN)), (b"margin = -1", dict(margin=-1)), (b"unknown flags", dict(flags=8)), (b"reserved", dict(reserved=1))]
    for word, kw in bad:
        assert call_q(**kw) == -1, f"{word.decode()} with {kw} was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"sgs_clearance_query" in msg, (word, msg)
    drv._sync()
    for get, what in ((w_get, "work"), (d_get, "d2"), (c_get, "out_counts"), (o_get, "out")):
        assert (np.array(get()) == SENTINEL).all(), f"a refused call wrote to {what}"
    assert call() == 0 and call(source=T, min_hits=1, flags=1, stride=2 * nx * ny) == 0       # the context still works
    assert call(work=d_ptr + 4 * nx * ny, d2=d_ptr, n=1) == 0                                  # work right behind d2 does not overlap it
    drv._sync()
    # the last call: one mask of zero bytes, no obstacle; behind it the second map of the call before: every cell unseen, all blocked
    assert np.array(c_get())[:32].view(np.uint32).tolist() == [0, 0, 0, nx * ny, nx * ny, 0, 0, 0]
    assert call_q() == 0
    drv._sync()
    assert np.array(o_get())[:16].view(np.uint32).tolist() == [1, NONE, 1, NONE]               # (0, 0) is four pixels left of the map


def check_misaligned(drv):
    """work, d2, out_counts and a seen map's src 1 and 2 bytes off their 4-byte alignment, the query's d2 and out likewise and its
    segs 4 bytes off their 8: each is refused with SGS_ERR_INVALID and a message that names the argument, before anything is
    enqueued — the poisoned outputs stay untouched.  A mask may begin at any byte."""
    nx, ny, pad = 8, 4, 16
    keep_s, s_ptr, _ = drv._put(np.zeros(2 * nx * ny + pad, np.uint32))
    keep_w, w_ptr, w_get = drv._bytes(4 * nx * ny + 4 * pad)
    keep_d, d_ptr, d_get = drv._bytes(4 * nx * ny + 4 * pad)
    keep_c, c_ptr, c_get = drv._bytes(16 + 4 * pad)
    keep_g, g_ptr, _ = drv._put(np.zeros(4 + pad, np.float64))
    keep_o, o_ptr, o_get = drv._bytes(8 + 4 * pad)
    keep_q, q_ptr, _ = drv._put(np.zeros(nx * ny + pad, np.uint32))
    assert all(v % 8 == 0 for v in (s_ptr, w_ptr, d_ptr, c_ptr, g_ptr, o_ptr, q_ptr))
    T = ref.SRC_TOPDOWN

    def call(src=0, work=0, d2=0, counts=0, source=T):
        p = c_params(nx, ny, source, 0, 1 if source == T else 0)
        return drv.call(s_ptr + src, 1, 2 * nx * ny, p, w_ptr + work, d_ptr + d2, c_ptr + counts)

    def call_q(d2=0, segs=0, out=0):
        return drv.call_query(q_ptr + d2, nx, ny, g_ptr + segs, 1, PLAIN, o_ptr + out)

    bad = [(call, word, {arg: off}) for word, arg in ((b"src", "src"), (b"work", "work"), (b"d2", "d2"), (b"out_counts", "counts")) for off in (1, 2)]
    bad += [(call_q, b"d2", dict(d2=1)), (call_q, b"d2", dict(d2=2)), (call_q, b"out", dict(out=1)), (call_q, b"out", dict(out=2)),
            (call_q, b"segs", dict(segs=4)), (call_q, b"segs", dict(segs=2))]
    for fn, word, kw in bad:
        assert fn(**kw) == -1, f"{word.decode()} off by {kw} bytes was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"aligned" in msg, (word, msg)
    drv._sync()
    for get, what in ((w_get, "work"), (d_get, "d2"), (c_get, "out_counts"), (o_get, "out")):
        assert (np.array(get()) == SENTINEL).all(), f"a refused call wrote to {what}"
    assert call() == 0 and call(src=4, work=4, d2=4, counts=4) == 0 and call(src=1, source=ref.SRC_MASK8) == 0 and call_q(d2=4, segs=8, out=4) == 0
    drv._sync()
    assert np.array(c_get())[:16].view(np.uint32).tolist() == [0, 0, 0, nx * ny]              # the mask of zero bytes: no obstacle


# ---- a real seen map ------------------------------------------------------------------------------------------------------------------------
def check_rendered_seen_map(drv, grid):
    """grid: uint32 [ny,nx,2] as sgs_topdown_map accumulated it from depth frames of scenes.make_room_mesh (topdown_cases.check_rendered
    returns it): its clearance against the restatement, with and without the unseen cells."""
    grid = np.asarray(grid, np.uint32)
    assert (grid[..., 1] > 0).sum() > 200
    check_seen_maps(drv, grid[None], "rendered seen map")
