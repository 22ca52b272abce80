"""The geodesic field's checks (sgs_geodesic_field, sgs_geodesic_path), shared by the CPU-emulator tests (test_emu_geodesic.py, its
mutants) and the GPU tests (test_gpu_geodesic.py): the pictures, a driver of the C ABI over plain buffers, and the assertions against
tests/geodesic_ref.py.  Every comparison is exact equality: there is no tolerance anywhere in this feature.  The field is the unique
fixed point of the relaxation (csrc/sgs_geodesic.h), so every schedule must give the same bits — the checks rely on it."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

import geodesic_ref as ref
from abi_driver import SENTINEL, AbiDriver, GpuBuffers

NONE = ref.NONE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geodesic_golden.json")


def c_params(nx, ny, source=ref.SRC_MASK8, max_d2=0, flags=0, reserved=0):
    from sage_gs import _capi
    return _capi.SgsGeodesicParams(int(nx), int(ny), int(source), int(max_d2), int(flags), int(reserved))


def tiles(T, nx, ny):
    return (nx + T - 1) // T, (ny + T - 1) // T


def default_rounds(T, nx, ny):
    tx, ty = tiles(T, nx, ny)
    return 2 * (tx + ty)


# ---- the C ABI over plain buffers -----------------------------------------------------------------------------------------------------
class AbiGeodesic(AbiDriver):
    """sgs_geodesic_field and sgs_geodesic_path over host buffers; a GPU driver overrides the buffer hooks (GpuGeodesic).  field_map
    and seeds are host arrays for both."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.T = int(self.lib.sgs_geodesic_tile())

    def call(self, src, n_maps, stride, params, field_map, n_fields, seeds, n_seeds, dist, state, rounds, status, stream=None):
        return int(self.lib.sgs_geodesic_field(self.ctx, src, int(n_maps), int(stride), None if params is None else C.byref(params), field_map, int(n_fields),
                                               seeds, int(n_seeds), dist, state, int(rounds), status, stream))

    def call_path(self, src, n_maps, stride, params, field_map, n_fields, dist, queries, n_queries, max_len, cells, info, stream=None):
        return int(self.lib.sgs_geodesic_path(self.ctx, src, int(n_maps), int(stride), None if params is None else C.byref(params), field_map, int(n_fields),
                                              dist, queries, int(n_queries), int(max_len), cells, info, stream))

    def _source(self, maps, source, stride):
        maps = np.asarray(maps)
        src = maps.astype(np.uint32) if source == ref.SRC_D2 else maps.astype(np.uint8)
        n, ny, nx = src.shape
        st = ny * nx if stride is None else int(stride)
        assert st >= ny * nx
        buf = np.full((n, st), 0 if source == ref.SRC_D2 else SENTINEL, src.dtype)      # the padding is blocked cells, if it were read
        buf[:, :ny * nx] = src.reshape(n, ny * nx)
        return self._put(buf) + (n, ny, nx, st)

    def field(self, maps, seeds, field_map=None, source=ref.SRC_MASK8, max_d2=0, rounds=None, stride=None, slack=64, max_calls=100000, first_only=False):
        """maps [n, ny, nx] (a mask, or d2 with source SRC_D2), seeds [(field, i, j)] -> (pairs uint32 [n_fields, ny, nx, 2], status
        uint32 [n_fields, 2], the calls made).  The first call runs `rounds` rounds (default 2 (tiles_x + tiles_y)); then the same
        number again with SGS_GEODESIC_CONTINUE until no tile is dirty (first_only: never).  dist, state and status hold 0xA5 bytes
        before the first call, each with `slack` bytes behind it that must stay so."""
        keep_s, s_ptr, _, n, ny, nx, st = self._source(maps, source, stride)
        fm = np.ascontiguousarray(np.arange(n) if field_map is None else field_map, np.int32)
        sd = np.ascontiguousarray(seeds, np.int32).reshape(-1, 3)
        nf = len(fm)
        words = int(self.lib.sgs_geodesic_state_words(nx, ny, nf))
        tx, ty = tiles(self.T, nx, ny)
        assert words == nf * (2 + tx * ty)
        rounds = default_rounds(self.T, nx, ny) if rounds is None else int(rounds)
        dist_bytes = 8 * nf * ny * nx
        keep_d, d_ptr, d_get = self._bytes(dist_bytes + slack)
        keep_w, w_ptr, w_get = self._bytes(4 * words + slack)
        keep_t, t_ptr, t_get = self._bytes(8 * nf + slack)
        calls = 0
        while True:
            p = c_params(nx, ny, source, max_d2, ref.CONTINUE if calls else 0)
            self.lib.check(self.call(s_ptr, n, st, p, fm.ctypes.data, nf, sd.ctypes.data, len(sd), d_ptr, w_ptr, rounds, t_ptr), self.ctx)
            self._sync()
            calls += 1
            status = np.array(t_get())[:8 * nf].view(np.uint32).reshape(nf, 2).copy()
            if first_only or not status[:, 0].any():
                break
            assert calls < max_calls and calls * rounds <= nx * ny + rounds, f"the field of {nx}x{ny} does not converge: {int(status[:, 0].sum())} tiles are dirty after {calls * rounds} rounds"
        db = np.array(d_get())
        assert (db[dist_bytes:] == SENTINEL).all(), "bytes were written behind dist"
        assert (np.array(w_get())[4 * words:] == SENTINEL).all(), "bytes were written behind state"
        assert (np.array(t_get())[8 * nf:] == SENTINEL).all(), "bytes were written behind status"
        return db[:dist_bytes].view(np.uint32).reshape(nf, ny, nx, 2).copy(), status, calls

    def paths(self, maps, dist, queries, max_len, field_map=None, source=ref.SRC_MASK8, max_d2=0, stride=None, slack=64):
        """queries [(field, i, j)] -> (cells int32 [n, max_len, 2], info uint32 [n, 2]); the cells never written read -1515870811 (0xA5)."""
        keep_s, s_ptr, _, n, ny, nx, st = self._source(maps, source, stride)
        fm = np.ascontiguousarray(np.arange(n) if field_map is None else field_map, np.int32)
        q = np.ascontiguousarray(queries, np.int32).reshape(-1, 3)
        keep_d, d_ptr, _ = self._put(np.ascontiguousarray(dist, np.uint32))
        keep_q, q_ptr, _ = self._put(q)
        cell_bytes = 8 * len(q) * max_len
        keep_c, c_ptr, c_get = self._bytes(cell_bytes + slack)
        keep_i, i_ptr, i_get = self._bytes(8 * len(q) + slack)
        self.lib.check(self.call_path(s_ptr, n, st, c_params(nx, ny, source, max_d2), fm.ctypes.data, len(fm), d_ptr, q_ptr, len(q), max_len, c_ptr, i_ptr), self.ctx)
        self._sync()
        cb, ib = np.array(c_get()), np.array(i_get())
        assert (cb[cell_bytes:] == SENTINEL).all(), "bytes were written behind out_cells"
        assert (ib[8 * len(q):] == SENTINEL).all(), "bytes were written behind out_info"
        return cb[:cell_bytes].view(np.int32).reshape(len(q), max_len, 2).copy(), ib[:8 * len(q)].view(np.uint32).reshape(len(q), 2).copy()


class GpuGeodesic(GpuBuffers, AbiGeodesic):
    """AbiGeodesic over torch device buffers, on a Renderer's context."""


# ---- pictures: (blocked bool [ny, nx], seeds [(i, j)]) -----------------------------------------------------------------------------------
def sizes(T):
    """nx x ny: one cell, a row, a column, and widths either side of one and two tiles by heights from 3 to T + 2; one of 3T+1 x 2T+1."""
    return ((1, 1), (1, 7), (7, 1), (T - 1, 3), (T, 5), (T + 1, T + 2), (2 * T + 1, T + 2), (3 * T + 1, 2 * T + 1))


def size_pictures(nx, ny, T):
    rs = np.random.RandomState(1000 * nx + ny)
    pics = {"empty_room_corner_seed": (np.zeros((ny, nx), bool), [(nx - 1, ny - 1)]),
            "all_blocked": (np.ones((ny, nx), bool), [(0, 0)])}
    ob = rs.rand(ny, nx) < 0.28
    free = np.argwhere(~ob)
    if len(free):
        picks = free[rs.choice(len(free), min(len(free), 5), replace=False)]
        pics["random_seeds_in_several_tiles"] = (ob, [(int(i), int(j)) for j, i in picks] + [(0, 0), (nx - 1, 0)])
    return pics


def serpentine(T):
    """A corridor one cell wide in a grid of 2T x 2T+1 that crosses the tile boundary x = T once per corridor row: rows 0, 2, 4, ...
    are free for x in T-3 .. T+2, and the wall rows between them are open at alternating ends.  Seed at its top-left end."""
    nx, ny = 2 * T, 2 * T + 1
    ob = np.ones((ny, nx), bool)
    lo, hi = T - 3, T + 2
    for k, j in enumerate(range(0, ny, 2)):
        ob[j, lo:hi + 1] = False
        if j + 1 < ny:
            ob[j + 1, hi if k % 2 == 0 else lo] = False
    return ob, [(lo, 0)]


def diagonal_corridor(T):
    """Free cells (k, k) alone, k = T-6 .. T+5, in a grid of 2T x 2T: the walk passes (T-1, T-1) -> (T, T) through the corner four tiles
    share, with (T-1, T) and (T, T-1) blocked; the seed lies in the last tile."""
    ob = np.ones((2 * T, 2 * T), bool)
    for k in range(T - 6, T + 6):
        ob[k, k] = False
    return ob, [(T + 5, T + 5)]


def sealed_region(T):
    """A room of T+9 x T+3 with a closed closet: the cells inside are free and unreachable; a seed on a blocked cell beside a real one."""
    nx, ny = T + 9, T + 3
    ob = np.zeros((ny, nx), bool)
    ob[4:12, T - 4:T + 5] = True
    ob[5:11, T - 3:T + 4] = False
    return ob, [(1, 1), (T - 4, 4)]


def edge_wall(T):
    """A grid of T+3 x T+4 (partial last tiles): a wall in column T+1 and one in row T+2, each running into the grid's edge and open only
    far from it: were the cells beyond the edge free, a walk would go round the wall's end outside the grid."""
    nx, ny = T + 3, T + 4
    ob = np.zeros((ny, nx), bool)
    ob[2:, T + 1] = True
    ob[T + 2, 2:T + 1] = True
    return ob, [(nx - 1, ny - 1)]


def edge_column(T):
    """A grid of 2T+1 x T+5 whose only free cells are its last column, a tile column one cell wide: every cell of those tiles is a
    border cell, and the tile below the seed's hears of it from the seed's tile alone."""
    ob = np.ones((T + 5, 2 * T + 1), bool)
    ob[:, 2 * T] = False
    return ob, [(2 * T, 0)]


def pictures(T):
    return {"edge_column": edge_column(T), "serpentine": serpentine(T), "diagonal_corridor": diagonal_corridor(T), "sealed_region": sealed_region(T), "edge_wall": edge_wall(T)}


_REF = {}


def want_field(ob, seeds):
    """ref.field, computed once per picture."""
    key = (ob.shape, ob.tobytes(), tuple(map(tuple, seeds)))
    if key not in _REF:
        _REF[key] = ref.field(ob, seeds)
    return _REF[key]


def check_field(name, got, ob, seeds):
    want = want_field(ob, seeds)
    if not np.array_equal(got, want):
        j, i = (int(v[0]) for v in np.nonzero((got != want).any(-1)))
        raise AssertionError(f"{name}: cell ({i}, {j}) is {tuple(int(v) for v in got[j, i])}, the restatement has {tuple(int(v) for v in want[j, i])}")


def check_pictures(drv, pics, label="", **kw):
    for name, (ob, seeds) in pics.items():
        dist, status, _ = drv.field(ob[None], [(0, i, j) for i, j in seeds], **kw)
        check_field(f"{label}{name} {ob.shape[1]}x{ob.shape[0]}", dist[0], ob, seeds)
        n_blocked = sum(bool(ob[j, i]) for i, j in seeds)
        assert status[0].tolist() == [0, n_blocked], f"{label}{name}: status {status[0].tolist()}, {n_blocked} seeds are blocked"


def check_sizes(drv, which=None):
    for nx, ny in (sizes(drv.T) if which is None else which):
        check_pictures(drv, size_pictures(nx, ny, drv.T), f"{nx}x{ny} ")


def check_picture_properties(T):
    ob, seeds = serpentine(T)
    f = want_field(ob, seeds)
    assert (f[~ob][:, 0] != NONE).all() and int(f[..., 0][~ob].max() + f[..., 1][~ob].max()) > 5 * T      # one corridor, all of it reached
    ob, seeds = diagonal_corridor(T)
    assert ob[T, T - 1] and ob[T - 1, T] and want_field(ob, seeds)[T - 6, T - 6].tolist() == [0, 11]
    ob, seeds = sealed_region(T)
    f = want_field(ob, seeds)
    assert not ob[7, T] and f[7, T].tolist() == [NONE, NONE] and ob[4, T - 4] and f[0, 0].tolist() == [0, 1]
    ob, seeds = edge_wall(T)
    f = want_field(ob, seeds)
    assert f[T + 3, T].tolist()[0] + f[T + 3, T].tolist()[1] > T                    # the cell beside the seed's pocket is a long way round


# ---- the serpentine: CONTINUE, and the schedule ---------------------------------------------------------------------------------------------
def check_serpentine_needs_continue(drv):
    ob, seeds = serpentine(drv.T)
    sd = [(0, i, j) for i, j in seeds]
    dist, status, _ = drv.field(ob[None], sd, first_only=True)
    assert status[0, 0] > 0, f"serpentine: final after the first call of {default_rounds(drv.T, ob.shape[1], ob.shape[0])} rounds: the case proves nothing"
    assert not np.array_equal(dist[0], want_field(ob, seeds))
    dist, status, calls = drv.field(ob[None], sd)
    assert calls > 1 and status[0].tolist() == [0, 0]
    check_field("serpentine", dist[0], ob, seeds)


def check_schedule_independence(drv):
    """rounds = 1 repeated under CONTINUE, the default, and one call of many rounds: bit-identical; a field alone equals the same field
    inside a batch."""
    T = drv.T
    ob, seeds = serpentine(T)
    sd = [(0, i, j) for i, j in seeds]
    one, _, calls_one = drv.field(ob[None], sd, rounds=1)
    dflt, _, _ = drv.field(ob[None], sd)
    big, status, calls_big = drv.field(ob[None], sd, rounds=4 * T)
    assert calls_big == 1 and calls_one > default_rounds(T, ob.shape[1], ob.shape[0]) and status[0, 0] == 0, (calls_big, calls_one)
    check_field("serpentine, one call", big[0], ob, seeds)
    assert np.array_equal(one, big), "the field depends on the rounds per call (rounds = 1)"
    assert np.array_equal(dflt, big), "the field depends on the rounds per call (default)"
    ob2 = size_pictures(2 * T + 1, T + 2, T)["random_seeds_in_several_tiles"][0]
    free = np.argwhere(~ob2)
    goals = [(int(i), int(j)) for j, i in free[:: max(1, len(free) // 4)][:4]]
    alone = [drv.field(ob2[None], [(0,) + g])[0][0] for g in goals]
    batch, status, _ = drv.field(ob2[None], [(f,) + g for f, g in enumerate(goals)], field_map=[0] * len(goals))
    for f, g in enumerate(goals):
        check_field(f"batch field {f}", batch[f], ob2, [g])
        assert np.array_equal(batch[f], alone[f]), f"field {f} depends on the batch"


# ---- batches, sources ------------------------------------------------------------------------------------------------------------------------
def check_batches(drv):
    """Three different maps with a padded, poisoned stride; five fields on them through a field_map that is not the identity; one
    field with two seeds, one with a blocked seed."""
    T = drv.T
    nx, ny = T + 5, T + 2
    rs = np.random.RandomState(7)
    maps = rs.rand(3, ny, nx) < np.array([0.1, 0.3, 0.2])[:, None, None]
    maps[:, 0, 0] = False
    maps[:, ny - 1, nx - 1] = False
    maps[1, 3, 3] = True
    fm = [2, 0, 1, 1, 2]
    seeds = [(0, 0, 0), (1, nx - 1, ny - 1), (2, 0, 0), (2, nx - 1, ny - 1), (3, 3, 3), (3, 0, 0), (4, nx - 1, ny - 1)]
    dist, status, _ = drv.field(maps, seeds, field_map=fm, stride=nx * ny + 37)
    for f, m in enumerate(fm):
        mine = [(i, j) for ff, i, j in seeds if ff == f]
        check_field(f"batch field {f} on map {m}", dist[f], maps[m], mine)
    assert status[:, 0].tolist() == [0] * 5 and status[:, 1].tolist() == [0, 0, 0, 1, 0], status.tolist()
    assert len({dist[f].tobytes() for f in range(5)}) == 5


def check_sources(drv):
    """A d2 map as the source: blocked iff d2 <= max_d2, at max_d2 = a value the map holds, one below and one above; equal to the mask
    of the same cells."""
    T = drv.T
    nx, ny = T + 3, 9
    rs = np.random.RandomState(3)
    d2 = rs.randint(0, 6, (ny, nx)).astype(np.uint32)
    d2[0, 0] = 5
    d2[ny - 1, nx - 1] = NONE
    seen = set()
    for max_d2 in (0, 1, 2):
        ob = ref.blocked_of(d2, ref.SRC_D2, max_d2)
        assert (d2 == max_d2).any() and (d2 == max_d2 + 1).any()
        seeds = [(0, 0), (nx - 1, ny - 1)]
        dist, status, _ = drv.field(d2[None], [(0,) + s for s in seeds], source=ref.SRC_D2, max_d2=max_d2)
        check_field(f"d2 source, max_d2 = {max_d2}", dist[0], ob, seeds)
        as_mask, _, _ = drv.field(ob[None], [(0,) + s for s in seeds])
        assert np.array_equal(as_mask, dist)
        seen.add(dist.tobytes())
    assert len(seen) == 3


# ---- paths -----------------------------------------------------------------------------------------------------------------------------------
def check_path_properties(name, ob, fld, query, cells, info, max_len, seeds):
    i, j = query
    want, want_status = ref.path(ob, fld, (i, j), max_len)
    n, status = int(info[0]), int(info[1])
    got = [tuple(int(v) for v in c) for c in cells[:n]]
    assert status == want_status, f"{name}: query {query} has status {status}, the restatement {want_status}"
    assert got == want, f"{name}: query {query} walks {got[:6]}..., the restatement {want[:6]}... ({n} and {len(want)} cells)"
    assert (cells[n:] == np.int32(-1515870811)).all(), f"{name}: query {query}: cells were written beyond the {n} counted"
    if status == ref.PATH_UNREACHABLE:
        assert n == 0 and (ob[j, i] or fld[j, i, 0] == NONE)
        return
    assert got[0] == (i, j) and all(not ob[y, x] for x, y in got)
    a, b = ref.count_steps(got)                                                     # (asserts the cells are 8-neighbours)
    if status == ref.PATH_OK:
        assert got[-1] in set(seeds) and (a, b) == tuple(int(v) for v in fld[j, i]) and n == a + b + 1, f"{name}: query {query}: {(a, b)} steps, the field has {fld[j, i].tolist()}"
    else:
        assert status == ref.PATH_TRUNCATED and n == max_len and int(fld[j, i, 0]) + int(fld[j, i, 1]) + 1 > max_len


def check_paths(drv):
    """Every cell of the sealed room and of the diagonal corridor as a start (free, blocked and unreachable ones), and seeded starts of
    a random map with two fields, at a max_len that truncates some: every property on every query."""
    T = drv.T
    for name, (ob, seeds) in (("sealed_region", sealed_region(T)), ("diagonal_corridor", diagonal_corridor(T)), ("serpentine", serpentine(T))):
        ny, nx = ob.shape
        fld = want_field(ob, seeds)
        dist, _, _ = drv.field(ob[None], [(0, i, j) for i, j in seeds], rounds=8 * T)
        check_field(name, dist[0], ob, seeds)
        step = 1 if name != "serpentine" else 7
        queries = [(0, i, j) for j in range(ny) for i in range(nx)][::step]
        seen = set()
        for max_len in (nx + ny, 4):
            cells, info = drv.paths(ob[None], dist, queries, max_len)
            seen |= set(info[:, 1].tolist())
            for q, c, n in zip(queries, cells, info):
                check_path_properties(f"{name}, max_len = {max_len}", ob, fld, q[1:], c, n, max_len, seeds)
        assert seen == {ref.PATH_OK, ref.PATH_UNREACHABLE, ref.PATH_TRUNCATED}, (name, seen)
    # two fields on one map, and a query that names no field or no cell
    ob, seeds = sealed_region(T)
    other = [(ob.shape[1] - 1, ob.shape[0] - 1)]
    dist, _, _ = drv.field(ob[None], [(0,) + seeds[0], (1,) + other[0]], field_map=[0, 0])
    queries = [(0, 5, 2), (1, 5, 2), (2, 5, 2), (0, -1, 2), (1, 5, ob.shape[0]), (-1, 0, 0)]
    cells, info = drv.paths(ob[None], dist, queries, 3 * T, field_map=[0, 0])
    assert info[:, 1].tolist() == [0, 0, 3, 3, 3, 3] and info[2:, 0].tolist() == [0] * 4
    check_path_properties("two fields, field 0", ob, want_field(ob, seeds[:1]), (5, 2), cells[0], info[0], 3 * T, seeds[:1])
    check_path_properties("two fields, field 1", ob, want_field(ob, other), (5, 2), cells[1], info[1], 3 * T, other)


# ---- the reference's own answers ------------------------------------------------------------------------------------------------------------
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def golden_grid(e):
    return np.array([[c == "1" for c in row] for row in e["grid"]])


def decode_path(start, digits):
    cells = [tuple(start)]
    for c in digits:
        di, dj = ref.DIRS[int(c)]
        cells.append((cells[-1][0] + di, cells[-1][1] + dj))
    return cells


def check_golden_trajectories(points_of):
    """points_of(path, scale, min_x, min_y, fixed_z, sample_step) -> [{"position", "rotation"}]: equal to the reference's recorded
    points as float64, bit for bit.  Returns the largest difference seen (0.0 when all are equal), for a report."""
    worst, n = 0.0, 0
    for e in golden()["grids"]:
        for t in e["trajectories"]:
            got = points_of(decode_path(t["start"], t["path"]), e["scale"], e["min_x"], e["min_y"], t["fixed_z"], t["sample_step"])
            assert len(got) == len(t["points"]) > 1
            for g, w in zip(got, t["points"]):
                n += 1
                worst = max(worst, float(np.abs(np.array(g["position"] + g["rotation"]) - np.array(w["position"] + w["rotation"])).max()))
    assert n > 100 and worst == 0.0, f"trajectory points differ from the reference's by up to {worst}"


def check_golden(drv=None, field_of=None, path_of=None):
    """For every recorded (start, goal) pair, none left out: the (a, b) of the reference's path is the field's pair at the start, null
    exactly where the field is NONE (the start free), and our own path has the same pair.  field_of(ob, goal) -> pairs [ny, nx, 2],
    path_of(ob, fld, goal, starts) -> [cells or None]; by default through the driver."""
    n_pairs = n_null = 0
    for e in golden()["grids"]:
        ob = golden_grid(e)
        for g in e["goals"]:
            goal = tuple(g["goal"])
            fld = field_of(ob, goal) if field_of else drv.field(ob[None], [(0,) + goal])[0][0]
            check_field(f"golden {e['name']} goal {goal}", fld, ob, [goal])
            starts = [tuple(p["start"]) for p in g["pairs"]]
            if path_of:
                ours = path_of(ob, fld, goal, starts)
            else:
                cells, info = drv.paths(ob[None], fld[None], [(0,) + s for s in starts], ob.size)
                ours = [[tuple(int(v) for v in c) for c in cs[:int(n[0])]] if n[1] == 0 else None for cs, n in zip(cells, info)]
            for p, s, mine in zip(g["pairs"], starts, ours):
                n_pairs += 1
                assert not ob[s[1], s[0]], "the golden file holds a blocked start"
                pair = tuple(int(v) for v in fld[s[1], s[0]])
                if p["path"] is None:
                    n_null += 1
                    assert pair == (NONE, NONE) and mine is None, f"golden {e['name']} {s} -> {goal}: the reference found no path, the field has {pair}"
                    continue
                theirs = decode_path(s, p["path"])
                assert theirs[0] == s and theirs[-1] == goal
                assert ref.count_steps(theirs) == pair, f"golden {e['name']} {s} -> {goal}: the reference's path has {ref.count_steps(theirs)}, the field {pair}"
                assert mine is not None and mine[0] == s and mine[-1] == goal and ref.count_steps(mine) == pair, f"golden {e['name']} {s} -> {goal}: our path"
    assert n_pairs > 1000 and n_null > 20, (n_pairs, n_null)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def check_refusals(drv):
    """Every refusal of the header returns SGS_ERR_INVALID with a message that names the argument and leaves the poisoned outputs
    untouched; then the context still works."""
    nx, ny, nf = 8, 4, 2
    keep_s, s_ptr, _ = drv._put(np.zeros(2 * nx * ny + 16, np.uint32))
    words = int(drv.lib.sgs_geodesic_state_words(nx, ny, nf))
    keep_d, d_ptr, d_get = drv._bytes(8 * nf * nx * ny + 64)
    keep_w, w_ptr, w_get = drv._bytes(4 * words + 64)
    keep_t, t_ptr, t_get = drv._bytes(8 * nf + 64)
    keep_q, q_ptr, _ = drv._put(np.array([[0, 1, 1], [1, 2, 2]], np.int32))
    keep_c, c_ptr, c_get = drv._bytes(8 * 2 * 16 + 64)
    keep_i, i_ptr, i_get = drv._bytes(16 + 64)
    fm_ok, sd_ok = np.array([0, 1], np.int32), np.array([[0, 1, 1], [1, 2, 2]], np.int32)

    def call(src=s_ptr, n=2, stride=nx * ny, fm=fm_ok, n_fields=nf, seeds=sd_ok, n_seeds=2, dist=d_ptr, state=w_ptr, rounds=1, status=t_ptr, null_params=False, **kw):
        fm = None if fm is None else np.ascontiguousarray(fm, np.int32)
        seeds = None if seeds is None else np.ascontiguousarray(seeds, np.int32)
        return drv.call(src, n, stride, None if null_params else c_params(**{**dict(nx=nx, ny=ny), **kw}), None if fm is None else fm.ctypes.data, n_fields,
                        None if seeds is None else seeds.ctypes.data, n_seeds, dist, state, rounds, status)

    D = ref.SRC_D2
    bad = [(b"null src", dict(src=None)), (b"null params", dict(null_params=True)), (b"null field_map", dict(fm=None)), (b"null seeds", dict(seeds=None)),
           (b"null dist", dict(dist=None)), (b"null state", dict(state=None)), (b"null status", dict(status=None)), (b"n_maps = 0", dict(n=0)),
           (b"n_fields = 0", dict(n_fields=0)), (b"n_fields = 65536", dict(n_fields=65536)), (b"n_seeds = 0", dict(n_seeds=0)), (b"n_seeds = -1", dict(n_seeds=-1)),
           (b"rounds = 0", dict(rounds=0)), (b"rounds = -3", dict(rounds=-3)), (b"nx = 0", dict(nx=0)), (b"ny = 4097", dict(ny=4097, stride=2 ** 40)),
           (b"nx = 4097", dict(nx=4097, stride=2 ** 40)), (b"field_map[1] = 2", dict(fm=[0, 2])), (b"field_map[0] = -1", dict(fm=[-1, 0])),
           (b"seeds[1] names field 2", dict(seeds=[[0, 1, 1], [2, 1, 1]])), (b"seeds[0] names field -1", dict(seeds=[[-1, 1, 1], [0, 1, 1]])),
           (b"seeds[0] = (8, 1) is outside", dict(seeds=[[0, 8, 1], [0, 1, 1]])), (b"seeds[1] = (1, 4) is outside", dict(seeds=[[0, 1, 1], [1, 1, 4]])),
           (b"seeds[0] = (-1, 0) is outside", dict(seeds=[[0, -1, 0], [0, 1, 1]])), (b"seeds[0] = (0, -1) is outside", dict(seeds=[[0, 0, -1], [0, 1, 1]])),
           (b"map_stride", dict(stride=nx * ny - 1)), (b"map_stride", dict(n=1, fm=[0, 0], stride=0)), (b"unknown source", dict(source=2)),
           (b"unknown source", dict(source=-1)), (b"unknown flags", dict(flags=2)), (b"unknown flags", dict(flags=0x80000001)), (b"reserved", dict(reserved=7)),
           (b"dist", dict(dist=d_ptr + 4)), (b"state", dict(state=w_ptr + 2)), (b"status", dict(status=t_ptr + 1)), (b"src", dict(src=s_ptr + 2, source=D)),
           (b"overlap", dict(state=d_ptr)), (b"overlap", dict(state=d_ptr + 8 * nf * nx * ny - 4)), (b"overlap", dict(dist=w_ptr + 4 * words - 8))]
    for word, kw in bad:
        assert call(**kw) == -1, f"{word.decode()} with {kw} was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"sgs_geodesic_field" in msg, (word, msg)

    def call_p(src=s_ptr, n=2, stride=nx * ny, fm=fm_ok, n_fields=nf, dist=d_ptr, queries=q_ptr, n_queries=2, max_len=16, cells=c_ptr, info=i_ptr, null_params=False, **kw):
        fm = None if fm is None else np.ascontiguousarray(fm, np.int32)
        return drv.call_path(src, n, stride, None if null_params else c_params(**{**dict(nx=nx, ny=ny), **kw}), None if fm is None else fm.ctypes.data, n_fields,
                             dist, queries, n_queries, max_len, cells, info)

    bad = [(b"null src", dict(src=None)), (b"null params", dict(null_params=True)), (b"null field_map", dict(fm=None)), (b"null dist", dict(dist=None)),
           (b"null queries", dict(queries=None)), (b"null out_cells", dict(cells=None)), (b"null out_info", dict(info=None)), (b"n_maps = 0", dict(n=0)),
           (b"n_fields = 0", dict(n_fields=0)), (b"n_fields = 513", dict(n_fields=513)), (b"n_queries = 0", dict(n_queries=0)), (b"max_len = 0", dict(max_len=0)),
           (b"nx = 0", dict(nx=0)), (b"field_map[1] = 2", dict(fm=[0, 2])), (b"map_stride", dict(stride=nx * ny - 1)), (b"unknown source", dict(source=3)),
           (b"unknown flags", dict(flags=1)), (b"unknown flags", dict(flags=4)), (b"reserved", dict(reserved=-1)), (b"dist", dict(dist=d_ptr + 4)),
           (b"queries", dict(queries=q_ptr + 2)), (b"out_cells", dict(cells=c_ptr + 1)), (b"out_info", dict(info=i_ptr + 2)), (b"src", dict(src=s_ptr + 1, source=D))]
    for word, kw in bad:
        assert call_p(**kw) == -1, f"{word.decode()} with {kw} was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"sgs_geodesic_path" in msg, (word, msg)
    drv._sync()
    for get, what in ((d_get, "dist"), (w_get, "state"), (t_get, "status"), (c_get, "out_cells"), (i_get, "out_info")):
        assert (np.array(get()) == SENTINEL).all(), f"a refused call wrote to {what}"
    assert call() == 0 and call(flags=ref.CONTINUE) == 0 and call_p() == 0             # the context still works; state right behind dist is fine
    assert call(src=s_ptr + 1, state=d_ptr + 8 * nf * nx * ny, dist=d_ptr) == 0
    drv._sync()
    assert np.array(t_get())[:16].view(np.uint32).tolist() == [0, 0, 0, 0]
    assert np.array(i_get())[:16].view(np.uint32).tolist() == [1, 0, 1, 0]             # (a free map: each query starts on its field's seed)
    assert drv.lib.sgs_geodesic_state_words(0, 4, 1) == -1 and drv.lib.sgs_geodesic_state_words(4, 4097, 1) == -1 and drv.lib.sgs_geodesic_state_words(4, 4, 0) == -1
