"""The checks of the item endpoints (sgs_endpoints), shared by the CPU-emulator tests (test_emu_endpoints.py, its mutants) and the GPU
tests (test_gpu_endpoints.py): scenes, a driver of the C ABI over plain buffers, and the assertions against tests/endpoints_ref.py
and tests/golden/endpoints_golden.json.  Every comparison is exact equality: every field of every item row, answer and counter is an
integer that depends on the map, the items, the queries and the params alone.  Grids and windows come from E = (1, 2, T - 1, T, T + 1,
2T + 2) with T = sgs_endpoints_tile() = 64, the cells of one ballot word; only the 2^19-entry limit needs more (a 4096 x 2 grid)."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

import endpoints_ref as ref
from abi_driver import SENTINEL, AbiDriver, GpuBuffers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "endpoints_golden.json")
T = ref.QUERY_TOWARDS


def c_params(nx, ny, source=ref.SRC_MASK8, max_d2=0, max_dist=50, flags=0, reserved=0):
    from sage_gs import _capi
    return _capi.SgsEndpointsParams(int(nx), int(ny), int(source), int(max_d2), int(max_dist), int(flags), int(reserved))


def csr(items):
    """(uint32 offsets [n + 1], int32 cells) of a list of index lists."""
    lens = [len(c) for c in items]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cells = np.concatenate([np.asarray(c, np.int64).reshape(-1) for c in items] + [np.zeros(0, np.int64)]).astype(np.int32)
    return offsets, cells


def as_queries(queries):
    q = np.zeros(len(queries), ref.QUERY_DTYPE)
    for k, (item, tx, ty, flags) in enumerate(queries):
        q[k] = (item, tx, ty, flags)
    return q


# ---- the C ABI over plain buffers -----------------------------------------------------------------------------------------------------
class AbiEndpoints(AbiDriver):
    """sgs_endpoints over host buffers; a GPU driver overrides the buffer hooks (GpuEndpoints)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.T = int(self.lib.sgs_endpoints_tile())

    def call(self, src, params, offsets, cells, n_items, queries, n_queries, work, work_bytes, items, answers, counts, stream=None):
        return int(self.lib.sgs_endpoints(self.ctx, src, None if params is None else C.byref(params), offsets, cells, int(n_items), queries, int(n_queries),
                                          work, int(work_bytes), items, answers, counts, stream))

    def run(self, src, items, queries, max_dist=50, source=ref.SRC_MASK8, max_d2=0, work_bytes=None, slack=64):
        """src [ny, nx] (bytes, or d2 words with SRC_D2), items a list of index lists, queries rows of (item, tx, ty, flags) ->
        (rows ITEM_DTYPE [n_items], answers ANSWER_DTYPE [n_queries], counts [4] ints).  work (work_bytes of it: by default what the
        restatement says this call needs), rows, answers and counters hold 0xA5 bytes before the call, each with `slack` bytes behind
        it that must stay so."""
        src = np.asarray(src)
        src = src.astype(np.uint32) if source == ref.SRC_D2 else src.astype(np.uint8)
        ny, nx = src.shape
        offsets, cells = csr(items)
        n_items, n_q = len(items), len(queries)
        bound = int(self.lib.sgs_endpoints_work_bytes(nx, ny, n_items))
        assert bound == 8 * n_items + ((n_items * nx * ny + 7) & ~7), bound
        if work_bytes is None:
            work_bytes = ref.work_needed([ref.item_row(c, nx, ny) for c in items], nx, ny, max_dist)
            assert work_bytes <= bound
        keep_s, s_ptr, _ = self._put(src)
        keep_o, o_ptr, _ = self._put(offsets)
        keep_c, c_ptr, _ = self._put(cells, slack=4)
        keep_q, q_ptr, _ = self._put(as_queries(queries), slack=4)
        keep_w, w_ptr, w_get = self._bytes(work_bytes + slack)
        keep_i, i_ptr, i_get = self._bytes(56 * n_items + slack)
        keep_a, a_ptr, a_get = self._bytes(16 * n_q + slack)
        keep_n, n_ptr, n_get = self._bytes(32 + slack)
        assert w_ptr % 8 == 0 and i_ptr % 8 == 0 and n_ptr % 8 == 0
        self.lib.check(self.call(s_ptr, c_params(nx, ny, source, max_d2, max_dist), o_ptr, c_ptr, n_items, q_ptr, n_q, w_ptr, work_bytes, i_ptr, a_ptr, n_ptr), self.ctx)
        self._sync()
        ib, ab, nb = np.array(i_get()), np.array(a_get()), np.array(n_get())
        assert (np.array(w_get())[work_bytes:] == SENTINEL).all(), "bytes were written behind work"
        assert (ib[56 * n_items:] == SENTINEL).all(), "bytes were written behind out_items"
        assert (ab[16 * n_q:] == SENTINEL).all(), "bytes were written behind out_queries"
        assert (nb[32:] == SENTINEL).all(), "bytes were written behind out_counts"
        return (ib[:56 * n_items].view(ref.ITEM_DTYPE).copy(), ab[:16 * n_q].view(ref.ANSWER_DTYPE).copy(), [int(v) for v in nb[:32].view(np.uint64)])


class GpuEndpoints(GpuBuffers, AbiEndpoints):
    """AbiEndpoints over torch device buffers, on a Renderer's context."""


# ---- one call against the restatement ---------------------------------------------------------------------------------------------------
def check_call(name, got, src, items, queries, max_dist=50, source=ref.SRC_MASK8, max_d2=0, want=None):
    """Every field of every item row, then of every answer, then the counters, each on its own assertion."""
    rows, answers, counts = got
    w_rows, w_answers, w_counts, _ = ref.endpoints(src, items, queries, max_dist, source, max_d2) if want is None else want
    for field in ref.ITEM_DTYPE.names:
        bad = np.nonzero(rows[field] != w_rows[field])[0]
        assert len(bad) == 0, f"{name}: item {int(bad[0])} has {field} = {int(rows[field][bad[0]])}, the restatement has {int(w_rows[field][bad[0]])}"
    for field in ref.ANSWER_DTYPE.names:
        bad = np.nonzero(answers[field] != w_answers[field])[0]
        assert len(bad) == 0, (f"{name}: query {int(bad[0])} {tuple(queries[bad[0]])} has {field} = {int(answers[field][bad[0]])}, "
                               f"the restatement has {int(w_answers[field][bad[0]])}")
    assert counts == w_counts, f"{name}: counters {counts}, the restatement has {w_counts}"


def run_and_check(drv, name, src, items, queries, **kw):
    got = drv.run(src, items, queries, **kw)
    check_call(name, got, src, items, queries, **kw)
    return got


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def rect(nx, x0, y0, x1, y1):
    """The raster indices of the rectangle [x0, x1) x [y0, y1), row by row."""
    ys, xs = np.mgrid[y0:y1, x0:x1]
    return (ys * nx + xs).reshape(-1)


def ring(nx, x0, y0, x1, y1, t=1):
    """A rectangle without its middle: it has an inner boundary."""
    ys, xs = np.mgrid[y0:y1, x0:x1]
    edge = (ys < y0 + t) | (ys >= y1 - t) | (xs < x0 + t) | (xs >= x1 - t)
    return (ys * nx + xs)[edge]


def edge_sizes(t):
    return (1, 2, t - 1, t, t + 1, 2 * t + 2)


def size_scene(nx, ny, seed):
    """A seeded scene on an nx x ny grid: obstacles at density 0.3 .. 0.7, a blob of cells with duplicates, a rectangle against the right
    and lower edge, a one-cell item at the origin and the last cell, and queries without a target, towards seeded cells and towards
    each corner."""
    rs = np.random.RandomState(seed)
    mask = (rs.rand(ny, nx) < rs.uniform(0.3, 0.7)).astype(np.uint8)
    blob = rs.randint(0, nx * ny, max(1, nx * ny // 9))
    blob = np.concatenate([blob, blob[:len(blob) // 2]])
    items = [blob, rect(nx, nx - max(1, nx // 3), ny - max(1, ny // 4), nx, ny), [0], [nx * ny - 1]]
    queries = []
    for k in range(len(items)):
        queries += [(k, 0, 0, 0), (k, 0, 0, T), (k, nx - 1, 0, T), (k, 0, ny - 1, T), (k, nx - 1, ny - 1, T)]
        queries += [(k, int(rs.randint(nx)), int(rs.randint(ny)), T) for _ in range(3)]
    return mask, items, queries


def check_sizes(drv, which=None):
    """Every width x height of the edge set — word seams and neighbour words crossed in both the grid and the windows —, with max_dist
    rotating through 0, 1, 50 and 63."""
    e = edge_sizes(drv.T)
    sizes = [(nx, ny) for nx in e for ny in e] if which is None else which
    for k, (nx, ny) in enumerate(sizes):
        mask, items, queries = size_scene(nx, ny, 100 * nx + ny)
        run_and_check(drv, f"{nx}x{ny}", mask, items, queries, max_dist=(0, 1, 50, 63)[k % 4])


def check_word_seams(drv):
    """A one-cell item at x = T - 1, T, 2T - 1 and 2T of a row of 3T + 2 blocked cells with ONE free cell k cells to its left or right: the
    nearest set bit lies in this ballot word, the word to the left or the word to the right."""
    t = drv.T
    nx = 3 * t + 2
    for at in (t - 1, t, 2 * t - 1, 2 * t):
        for off in (-63, -62, -t + 1, -2, -1, 1, 2, t - 1, 62, 63):
            if not 0 <= at + off < nx:
                continue
            mask = np.ones((1, nx), np.uint8)
            mask[0, at + off] = 0
            got = run_and_check(drv, f"seam: item at {at}, free cell at {at + off}", mask, [[at]], [(0, 0, 0, 0)], max_dist=63)
            assert got[1][0].tolist() == (at + off, 0, abs(off), 1)
    # A window begins max_dist cells left of its item, so a one-cell item sits in lane 63 of its first word.  With a second cell at
    # x = 0 the window begins at the grid's edge, and the cell at `at` lies in the word to the RIGHT of a free cell before the seam.
    for at in (t, t + 6, 2 * t - 1, 2 * t, 2 * t + 1):
        for off in (-1, -7, -30, 1, 7, 30):
            mask = np.ones((1, nx), np.uint8)
            mask[0, at + off] = 0
            got = run_and_check(drv, f"seam: item at 0 and {at}, free cell at {at + off}", mask, [[0, at]], [(0, 0, 0, 0)], max_dist=63)
            assert got[1][0].tolist() == (at + off, 0, abs(off), 1)


def check_max_dist(drv):
    """For max_dist m in 0, 1, 50, 63: the only free cell at L1 distance m is found; at m + 1 it is not.  The free cell lies down and
    right of a one-cell item (the distance is split between the row pass and the column sweeps), then up and left."""
    nx, ny = 70, 66
    for m in (0, 1, 50, 63):
        for sign in (1, -1):
            ix, iy = (2, 1) if sign > 0 else (nx - 3, ny - 2)
            for dist, found in ((m, True), (m + 1, False)):
                dx = dist // 2
                fx, fy = ix + sign * dx, iy + sign * (dist - dx)
                mask = np.ones((ny, nx), np.uint8)
                mask[fy, fx] = 0
                got = run_and_check(drv, f"max_dist {m}: free cell at distance {dist}, sign {sign}", mask, [[iy * nx + ix]], [(0, 0, 0, 0), (0, fx, fy, T)], max_dist=m)
                assert (got[1]["d"][0] == dist) == found and got[1]["d"][0] in (dist, -1)


def shapes_scene(t):
    """On a (t + 6) x (t + 3) grid with a wall of obstacles: items touching each grid edge, a ring, a one-cell item in each corner, an
    L whose centroid lies outside it, and an item with duplicates whose mean lands on .5."""
    nx, ny = t + 6, t + 3
    rs = np.random.RandomState(5)
    mask = (rs.rand(ny, nx) < 0.35).astype(np.uint8)
    mask[ny // 2, 3:nx - 3] = 1
    ell = np.concatenate([rect(nx, 10, 10, 12, 30), rect(nx, 12, 28, 40, 30)])
    half = [20 * nx + 50, 20 * nx + 50, 21 * nx + 51, 20 * nx + 51]                 # sums 202 and 81 over 4: the means 50.5 and 20.25
    half2 = [20 * nx + 50, 23 * nx + 51]                                             # means 50.5 and 21.5: half to even gives 50 and 22
    items = [rect(nx, 0, 5, 3, 9), rect(nx, nx - 2, 30, nx, 41), rect(nx, 20, 0, 33, 2), rect(nx, 5, ny - 3, 9, ny), ring(nx, 30, 35, 47, 50, 2),
             [0], [nx - 1], [(ny - 1) * nx], [ny * nx - 1], ell, half, half2]
    queries = []
    for k in range(len(items)):
        queries += [(k, 0, 0, 0), (k, nx // 2, ny // 2, T), (k, 0, ny - 1, T), (k, nx - 1, 0, T), (k, 38, 42, T)]
    return mask, items, queries


def check_shapes(drv):
    mask, items, queries = shapes_scene(drv.T)
    rows, answers, counts = run_and_check(drv, "shapes", mask, items, queries)
    nx = mask.shape[1]
    assert rows["boundary"][4] == len(ref.boundary(items[4], nx, mask.shape[0])) == 2 * (17 + 15) - 4 + 2 * (13 + 11)       # the ring: outer and inner boundary
    assert (int(rows["cx"][10]), int(rows["cy"][10])) == (50, 20) and (int(rows["cx"][11]), int(rows["cy"][11])) == (50, 22)
    # the ring's hole is searched too: with everything but the hole's middle blocked, the answer is inside the ring
    hole = np.ones_like(mask)
    hole[42, 38] = 0
    got = run_and_check(drv, "ring, only its hole free", hole, [items[4]], [(0, 0, 0, 0)])
    assert got[1][0].tolist() == (38, 42, 6, 1)


def check_whole_grid(drv):
    """An item equal to the whole grid: B is the grid's border.  On an all-free and on a border-blocked map."""
    for nx, ny in ((1, 1), (2, 2), (7, 5), (drv.T + 1, 9)):
        free = np.zeros((ny, nx), np.uint8)
        inner = np.ones((ny, nx), np.uint8)
        inner[ny // 2, nx // 2] = 0
        queries = [(0, 0, 0, 0), (0, nx - 1, ny - 1, T), (0, 0, ny - 1, T)]
        for name, m in (("free", free), ("only the middle free", inner)):
            rows, _, _ = run_and_check(drv, f"whole grid {nx}x{ny}, {name}", m, [rect(nx, 0, 0, nx, ny)], queries)
            assert rows["boundary"][0] == (nx * ny if min(nx, ny) <= 2 else 2 * (nx + ny) - 4)


def check_entry_limit(drv):
    """2^19 entries and one more, on a 4096 x 2 grid: every cell once and cell 0 over and over, so that the mean lies near x = 32, every
    cell is a boundary cell and all 8 192 are examined at d = 0, with the target at the far end.  There both factors of the half-plane
    are near 2^31 and the product near 2^62; in 32 bits its sign is noise."""
    nx, ny = 4096, 2
    mask = (np.random.RandomState(19).rand(ny, nx) < 0.5).astype(np.uint8)
    mask[0, 0], mask[0, 5] = 1, 0
    n = ref.MAX_ENTRIES
    at = np.concatenate([rect(nx, 0, 0, nx, ny), np.zeros(n - nx * ny, np.int64)])
    far = [(0, nx - 1, ny - 1, T), (0, nx - 1, 0, T), (0, 0, ny - 1, T), (0, 0, 0, 0), (0, 40, 0, T)]
    f = n * (nx - 1) - (nx - 1) * nx
    assert 2 ** 61 < f * f < 2 ** 62 and len(at) == n
    rows, answers, counts = run_and_check(drv, "2^19 entries", mask, [at], far, max_dist=3)
    assert int(rows["n"][0]) == n and int(rows["flags"][0]) == 0 and counts[2] == 0 and answers["d"][0] == 0 and answers["n_at_d"][0] > 1000
    rows, answers, counts = run_and_check(drv, "2^19 + 1 entries", mask, [np.concatenate([at, [1]]), [5]], far + [(1, 0, 0, 0)], max_dist=3)
    assert int(rows["flags"][0]) == ref.ITEM_TOO_LONG and counts[:3] == [1, 5, 1] and (answers["d"][:5] == -1).all()


def check_flagged_items(drv):
    """An empty item, an index below 0, one at nx * ny and one far past it: flagged, no field, their queries answer none; the items
    beside them are not disturbed.  Queries with an item outside 0 .. n - 1, a target outside the grid or unknown flags answer none."""
    nx, ny = 20, 11
    rs = np.random.RandomState(3)
    mask = (rs.rand(ny, nx) < 0.4).astype(np.uint8)
    items = [rect(nx, 3, 3, 6, 5), [], [5, -1, 7], [nx * ny], rect(nx, 10, 6, 12, 9), [4, 2 ** 31 - 1], []]
    queries = [(k, 0, 0, f) for k in range(len(items)) for f in (0, T)]
    queries += [(-1, 0, 0, 0), (len(items), 0, 0, 0), (2 ** 31 - 1, 0, 0, T), (-2 ** 31, 0, 0, 0), (0, nx, 0, T), (0, -1, 0, T), (0, 0, ny, T), (0, 0, -1, T),
                (0, 2 ** 31 - 1, -2 ** 31, T), (0, nx, -1, 0), (0, 0, 0, 2), (0, 0, 0, 0x80000001), (4, 19, 10, T)]
    rows, answers, counts = run_and_check(drv, "flagged items", mask, items, queries)
    assert rows["flags"].tolist() == [0, 1, 2, 2, 0, 2, 1] and counts[2] == 5
    assert answers["d"][-4] >= 0, "a target outside the grid without the target bit is no target"
    assert answers["d"][-1] >= 0 and (answers["d"][-3:-1] == -1).all()


def check_sources(drv):
    """The d2 map of the clearance restatement with max_d2 = 0, 1, 4, 8: free iff d2 > max_d2, against the same call on the mask of
    those cells."""
    import clearance_ref
    t = drv.T
    rs = np.random.RandomState(11)
    ob = rs.rand(t + 7, t + 20) < 0.06
    d2 = clearance_ref.d2_two_pass(ob)
    ny, nx = ob.shape
    items = [rect(nx, 8, 8, 15, 13), rect(nx, t, 30, t + 5, 36), [3 * nx + 40]]
    queries = [(k, tx, ty, f) for k in range(3) for tx, ty, f in ((0, 0, 0), (nx - 1, ny - 1, T), (0, ny - 1, T), (nx // 2, 0, T))]
    seen = set()
    for max_d2 in (0, 1, 4, 8):
        assert (d2 == max_d2).any() and (d2 == max_d2 + 1).any()
        got = run_and_check(drv, f"d2 source, max_d2 = {max_d2}", d2, items, queries, source=ref.SRC_D2, max_d2=max_d2, max_dist=20)
        as_mask = drv.run((d2 <= max_d2).astype(np.uint8), items, queries, max_dist=20)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:2], as_mask[:2])) and got[2] == as_mask[2]
        seen.add(got[1].tobytes())
    assert len(seen) == 4


def check_batches(drv):
    """Items and queries in one call against each item alone with its queries, bit for bit."""
    mask, items, queries = shapes_scene(drv.T)
    rows, answers, counts = run_and_check(drv, "batch", mask, items, queries)
    for k in range(len(items)):
        mine = [n for n, q in enumerate(queries) if q[0] == k]
        r1, a1, c1 = drv.run(mask, [items[k]], [(0,) + tuple(queries[n][1:]) for n in mine])
        assert r1[0].tobytes() == rows[k].tobytes(), f"batch item {k}: the row depends on the batch"
        assert a1.tobytes() == answers[mine].tobytes(), f"batch item {k}: an answer depends on the batch"
    shuffled = list(reversed(queries))
    _, a2, _ = drv.run(mask, items, shuffled)
    assert a2.tobytes() == answers[::-1].tobytes(), "an answer depends on the order of the queries"


def check_short_work(drv):
    """work one byte short, shorter than its header, and empty: SGS_OK, the item rows (without the boundary count) and the counters
    written, every query none, counters[3] the bytes needed; the retry with that many is the full answer."""
    mask, items, queries = shapes_scene(drv.T)
    ny, nx = mask.shape
    want = ref.endpoints(mask, items, queries)
    need = want[2][3]
    for short in (need - 1, 8 * len(items) + 8, 8 * len(items), 8 * len(items) - 8, 0):
        rows, answers, counts = drv.run(mask, items, queries, work_bytes=short)
        assert counts == [0, len(queries), want[2][2], need], f"work of {short} bytes: counters {counts}"
        assert answers.tobytes() == np.array([ref.NONE] * len(queries), ref.ANSWER_DTYPE).tobytes(), f"work of {short} bytes: a query was answered"
        w_rows = want[0].copy()
        w_rows["boundary"] = 0
        assert rows.tobytes() == w_rows.tobytes(), f"work of {short} bytes: the item rows differ"
    check_call("the retry", drv.run(mask, items, queries, work_bytes=counts[3]), mask, items, queries, want=want)
    check_call("more work than needed", drv.run(mask, items, queries, work_bytes=need + 4096), mask, items, queries, want=want)


# ---- the reference's own answers ------------------------------------------------------------------------------------------------------------
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def golden_grid(scene):
    return np.array([list(bytes.fromhex(row)) for row in scene["grid"]], np.uint8)


def golden_items(scene):
    """{name: raster indices} of a scene's items, from their (y, x) lists."""
    nx = scene["width"]
    return {name: np.array([y * nx + x for y, x in it["mask_coords"]], np.int64) for name, it in scene["items"].items()}


def check_golden_queries(run):
    """run(grid uint8 [ny, nx], items list, queries) -> (rows, answers, counts).  Per scene: every centroid and boundary count; per
    query the None answers and d*; the answer itself where n_at_d == 1, and otherwise that the reference's cell is a candidate."""
    n_forced = n_none = n_q = 0
    for s in golden()["scenes"]:
        grid, items = golden_grid(s), golden_items(s)
        names = list(items)
        queries = [(names.index(q["item"]), q["towards"][0], q["towards"][1], T) if q["towards"] is not None else (names.index(q["item"]), 0, 0, 0) for q in s["queries"]]
        rows, answers, counts = run(grid, [items[n] for n in names], queries)
        _, _, _, cands = ref.endpoints(grid, [items[n] for n in names], queries)
        for k, name in enumerate(names):
            it = s["items"][name]
            assert [int(rows["cx"][k]), int(rows["cy"][k])] == it["centroid"], f"{s['name']}: {name}: centroid {(int(rows['cx'][k]), int(rows['cy'][k]))}, the reference has {it['centroid']}"
            assert int(rows["boundary"][k]) == it["n_boundary"], f"{s['name']}: {name}: {int(rows['boundary'][k])} boundary cells, the reference has {it['n_boundary']}"
        for k, q in enumerate(s["queries"]):
            a = answers[k]
            what = f"{s['name']}: query {k} ({q['item']} towards {q['towards']})"
            if q["answer"] is None:
                assert a.tolist() == ref.NONE, f"{what}: {a.tolist()}, the reference answers None"
                n_none += 1
                continue
            assert int(a["d"]) == q["d"], f"{what}: d = {int(a['d'])}, the reference's answer {q['answer']} lies at {q['d']}"
            if int(a["n_at_d"]) == 1:
                assert [int(a["x"]), int(a["y"])] == q["answer"], f"{what}: ({int(a['x'])}, {int(a['y'])}), the reference has {q['answer']}"
                n_forced += q["towards"] is not None
            else:
                assert tuple(q["answer"]) in cands[k], f"{what}: the reference's {q['answer']} is no candidate at d = {int(a['d'])}"
            n_q += 1
    assert n_forced >= 40 and n_none >= 20 and n_q > 100, (n_forced, n_none, n_q)


def golden_inst(scene):
    """The reference's itemid2inst of a scene: {name: {"mask_coords": [(y, x)]}}."""
    return {name: {"mask_coords": [tuple(c) for c in it["mask_coords"]]} for name, it in scene["items"].items()}


def check_golden_connectivity(run):
    """The reference's build_connectivity_map groups, as a set of frozensets: an item belongs to the 4-connected region of free cells
    (the regions restatement) that holds its answer without a target."""
    import regions_ref
    for s in golden()["scenes"]:
        grid, items = golden_grid(s), golden_items(s)
        names = list(items)
        _, answers, _ = run(grid, [items[n] for n in names], [(k, 0, 0, 0) for k in range(len(names))])
        labels, _ = regions_ref.label(grid == 0, 4)
        groups = {}
        for name, a in zip(names, answers):
            if int(a["d"]) >= 0:
                groups.setdefault(int(labels[int(a["y"]), int(a["x"])]), set()).add(name)
        assert 0 not in groups
        got, want = {frozenset(g) for g in groups.values()}, {frozenset(g) for g in s["connectivity"]}
        assert got == want, f"{s['name']}: groups {sorted(sorted(g) for g in got)}, the reference has {s['connectivity']}"
    assert sum(len(s["connectivity"]) for s in golden()["scenes"]) >= 4


def check_golden_pair_endpoints(run):
    """The recorded pairs (both endpoints forced): the two answers are the first and the last cell of the reference's trajectory; where
    it found no path both answers exist and lie in different 8-connected regions of the free cells."""
    import regions_ref
    n_path = n_none = 0
    for s in golden()["scenes"]:
        grid, items = golden_grid(s), golden_items(s)
        names = list(items)
        cent = {n: s["items"][n]["centroid"] for n in names}
        queries = []
        for p in s["pairs"]:
            queries += [(names.index(p["start"]), cent[p["end"]][0], cent[p["end"]][1], T), (names.index(p["end"]), cent[p["start"]][0], cent[p["start"]][1], T)]
        if not queries:
            continue
        _, answers, _ = run(grid, [items[n] for n in names], queries)
        labels, _ = regions_ref.label(grid == 0, 8)
        for k, p in enumerate(s["pairs"]):
            a, b = answers[2 * k], answers[2 * k + 1]
            what = f"{s['name']}: {p['start']} -> {p['end']}"
            assert int(a["n_at_d"]) == 1 and int(b["n_at_d"]) == 1, f"{what}: an endpoint is not forced"
            if p["result"] is None:
                assert labels[int(a["y"]), int(a["x"])] != labels[int(b["y"]), int(b["x"])], f"{what}: the reference found no path, the endpoints share a region"
                n_none += 1
                continue
            cell = lambda q: [int(np.floor((q["position"][0] - s["min"][0]) / s["scale"])), int(np.floor((q["position"][1] - s["min"][1]) / s["scale"]))]      # noqa: E731
            pts = p["result"]["points"]
            assert [int(a["x"]), int(a["y"])] == cell(pts[0]) and [int(b["x"]), int(b["y"])] == cell(pts[-1]), f"{what}: the endpoints differ from the reference's trajectory"
            n_path += 1
    assert n_path >= 20 and n_none >= 5, (n_path, n_none)


def check_golden_drv(drv):
    run = lambda grid, items, queries: drv.run(grid, items, queries)          # noqa: E731
    check_golden_queries(run)
    check_golden_connectivity(run)
    check_golden_pair_endpoints(run)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def check_refusals(drv):
    """Every refusal of the header returns SGS_ERR_INVALID with a message that names the argument and leaves the poisoned outputs
    untouched; then the context still works."""
    nx, ny, n, nq = 8, 4, 2, 3
    keep_s, s_ptr, _ = drv._put(np.zeros(nx * ny + 16, np.uint32))
    keep_o, o_ptr, _ = drv._put(np.array([0, 2, 3], np.uint32), slack=8)
    keep_c, c_ptr, _ = drv._put(np.array([1, 2, 12], np.int32), slack=8)
    keep_q, q_ptr, _ = drv._put(as_queries([(0, 0, 0, 0), (1, 7, 3, T), (1, 0, 0, 0)]), slack=8)
    bytes_ = int(drv.lib.sgs_endpoints_work_bytes(nx, ny, n))
    keep_w, w_ptr, w_get = drv._bytes(bytes_ + 64)
    keep_i, i_ptr, i_get = drv._bytes(56 * n + 64)
    keep_a, a_ptr, a_get = drv._bytes(16 * nq + 64)
    keep_n, n_ptr, n_get = drv._bytes(32 + 64)
    keep_b, b_ptr, b_get = drv._bytes(bytes_ + 56 * n + 16 * nq + 32 + 64)           # one buffer for the overlap cases

    def call(src=s_ptr, offsets=o_ptr, cells=c_ptr, n_items=n, queries=q_ptr, n_queries=nq, work=w_ptr, work_bytes=bytes_, items=i_ptr, answers=a_ptr,
             counts=n_ptr, null_params=False, **kw):
        return drv.call(src, None if null_params else c_params(**{**dict(nx=nx, ny=ny), **kw}), offsets, cells, n_items, queries, n_queries, work, work_bytes,
                        items, answers, counts)

    D = ref.SRC_D2
    bad = [(b"null src", dict(src=None)), (b"null params", dict(null_params=True)), (b"null item_offsets", dict(offsets=None)), (b"null item_cells", dict(cells=None)),
           (b"null work", dict(work=None)), (b"null out_items", dict(items=None)), (b"null out_counts", dict(counts=None)), (b"null queries", dict(queries=None)),
           (b"null out_queries", dict(answers=None)), (b"n_queries = -1", dict(n_queries=-1)), (b"n_queries = 4194305", dict(n_queries=(1 << 22) + 1)),
           (b"n_items = 0", dict(n_items=0)), (b"n_items = -3", dict(n_items=-3)), (b"n_items = 65536", dict(n_items=65536)), (b"nx = 0", dict(nx=0)),
           (b"ny = 0", dict(ny=0)), (b"nx = 4097", dict(nx=4097)), (b"ny = 4097", dict(ny=4097)), (b"unknown source 2", dict(source=2)),
           (b"unknown source -1", dict(source=-1)), (b"max_dist = -1", dict(max_dist=-1)), (b"max_dist = 64", dict(max_dist=64)),
           (b"max_d2 = 3 with a mask", dict(max_d2=3)), (b"unknown flags 0x1", dict(flags=1)), (b"unknown flags 0x80000000", dict(flags=0x80000000)),
           (b"reserved = 7", dict(reserved=7)), (b"reserved = -1", dict(reserved=-1)), (b"work_bytes = -8", dict(work_bytes=-8)),
           (b"item_offsets 0x", dict(offsets=o_ptr + 2)), (b"item_cells 0x", dict(cells=c_ptr + 1)), (b"queries 0x", dict(queries=q_ptr + 2)),
           (b"out_queries 0x", dict(answers=a_ptr + 2)), (b"src 0x", dict(src=s_ptr + 2, source=D)), (b"work 0x", dict(work=w_ptr + 4)),
           (b"out_items 0x", dict(items=i_ptr + 4)), (b"out_counts 0x", dict(counts=n_ptr + 4)),
           (b"overlap", dict(work=b_ptr, items=b_ptr + bytes_ - 8)), (b"overlap", dict(work=b_ptr + 56 * n - 8, items=b_ptr)),
           (b"overlap", dict(work=b_ptr, answers=b_ptr + bytes_ - 4)), (b"overlap", dict(work=b_ptr + 8, counts=b_ptr))]
    for word, kw in bad:
        assert call(**kw) == -1, f"{word.decode()} with {kw} was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"sgs_endpoints" in msg, (word, msg)
    drv._sync()
    for get, what in ((w_get, "work"), (i_get, "out_items"), (a_get, "out_queries"), (n_get, "out_counts"), (b_get, "an output or work")):
        assert (np.array(get()) == SENTINEL).all(), f"a refused call wrote to {what}"
    W = drv.lib.sgs_endpoints_work_bytes
    assert W(0, 4, 1) == -1 and W(4, 4097, 1) == -1 and W(4, 4, 0) == -1 and W(4, 4, 65536) == -1 and W(4096, 4096, 3) == 24 + 3 * 4096 * 4096 and W(3, 3, 1) == 8 + 16
    # the context still works: outputs right behind work, a mask at any byte, no queries with null pointers
    assert call() == 0 and call(src=s_ptr + 1, work=b_ptr, items=b_ptr + bytes_, answers=b_ptr + bytes_ + 56 * n, counts=b_ptr + bytes_ + 56 * n + 16 * nq) == 0
    assert call(queries=None, answers=None, n_queries=0) == 0
    drv._sync()
    a = np.array(a_get())[:16 * nq].view(ref.ANSWER_DTYPE)
    assert a.tolist() == [(1, 0, 0, 2), (4, 1, 0, 1), (4, 1, 0, 1)] and [int(v) for v in np.array(n_get())[:32].view(np.uint64)][:3] == [0, 0, 0]
