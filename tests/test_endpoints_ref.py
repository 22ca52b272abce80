"""The restatement of the item endpoints (tests/endpoints_ref.py) held to a brute force — the field as "min over B of |dx| + |dy|",
the answer as a scan of every cell in Python integers — on seeded grids, to its own arithmetic (half to even), and to the reference's
recorded answers (tests/golden/endpoints_golden.json).  NumPy only."""
import os
from fractions import Fraction

import numpy as np

import endpoints_cases as ec
import endpoints_ref as ref


def brute_field(b, nx, ny):
    ys, xs = np.mgrid[:ny, :nx]
    return np.min([np.abs(xs - x) + np.abs(ys - y) for (y, x) in b], axis=0)


def brute_query(free, cells, max_dist, target):
    ny, nx = free.shape
    pts = [(int(c) // nx, int(c) % nx) for c in cells]
    s = set(pts)
    b = [(y, x) for (y, x) in s if not {(y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)} <= s]
    mx, my = Fraction(sum(x for _, x in pts), len(pts)), Fraction(sum(y for y, _ in pts), len(pts))
    best = {}
    for y in range(ny):
        for x in range(nx):
            d = min(abs(x - bx) + abs(y - by) for (by, bx) in b)
            if d > max_dist or not free[y, x]:
                continue
            if target is not None and (x - mx) * (target[0] - mx) + (y - my) * (target[1] - my) < 0:
                continue
            best.setdefault(d, []).append((x, y))
    if not best:
        return ref.NONE, set()
    d = min(best)
    return (best[d][0][0], best[d][0][1], d, len(best[d])), set(best[d])


def test_the_field_is_the_l1_distance_to_the_boundary():
    for seed, (nx, ny) in enumerate(((1, 1), (7, 1), (1, 9), (13, 11), (40, 23), (66, 5))):
        rs = np.random.RandomState(seed)
        cells = rs.randint(0, nx * ny, max(1, nx * ny // 5))
        b = ref.boundary(cells, nx, ny)
        assert np.array_equal(ref.field(b, nx, ny), brute_field(b, nx, ny))
    assert ref.boundary(ec.rect(9, 2, 2, 7, 6), 9, 8) == {(y, x) for y in range(2, 6) for x in range(2, 7) if y in (2, 5) or x in (2, 6)}
    assert len(ref.boundary(ec.rect(5, 0, 0, 5, 4), 5, 4)) == 14                     # the whole grid: its border


def test_answers_against_a_scan_of_every_cell():
    n_none = n_tie = 0
    for seed in range(40):
        rs = np.random.RandomState(100 + seed)
        nx, ny = int(rs.randint(1, 24)), int(rs.randint(1, 24))
        free = rs.rand(ny, nx) > rs.uniform(0.2, 0.95)
        cells = rs.randint(0, nx * ny, int(rs.randint(1, 12)))
        cells = np.concatenate([cells, cells[:int(rs.randint(0, len(cells) + 1))]])
        for target in (None, (int(rs.randint(nx)), int(rs.randint(ny))), (0, 0), (nx - 1, ny - 1)):
            for max_dist in (0, 2, 50):
                got = ref.query(free, cells, max_dist, target)
                assert got == brute_query(free, cells, max_dist, target), (seed, target, max_dist)
                n_none += got[0] == ref.NONE
                n_tie += got[0][3] > 1
    assert n_none > 20 and n_tie > 20


def test_half_to_even_and_the_rows():
    assert [ref.round_half_even(s, n) for s, n in ((1, 2), (3, 2), (5, 2), (7, 2), (10, 4), (14, 4), (9, 4), (11, 4), (0, 3))] == [0, 2, 2, 4, 2, 4, 2, 3, 0]
    rs = np.random.RandomState(4)
    for _ in range(200):
        n = int(rs.randint(1, 30))
        v = rs.randint(0, 4096, n)
        assert ref.round_half_even(int(v.sum()), n) == int(round(np.array(v).mean()))
    row = ref.item_row([12, 12, 13, 22], 10, 5)
    assert row.tolist() == (4, 0, 2, 1, 4, 3, 2, 1, 3, 0, 9, 5)
    assert ref.item_row([], 10, 5).tolist() == (0, 1, ref.INT32_MAX, ref.INT32_MAX, 0, 0, -1, -1, 0, 0, 0, 0)
    assert int(ref.item_row([3, 50], 10, 5)["flags"]) == ref.ITEM_BAD_CELL and int(ref.item_row([-1], 10, 5)["flags"]) == ref.ITEM_BAD_CELL
    assert ref.window(row, 10, 5, 2) == (0, 0, 6, 5) and ref.window(row, 10, 5, 0) == (2, 1, 2, 2)
    assert ref.work_needed([row, ref.item_row([], 10, 5)], 10, 5, 0) == 16 + 8


def test_the_golden_file_is_small_and_the_restatement_agrees_with_it():
    assert os.path.getsize(ec.GOLDEN) < 200 * 1024
    run = lambda grid, items, queries: ref.endpoints(grid, items, queries)[:3]          # noqa: E731
    ec.check_golden_queries(run)
    ec.check_golden_connectivity(run)
    ec.check_golden_pair_endpoints(run)
