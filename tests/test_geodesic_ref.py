"""The restatement of the geodesic field (tests/geodesic_ref.py) held to three independent checks: a brute-force Bellman-Ford loop on
tiny maps, SciPy's Dijkstra with float weights 1 and sqrt(2) on the same graphs — SciPy checking the DEFINITION, the pairs recovered by
minimising |a + b sqrt(2) - d| —, and the reference's own recorded answers (tests/golden/geodesic_golden.json).  CPU only."""
import itertools
import math

import numpy as np
import pytest

import geodesic_cases as gc
import geodesic_ref as ref


def _tiny_maps():
    rs = np.random.RandomState(0)
    for k in range(40):
        ny, nx = int(rs.randint(1, 10)), int(rs.randint(1, 10))
        ob = rs.rand(ny, nx) < (0.0, 0.2, 0.35, 0.5)[k % 4]
        seeds = [(int(rs.randint(nx)), int(rs.randint(ny))) for _ in range(1 + k % 3)]
        yield ob, seeds
    ob = np.ones((5, 5), bool)                                                     # a diagonal corridor: only corner-cutting steps
    for k in range(5):
        ob[k, k] = False
    yield ob, [(0, 0)]


def test_less_is_the_order_of_a_plus_b_sqrt2():
    """Against exact arithmetic: a1 + b1 sqrt(2) < a2 + b2 sqrt(2) decided in Python integers of any size by squaring both sides."""
    def exact(a1, b1, a2, b2):
        p, q = a1 - a2, b2 - b1                                                    # p < q sqrt(2)
        if p < 0 <= q or (p == 0 and q > 0):
            return True
        if q <= 0 <= p:
            return False
        return p * p < 2 * q * q if p > 0 else p * p > 2 * q * q
    vals = [0, 1, 2, 3, 5, 7, 12, 29, 70, 99, 169, 408, 577, 985, 1393, 4096 ** 2]  # convergents of sqrt(2) among them: the closest calls
    for a1, b1, a2, b2 in itertools.product(vals, repeat=4):
        assert ref.less(a1, b1, a2, b2) == exact(a1, b1, a2, b2)
        assert not (ref.less(a1, b1, a2, b2) and ref.less(a2, b2, a1, b1))
        assert (a1, b1) == (a2, b2) or ref.less(a1, b1, a2, b2) or ref.less(a2, b2, a1, b1)      # two different pairs never cost the same
    A = np.array(list(itertools.product(vals[:9], repeat=4)), np.int64)
    assert np.array_equal(ref.less(A[:, 0], A[:, 1], A[:, 2], A[:, 3]).astype(bool), [exact(*r) for r in A.tolist()])
    # where fp32 fails: 47321 diagonal steps are cheaper than 66922 straight ones by 7.5e-6, far below the spacing of floats at 66922
    assert ref.less(0, 47321, 66922, 0) and np.float32(47321) * np.float32(math.sqrt(2)) == np.float32(66922)


def test_field_against_the_brute_force_loop():
    for ob, seeds in _tiny_maps():
        assert np.array_equal(ref.field(ob, seeds), ref.field_brute_force(ob, seeds)), (ob.astype(int).tolist(), seeds)


def test_field_against_scipy_dijkstra():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import dijkstra
    maps = list(_tiny_maps()) + [gc.sealed_region(8), (gc.size_pictures(21, 13, 8)["random_seeds_in_several_tiles"][0], [(0, 0)])]
    for ob, seeds in maps:
        ny, nx = ob.shape
        seeds = [s for s in seeds if not ob[s[1], s[0]]]
        if not seeds:
            continue
        rows, cols, w = [], [], []
        for j in range(ny):
            for i in range(nx):
                if ob[j, i]:
                    continue
                for di, dj in ref.DIRS:
                    ni, nj = i + di, j + dj
                    if 0 <= ni < nx and 0 <= nj < ny and not ob[nj, ni]:
                        rows.append(j * nx + i); cols.append(nj * nx + ni); w.append(1.0 if di == 0 or dj == 0 else ref.SQRT2)
        g = sp.csr_matrix((w, (rows, cols)), shape=(ny * nx, ny * nx))
        d = dijkstra(g, indices=[j * nx + i for i, j in seeds], min_only=True).reshape(ny, nx)
        fld = ref.field(ob, seeds)
        n = nx * ny
        a, b = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
        cost = a + b * ref.SQRT2
        for j in range(ny):
            for i in range(nx):
                if not np.isfinite(d[j, i]) or ob[j, i]:
                    assert fld[j, i].tolist() == [ref.NONE, ref.NONE]
                    continue
                k = np.unravel_index(np.argmin(np.abs(cost - d[j, i])), cost.shape)
                assert fld[j, i].tolist() == [int(k[0]), int(k[1])], (i, j, d[j, i])
        assert np.allclose(ref.distance_cells(fld)[~ob], d[~ob], rtol=0, atol=1e-9)                  # (SciPy's floats against a + b sqrt(2): the pairs above are the check)


def test_pictures_have_the_properties_the_checks_rely_on():
    for T in (32, 64):
        gc.check_picture_properties(T)


def test_path_follows_the_fixed_neighbour_order():
    ob = np.zeros((4, 4), bool)
    fld = ref.field(ob, [(0, 0)])
    assert fld[3, 2].tolist() == [1, 2]
    cells, status = ref.path(ob, fld, (2, 3))
    assert status == ref.PATH_OK and cells == [(2, 3), (2, 2), (1, 1), (0, 0)]      # (0, -1) comes before the diagonals
    assert ref.path(ob, fld, (2, 3), 2) == ([(2, 3), (2, 2)], ref.PATH_TRUNCATED)
    assert ref.path(ob, fld, (4, 0)) == ([], ref.PATH_INVALID)
    ob[1, 1] = True
    assert ref.path(ob, ref.field(ob, [(0, 0)]), (1, 1)) == ([], ref.PATH_UNREACHABLE)
    assert ref.count_steps(cells) == (1, 2)


def test_the_references_own_answers():
    """Every recorded pair: the reference's path has the field's pair, null exactly where the field is NONE, our path has the pair."""
    gc.check_golden(field_of=lambda ob, goal: ref.field(ob, [goal]),
                    path_of=lambda ob, fld, goal, starts: [(lambda c, s: c if s == ref.PATH_OK else None)(*ref.path(ob, fld, st)) for st in starts])


def test_trajectory_points_equal_the_references():
    gc.check_golden_trajectories(lambda *a: [dict(position=list(p), rotation=list(r)) for p, r in zip(*ref.trajectory_points(*a))])
    from sage_gs import geodesic
    gc.check_golden_trajectories(geodesic.trajectory_points)


def test_heap_search_has_the_fields_step_counts():
    for name, (ob, seeds) in gc.pictures(8).items():
        fld = ref.field(ob, seeds[:1])
        free = [(int(i), int(j)) for j, i in np.argwhere(~ob)][::5]
        for s in free:
            p = ref.heap_search(ob, s, seeds[0])
            if p is None:
                assert fld[s[1], s[0], 0] == ref.NONE or ob[seeds[0][1], seeds[0][0]], (name, s)
            else:
                assert ref.count_steps(p) == tuple(int(v) for v in fld[s[1], s[0]]), (name, s)
