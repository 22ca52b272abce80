"""tests/regions_ref.py held to three things it does not share code with: a brute-force flood fill on tiny grids, scipy.ndimage.label
for both structures on seeded random grids, and the items the reference's own build_semantic_maps wrote
(tests/golden/regions_golden.json).  CPU only."""
import numpy as np
import pytest

import regions_cases as rc
import regions_ref as ref


@pytest.mark.parametrize("conn", [8, 4])
def test_label_equals_a_flood_fill_on_tiny_grids(conn):
    rs = np.random.RandomState(3)
    for ny, nx in ((1, 1), (1, 7), (7, 1), (2, 2), (5, 6), (9, 4), (8, 8)):
        for density in (0.0, 0.3, 0.5, 0.7, 1.0):
            a = rs.rand(ny, nx) < density
            got, want = ref.label(a, conn), ref.flood_fill(a, conn)
            assert got[1] == want[1] and np.array_equal(got[0], want[0]), (ny, nx, density)


@pytest.mark.parametrize("conn", [8, 4])
def test_label_equals_scipy_on_seeded_grids(conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if conn == 8 else None
    rs = np.random.RandomState(5)
    for k in range(30):
        ny, nx = int(rs.randint(1, 70)), int(rs.randint(1, 70))
        a = rs.rand(ny, nx) < (0.3, 0.45, 0.6, 0.8)[k % 4]
        want, n = ndimage.label(a, structure=structure)
        got, m = ref.label(a, conn)
        assert m == n and np.array_equal(got, want), (k, ny, nx)


def test_rows_and_counters_by_hand():
    a = np.array([[1, 1, 0, 0, 1],
                  [0, 0, 0, 0, 1],
                  [1, 0, 1, 0, 0],
                  [0, 1, 0, 0, 1]], bool)
    labels, rows, counts = ref.regions(a, 8, max_regions=5)
    assert labels.tolist() == [[1, 1, 0, 0, 2], [0, 0, 0, 0, 2], [3, 0, 3, 0, 0], [0, 3, 0, 0, 4]]
    assert counts.tolist() == [4, 8, 3, 3]                                        # labels 1 and 2 have two cells, label 3 three
    assert rows[2].tolist() == (3, 0, 2, 3, 4, 10, 0 + 2 + 1, 2 + 2 + 3) and rows[3].tolist() == (1, 4, 3, 5, 4, 19, 4, 3)
    assert rows[4].tobytes() == ref.empty_rows(1).tobytes() and rows[4].tolist() == (0, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0, 2 ** 32 - 1, 0, 0)
    assert ref.regions(a, 4)[2].tolist() == [6, 8, 2, 1]
    tie = np.array([[1, 0, 1, 1, 0, 1, 1]], bool)
    assert ref.regions(tie)[2].tolist() == [3, 5, 2, 2]                           # the least label among the largest
    assert ref.regions(np.zeros((2, 3), bool))[2].tolist() == [0, 0, 0, 0]


def test_the_pictures_show_what_they_are_there_for():
    rc.check_picture_properties(32)
    rc.check_picture_properties(16)


def test_the_references_items_from_the_restatements_labels():
    from sage_gs import regions
    rc.check_golden(lambda occ, scale, x_min, y_min: regions.semantic_map_items(occ, scale, x_min, y_min, label_fn=lambda cells: ref.label(cells, 8)))
    for s in rc.golden()["scenes"]:
        assert regions.wall_value(rc.golden_occupancy(s)) == s["wall_value"]


def test_reachability_from_the_restatements_labels():
    rc.check_reachability(lambda free: ref.label(free, 8)[0])
