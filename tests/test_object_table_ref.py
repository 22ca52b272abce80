"""The restatement of the visible-object table (tests/object_table_ref.py) against the rule read aloud: a Python loop over the pixels,
on frames of at most 12 x 7 — so that the bincount / minimum.at form is not only checked against itself."""
import numpy as np

import object_cases as oc
import object_table_ref as ref


def _same(a, b):
    assert a[0].tobytes() == b[0].tobytes(), ref.first_difference(a[0], b[0])
    assert a[1].tolist() == b[1].tolist()


def test_restatement_equals_the_loop_on_small_frames():
    rs = np.random.RandomState(0)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.5, 1e-45, 2.0, 2.0, 0.25], np.float32)
    for k in range(40):
        H, W = rs.randint(1, 8), rs.randint(1, 13)
        n_labels = int(rs.randint(1, 6))
        ids = rs.randint(-3, n_labels + 2, (H, W)).astype(np.int32)
        depth = specials[rs.randint(0, len(specials), (H, W))]
        depth.view(np.uint32)[rs.rand(H, W) < 0.1] |= np.uint32(0x80000000)          # NaNs of the other sign among them
        _same(ref.table(ids, depth, n_labels), ref.table_by_loop(ids, depth, n_labels))
        _same(ref.table(ids, None, n_labels), ref.table_by_loop(ids, None, n_labels))


def test_small_pictures_of_the_cases():
    for make in (oc.one_pixel, oc.edge_labels, oc.depth_specials):
        for ids, depth, n_labels in make():
            assert ids.shape[0] <= 7 and ids.shape[1] <= 16
            _same(ref.table(ids, depth, n_labels), ref.table_by_loop(ids, depth, n_labels))


def test_known_table():
    ids = np.array([[0, 0, -1], [2, 0, 7]], np.int32)
    depth = np.array([[3.0, 1.0, 9.0], [4.0, -1.0, 0.5]], np.float32)
    rows, counts = ref.table(ids, depth, 3)
    assert rows[0].tolist() == (3, 0, 0, 2, 2, 1.0, 2, 1) and rows[2].tolist() == (1, 0, 1, 1, 2, 4.0, 0, 1)
    assert rows[1].tolist() == (0, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0, float("inf"), 0, 0) and counts.tolist() == [1, 1]
    assert ref.ROW_DTYPE.itemsize == 40


def test_the_pictures_are_what_they_are_built_for():
    oc.check_picture_properties()
