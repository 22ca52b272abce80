"""The clearance map's restatement (tests/clearance_ref.py) held to two things that are not it: a Python loop over cells and obstacles
on maps of at most 12 x 9, and SciPy's distance_transform_edt on seeded maps up to 130 x 97 — rint(edt^2) is the integer map, since
edt^2 is within 4 * 2^-53 of an integer, relatively.  The query in Python floats is held to hand-computed cells, and its NumPy
form to it.  None of this touches the library."""
import math

import numpy as np
import pytest

import clearance_cases as cc
import clearance_ref as ref


def loop_d2(ob):
    ny, nx = ob.shape
    out = np.full((ny, nx), ref.NONE, np.uint32)
    where = [(i, j) for j in range(ny) for i in range(nx) if ob[j, i]]
    for j in range(ny):
        for i in range(nx):
            for a, b in where:
                out[j, i] = min(int(out[j, i]), (i - a) ** 2 + (j - b) ** 2)
    return out


def small_maps():
    rs = np.random.RandomState(2)
    maps = [rs.rand(ny, nx) < d for nx, ny in ((1, 1), (1, 7), (7, 1), (12, 9), (5, 9), (12, 2)) for d in (0.0, 0.05, 0.3, 1.0)]
    return maps + [cc.shape_pictures()["ties"]]


def test_both_forms_equal_a_python_loop_on_small_maps():
    for ob in small_maps():
        want = loop_d2(ob)
        assert np.array_equal(ref.d2_brute(ob), want) and np.array_equal(ref.d2_two_pass(ob), want), ob.shape
    assert loop_d2(cc.shape_pictures()["ties"])[4, 3] == 25


def test_two_pass_equals_brute_force_on_every_picture():
    pics = {**cc.lane_pictures(), **cc.shape_pictures()}
    for nx, ny in cc.SIZES:
        pics.update({f"{nx}x{ny} {k}": v for k, v in cc.size_pictures(nx, ny).items()})
    for name, ob in pics.items():
        assert np.array_equal(ref.d2_two_pass(ob), ref.d2_brute(ob)), name
    cc.check_picture_properties()
    cc.check_seen_map_properties()


def test_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(4)
    for nx, ny, d in ((130, 97, 0.01), (130, 97, 0.002), (64, 3, 0.1), (3, 257, 0.01), (97, 130, 0.3)):
        ob = rs.rand(ny, nx) < d
        assert ob.any()
        e = ndi.distance_transform_edt(~ob) ** 2
        # SciPy roots an exact integer and the test squares it again: two roundings, a relative error below 4 * 2^-53 — nowhere near 0.5
        assert np.abs(e - np.rint(e)).max() <= 4 * 2.0 ** -53 * e.max() < 1e-9
        assert np.array_equal(np.rint(e).astype(np.uint32), ref.d2_two_pass(ob)), (nx, ny, d)


def test_counts_and_obstacles():
    d = np.array([[0, 1, 4], [ref.NONE - 1, 5, 2]], np.uint32)
    assert ref.counts(d, 0) == [1, 0, 5, 0] and ref.counts(d, 4) == [1, 3, 2, 0] and ref.counts(d, ref.NONE - 1) == [1, 5, 0, 0]
    assert ref.counts(np.full((2, 2), ref.NONE, np.uint32), 7) == [0, 0, 0, 4]
    g = np.array([[[0, 0], [2, 0], [0, 1], [5, 3], [2, 2]]], np.uint32)              # (free, occupied)
    assert ref.obstacles(g, None, 1).tolist() == [[False, False, True, True, True]]
    assert ref.obstacles(g, None, 3).tolist() == [[False, False, False, True, False]]
    assert ref.obstacles(g, None, 1, True).tolist() == [[True, False, True, True, True]]
    assert ref.obstacles(g, None, 3, True).tolist() == [[True, True, True, True, True]]


def test_inflation_limit():
    for (r, s), want in {(0.1, 0.05): 4, (0.15, 0.05): 8, (0.25, 0.05): 25, (0.12, 0.05): 5, (0.3, 0.1): 8, (0.5, 0.05): 100, (0.0, 0.05): 0}.items():
        assert ref.inflation_limit(r, s) == want, (r, s)
    assert math.sqrt((0.05 * 3) ** 2) > 0.15                                            # why three cells are outside a radius of 0.15


def test_inflation_limit_is_scipys_threshold():
    ndi = pytest.importorskip("scipy.ndimage")
    ob = np.zeros((41, 41), bool)
    ob[20, 20] = True
    d2 = ref.d2_two_pass(ob)
    for r, s in ((0.1, 0.05), (0.15, 0.05), (0.25, 0.05), (0.12, 0.05), (0.3, 0.1), (0.5, 0.05)):
        assert np.array_equal(ndi.distance_transform_edt(~ob, sampling=s) <= r, d2 <= ref.inflation_limit(r, s)), (r, s)


def test_query_by_hand():
    d2 = cc.id_map()
    f = cc.PLAIN
    q = lambda x, y, **kw: ref.query(d2, f.but(**kw), [[0.0, 0.0, x, y]])[0].tolist()      # noqa: E731
    assert q(1.0, -2.0) == [1, 1] and q(1.0 + 8 * 0.25, -2.0 + 6 * 0.25) == [0, 609]
    assert q(1.0 + 0.25 * 2.5, -2.0) == [1, 3] and q(1.0 + 0.25 * 3.5, -2.0) == [1, 5]     # ties to even
    assert q(1.0 - 0.5, -2.0) == [1, 1] and q(1.0 - 0.5, -2.0, margin=1) == [1, ref.NONE]
    assert q(float("nan"), 0.0) == [1, ref.NONE] and q(0.0, float("inf")) == [1, ref.NONE]
    assert q(-1.0, 2.0, flags=ref.NEGATE) == [1, 1] and q(3.0, -2.0, flags=ref.FLIP_X, sum_x=4.0) == [1, 1]
    assert q(1.0, 1.5, flags=ref.FLIP_Y, sum_y=-0.5) == [1, 1]
    # ten samples from cell (0, 0) to cell (8, 6) with only cell 609 colliding: the last sample is the first hit
    seg = [[1.0, -2.0, 3.0, -0.5]]
    assert ref.query(d2, f.but(n_samples=10, max_d2=0), seg)[0].tolist() == [0, 609]
    only_end = np.where(d2 == 609, 0, d2)
    assert ref.query(only_end, f.but(n_samples=10, max_d2=0), seg)[0].tolist() == [10, 0]


def test_vectorised_query_equals_the_loop():
    d2 = cc.id_map()
    segs = np.concatenate([cc.query_segments(), cc.half_way_points()[1], [[float("nan"), 0, 1, 1], [0, 0, float("inf"), 1], [2, -1, 2, -1]]])
    for flags in (0, 7, ref.FLIP_X):
        for margin in (0, 2):
            for ns in (0, 1, 2, 10):
                f = cc.PLAIN.but(flags=flags, margin=margin, n_samples=ns, max_d2=250, sum_x=4.0, sum_y=-2.5)
                assert np.array_equal(ref.query_vectorised(d2, f, segs), ref.query(d2, f, segs)), (flags, margin, ns)
