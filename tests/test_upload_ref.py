"""The upload's restatement (tests/upload_ref.py) against numbers worked out by hand: Morton keys of a few points, the bounds' treatment of
non-finite coordinates, and the window it allows a chunk's radius — on the restatement's own fp64 numbers."""
import numpy as np
import pytest

import upload_ref as ur

Q = 2097151          # 2^21 - 1
# (x, y, z) on the lattice [0, Q]^3 with both corners present (inv == 1.0f: the cell IS the coordinate) -> key, worked out by hand
LATTICE_KEYS = (
    ((0, 0, 0), 0x0),
    ((Q, Q, Q), 0x7FFFFFFFFFFFFFFF),
    ((1, 0, 0), 0x1), ((0, 1, 0), 0x2), ((0, 0, 1), 0x4),
    ((2, 0, 0), 0x8), ((3, 0, 0), 0x9), ((0, 0, 2), 0x20),
    ((5, 3, 6), 0o563),                              # bits 0: x1 y1 z0 = 3; bits 1: x0 y1 z1 = 6; bits 2: x1 y0 z1 = 5 (octal digit per bit triple)
    ((1 << 20, 0, 0), 1 << 60), ((0, 1 << 20, 0), 1 << 61), ((0, 0, 1 << 20), 1 << 62),
    ((Q, 0, 0), 0x1249249249249249), ((0, Q, 0), 0x2492492492492492), ((0, 0, Q), 0x4924924924924924),
    ((255, 0, 0), 0o111_111_11), ((256, 0, 0), 1 << 24),
)


def test_keys_of_a_hand_written_table():
    pts = np.array([p for p, _ in LATTICE_KEYS], np.float32)
    want = np.array([k for _, k in LATTICE_KEYS], np.uint64)
    lo, hi = ur.mean_bounds(pts)
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [Q, Q, Q]
    assert np.array_equal(ur.axis_cells(pts), pts.astype(np.uint64))
    got = ur.morton_keys(pts)
    assert got.dtype == np.uint64 and np.array_equal(got, want), [hex(int(g)) for g in got]
    assert np.array_equal(ur.deinterleave(want), pts.astype(np.uint64))
    # the permutation: ascending keys, equal keys in input order
    both = np.concatenate([pts, pts])
    perm = ur.expected_perm(np.concatenate([both] * 2))               # 68 points: more than the 64 below which nothing is sorted
    k = ur.morton_keys(np.concatenate([both] * 2))[perm]
    assert (np.diff(k.astype(np.float64)) >= 0).all()
    same = k[1:] == k[:-1]
    assert (perm[1:][same] > perm[:-1][same]).all()
    assert np.array_equal(ur.expected_perm(both), np.arange(len(both)))            # 34 points: not sorted
    assert np.array_equal(ur.expected_perm(np.concatenate([both] * 2), sorted_=False), np.arange(68))


def test_keys_over_real_bounds_and_non_finite_coordinates():
    # x over [-1, 1]: inv = 2097151 / 2 = 1048575.5 exactly; x = 0 -> u = 1048575.5 -> cell 1048575 = twenty ones
    pts = np.array([[-1, 5, 0], [1, 5, 0], [0, 5, 0], [0.5, 5, 0]], np.float32)
    q = ur.axis_cells(pts)
    assert q[:, 0].tolist() == [0, Q, 1048575, 1572863] and (q[:, 1:] == 0).all()      # (1.5 * 1048575.5 = 1572863.25; constant axes: inv = 0)
    assert ur.morton_keys(pts).tolist() == [0, 0x1249249249249249, 0x0249249249249249, 0x1049249249249249]
    # NaN, +-inf and +-3.0e38f take no part in the bounds, their own axis key is 0, the others' keys do not move
    wild = np.array([[np.nan, 5, 0], [0.5, np.inf, 0], [0.5, 5, -np.inf], [3.0e38, 5, 0], [-3.0e38, 5, 0], [0.5, -3.0e38, 3.0e38]], np.float32)
    both = np.concatenate([pts, wild])
    lo, hi = ur.mean_bounds(both)
    assert lo.tolist() == [-1, 5, 0] and hi.tolist() == [1, 5, 0]
    k = ur.morton_keys(both)
    assert np.array_equal(k[:4], ur.morton_keys(pts))
    assert k[4:].tolist() == [0, 0x1049249249249249, 0x1049249249249249, 0, 0, 0x1049249249249249]
    # -0.0 and +0.0 on an otherwise constant axis: hi > lo is False, the axis contributes nothing
    z = np.array([[-1, 0.0, 0], [1, -0.0, 0], [0, 0.0, 0]], np.float32)
    assert ur.morton_keys(z).tolist() == [0, 0x1249249249249249, 0x0249249249249249]
    # no finite coordinate at all
    assert ur.morton_keys(np.full((3, 3), np.nan, np.float32)).tolist() == [0, 0, 0]


def _chunk_scene(n=200, seed=3):
    rng = np.random.default_rng(seed)
    m = (rng.uniform(-1, 1, (n, 3)) * np.array([1.0, 0.3, 2.0]) + np.array([3.0, -2.0, 40.0])).astype(np.float32)
    s = np.exp(rng.uniform(-4, -1, (n, 3))).astype(np.float32)
    return m, s


def _exact_bounds(m, s, pad=1.0001):
    """Chunk bounds from fp64 arithmetic alone: centre as the restatement defines it, R = pad d + 1e-6 |c|_1 + 1e-30 rounded to fp32."""
    n = len(m); nc = (n + 63) // 64
    cb = np.zeros((nc, 8), np.float32)
    for c in range(nc):
        mm, ss = m[64 * c: 64 * c + 64], s[64 * c: 64 * c + 64]
        centre = np.float32(0.5) * (mm.min(axis=0) + mm.max(axis=0))
        d = np.sqrt(((mm.astype(np.float64) - centre.astype(np.float64)) ** 2).sum(axis=1)).max()
        cb[c, :3] = centre
        cb[c, 3] = pad * d + 1.0e-6 * np.abs(centre.astype(np.float64)).sum() + 1.0e-30
        cb[c, 4] = ss.max()
    return cb


def test_radius_window_on_the_restatements_own_numbers():
    m, s = _chunk_scene()
    cb = _exact_bounds(m, s)
    assert ur.check_chunk_bounds(m, s, cb, "exact") == 4            # 200 Gaussians: three full chunks and one of 8
    # ... the window: d itself is the least, the kernel's padding fits with room, three times the padding does not
    for pad, caught in ((1.0, None), (1.00019, None), (0.9999, "a member lies outside the sphere"), (1.0003, "the sphere is not tight")):
        cbp = _exact_bounds(m, s, pad)
        if caught is None:
            ur.check_chunk_bounds(m, s, cbp, f"pad {pad}")
        else:
            with pytest.raises(AssertionError, match=caught):
                ur.check_chunk_bounds(m, s, cbp, f"pad {pad}")
    for col, value, caught in ((3, np.inf, "the sphere is not tight"), (4, 0.0, "s_max of chunk 0"), (0, np.nextafter(cb[3, 0], np.float32(9)), "the centre of chunk 3"),
                               (6, 1.0, "spare words")):
        bad = cb.copy(); bad[3 if col == 0 else 0, col] = value
        with pytest.raises(AssertionError, match=caught):
            ur.check_chunk_bounds(m, s, bad, "seeded")
    # padding lanes take no part: the last chunk's bounds are those of its 8 members
    far = np.concatenate([m, np.zeros((56, 3), np.float32)])
    assert not np.array_equal(_exact_bounds(far, np.concatenate([s, s[:56]]))[3, :3], cb[3, :3])


def test_chunks_that_must_never_be_culled():
    m, s = _chunk_scene()
    for value in (np.nan, np.inf, -np.inf, 3.0e38, 1.0e30):
        mm = m.copy(); mm[70, 1] = value
        cb = _exact_bounds(m, s)
        if np.isfinite(value):          # (3.0e38f and 1e30 are finite: the centre is held to; the fp32 squares of the distance overflow)
            cb[1, :3] = np.float32(0.5) * (mm[64:128].min(axis=0) + mm[64:128].max(axis=0))
        with pytest.raises(AssertionError, match="must never be culled"):
            ur.check_chunk_bounds(mm, s, cb, repr(value))
        cb[1, 3] = np.inf
        ur.check_chunk_bounds(mm, s, cb, repr(value))
    ss = s.copy(); ss[130, 2] = 3.0e37
    cb = _exact_bounds(m, ss)
    with pytest.raises(AssertionError, match="must never be culled"):
        ur.check_chunk_bounds(m, ss, cb, "s_max")
    cb[2, 3] = np.inf
    ur.check_chunk_bounds(m, ss, cb, "s_max")
