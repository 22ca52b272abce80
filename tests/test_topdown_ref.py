"""tests/topdown_ref.py (the NumPy restatement the top-down map's kernels are held to) against a pixel-by-pixel Python loop on small
frames, and against a case computed by hand: every product there is exact and the expected cells are written out as literals."""
import numpy as np
import pytest

import topdown_ref as ref

F = np.float32


def loop(depth, P, p, grid=None):
    """One pixel at a time, in np.float32 scalars, the header's text line by line."""
    n, H, W = depth.shape
    g = np.zeros((p.ny, p.nx, 2), np.uint32)
    if grid is not None and not (p.flags & ref.CLEAR):
        g[:] = grid
    counts = np.zeros((n, 4), np.uint32)
    inv = F(1.0) / F(p.cell_size)
    with np.errstate(all="ignore"):
        for f in range(n):
            a = [F(v) for v in P[f]]
            for y in range(H):
                for x in range(W):
                    z = F(depth[f, y, x])
                    if not (F(p.min_z) <= z and z <= F(p.max_z)):
                        counts[f, 0] += 1
                        continue
                    d = [F(F(F(F(x) * a[3 * k]) + F(F(y) * a[3 * k + 1])) + a[3 * k + 2]) for k in range(3)]
                    q = [F(F(z * d[k]) + a[9 + k]) for k in range(3)]
                    u = F(F(q[0] - F(p.origin_x)) * inv)
                    v = F(F(q[1] - F(p.origin_y)) * inv)
                    if not (u >= 0 and u < F(p.nx) and v >= 0 and v < F(p.ny)):
                        counts[f, 1] += 1
                        continue
                    h = q[2]
                    if F(p.free_lo) <= h and h <= F(p.free_hi):
                        ch = 0
                    elif F(p.occ_lo) < h and h <= F(p.occ_hi):
                        ch = 1
                    else:
                        counts[f, 2] += 1
                        continue
                    counts[f, 3] += 1
                    g[int(v), int(u), ch] += 1
    return g, counts


def _random_case(seed, n, H, W):
    rs = np.random.RandomState(seed)
    depth = rs.uniform(0.0, 7.0, (n, H, W)).astype(F)
    specials = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1.0, 0.1, 6.5]
    for k, s in enumerate(specials[:H * W]):
        depth.reshape(n, -1)[k % n, (3 * k) % (H * W)] = s
    P = np.stack([ref.pix_to_map(W / 1.2, H / 0.9, W / 2, H / 2,
                                 _look(rs.uniform(-1, 1, 3) + [0, 0, 1.2], rs.uniform(0, 6.28), rs.uniform(-0.9, 0.3))) for _ in range(n)])
    return depth, P


def _look(pos, yaw, pitch):
    """world (z up) -> camera (+Z forward, +X right, +Y down) of a camera at pos, turned by yaw about z and pitched."""
    fwd = np.array([np.cos(yaw) * np.cos(pitch), np.sin(yaw) * np.cos(pitch), np.sin(pitch)])
    right = np.array([np.sin(yaw), -np.cos(yaw), 0.0])
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    v = np.eye(4)
    v[:3, :3], v[:3, 3] = R, -R @ np.asarray(pos, np.float64)
    return v


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 7, 12), (3, 5, 3), (1, 7, 1), (2, 1, 12)], ids=str)
def test_restatement_equals_the_pixel_loop(shape):
    n, H, W = shape
    depth, P = _random_case(17 * H + W, n, H, W)
    seen = np.zeros(4, np.int64)
    for p in (ref.Params(nx=40, ny=36, origin_x=-2.0, origin_y=-1.8, cell_size=0.1),
              ref.Params(nx=5, ny=3, origin_x=-1.0, origin_y=-0.5, cell_size=0.37, min_z=0.0, max_z=float("inf"), free_hi=0.4, occ_lo=0.2)):
        got, got_counts = ref.topdown(depth, P, p)
        want, want_counts = loop(depth, P, p)
        assert np.array_equal(got, want) and np.array_equal(got_counts, want_counts)
        assert (got_counts.sum(1) == H * W).all() and int(got.sum()) == int(got_counts[:, 3].sum())
        before = np.arange(2 * p.nx * p.ny, dtype=np.uint32).reshape(p.ny, p.nx, 2)
        q = p.but(flags=0)
        acc, _ = ref.topdown(depth, P, q, grid=before)
        assert np.array_equal(acc, loop(depth, P, q, grid=before)[0]) and np.array_equal(acc, before + want)
        assert np.array_equal(ref.topdown(depth, P, p, grid=before)[0], want)
        seen += got_counts.sum(0).astype(np.int64)
    if H * W > 1:
        assert seen[3] > 0 and seen[0] > 0, "the case proves too little"


def hand_case():
    """A camera 2 m above a floor, looking straight down, axes aligned: fx = fy = 4 and cx = cy = 0.5, so map x = z * 0.25 x,
    map y = z * 0.25 y and h = 2 - z; cells of 0.25 m from the origin, so u = z x and v = z y.  Depths are powers of two: every
    product is exact.  6 x 8 cells, z in [0.1, 6.5], free [-0.15, 0.15], occupied (0.15, 1.5]."""
    P = np.array([0.25, 0, 0, 0, 0.25, 0, 0, 0, -1, 0, 0, 2], F)
    depth = np.array([[[2, 2, 1, 0.5],           # (0,0) h 0 free; (2,0) h 0 free; (2,0) h 1 occupied; u 1.5 -> (1,0), h 1.5: the band's edge, occupied
                       [2, 4, 8, 2]]], F)        # (0,2) free; u 4, v 4, h -2: no band; z 8 > 6.5; u 6 == nx: outside
    return depth, P[None], ref.Params(nx=6, ny=8, origin_x=0.0, origin_y=0.0, cell_size=0.25)


def test_hand_computed_case():
    depth, P, p = hand_case()
    want = np.zeros((8, 6, 2), np.uint32)
    want[0, 0, 0] = 1
    want[0, 2, 0] = 1
    want[0, 2, 1] = 1
    want[0, 1, 1] = 1
    want[2, 0, 0] = 1
    grid, counts = ref.topdown(depth, P, p)
    assert np.array_equal(grid, want) and counts.tolist() == [[1, 1, 1, 5]]
    assert ref.summary(grid) == [2, 2, 3, 2] and ref.summary(grid, 2) == [0, 0, 3, 2]
    cls, key = ref.classify(depth[0], P[0], p)
    assert cls.tolist() == [[3, 3, 3, 3], [3, 2, 0, 1]] and key.tolist() == [[0, 4, 5, 3], [24, -1, -1, -1]]


def test_pix_to_map_of_the_hand_case_camera():
    view = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 2], [0, 0, 0, 1]], np.float64)     # camera z = 2 - world z (a mirror: only the numbers matter here)
    assert ref.pix_to_map(4, 4, 0.5, 0.5, view).tolist() == hand_case()[1][0].tolist()


def test_summary_counts_cells_on_both_sides_of_min_hits():
    g = np.zeros((2, 3, 2), np.uint32)
    g[0, 0] = (5, 0); g[0, 1] = (2, 3); g[0, 2] = (3, 2); g[1, 0] = (0, 7); g[1, 1] = (2, 2)
    assert ref.summary(g, 1) == [4, 1, 12, 14] and ref.summary(g, 3) == [2, 2, 12, 14] and ref.summary(g, 8) == [0, 0, 12, 14]
    big = np.full((3, 2, 2), 0xFFFFFFFF, np.uint32)
    assert ref.summary(big, 1) == [6, 0, 6 * 0xFFFFFFFF, 6 * 0xFFFFFFFF]
