"""The geodesic field and its paths (sgs_geodesic_field, sgs_geodesic_path; csrc/sgs_geodesic.h), restated on the host in integers.

A cost is the pair (a, b) = (straight steps, diagonal steps) and stands for a + b sqrt(2); two costs are compared exactly (less), as
the kernels compare them.  field() is a Dijkstra in buckets of width 1 (Dial): a cell whose cost lies in [d, d + 1) can only give its
neighbours costs >= d + 1, so once the buckets below d are done every cell of bucket d is final, and a whole bucket is relaxed at once
in NumPy.  The bucket of a cost is floor(a + b sqrt(2)) = a + isqrt(2 b^2), an integer computed exactly: no float decides anything.
test_geodesic_ref.py holds it to a brute-force loop, to SciPy's Dijkstra and to the reference's recorded answers."""
from __future__ import annotations

import heapq
import math

import numpy as np

NONE = 0xFFFFFFFF
SRC_MASK8, SRC_D2 = 0, 1
CONTINUE = 1
PATH_OK, PATH_UNREACHABLE, PATH_TRUNCATED, PATH_INVALID, PATH_NOT_FINAL = 0, 1, 2, 3, 4
DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))      # (di, dj): the reference's order, and the path's
SQRT2 = math.sqrt(2.0)


def less(a1, b1, a2, b2):
    """a1 + b1 sqrt(2) < a2 + b2 sqrt(2), exactly; Python ints or int64 arrays (|p|, |q| < 2^31)."""
    p, q = a1 - a2, b2 - b1
    if isinstance(p, np.ndarray) or isinstance(q, np.ndarray):
        p, q = np.asarray(p, np.int64), np.asarray(q, np.int64)
        pp, qq = p * p, 2 * q * q
        return np.where((p <= 0) & (q >= 0), (p != 0) | (q != 0), np.where((p >= 0) & (q <= 0), False, np.where(p > 0, pp < qq, pp > qq)))
    if p <= 0 and q >= 0:
        return p != 0 or q != 0
    if p >= 0 and q <= 0:
        return False
    return p * p < 2 * q * q if p > 0 else p * p > 2 * q * q


def blocked_of(src, source=SRC_MASK8, max_d2=0):
    src = np.asarray(src)
    return src != 0 if source == SRC_MASK8 else src.astype(np.uint32) <= np.uint32(max_d2)


def _isqrt_2b2(n):
    """isqrt(2 b^2) for b = 0 .. n - 1, exactly."""
    b = np.arange(n, dtype=np.int64)
    t = 2 * b * b
    k = np.floor(np.sqrt(t.astype(np.float64))).astype(np.int64)
    k -= k * k > t
    k += (k + 1) * (k + 1) <= t
    assert ((k * k <= t) & ((k + 1) * (k + 1) > t)).all()
    return k


def field(blocked, seeds):
    """blocked bool [ny, nx], seeds [(i, j)] -> uint32 [ny, nx, 2]: the pair of every cell, NONE where blocked or unreachable.  Seeds on
    blocked cells are ignored."""
    blocked = np.asarray(blocked, bool)
    ny, nx = blocked.shape
    W = nx + 2
    wall = np.ones((ny + 2, W), bool)
    wall[1:-1, 1:-1] = blocked
    wall = wall.reshape(-1)
    A = np.zeros(wall.size, np.int64)
    B = np.zeros(wall.size, np.int64)
    reached = np.zeros(wall.size, bool)
    done = np.zeros(wall.size, bool)
    isq = _isqrt_2b2(ny * nx + 2)
    start = np.unique(np.array([(j + 1) * W + i + 1 for i, j in seeds if not blocked[j, i]], np.int64))
    reached[start] = True
    buckets = {0: [start]} if len(start) else {}
    offs = [(dj * W + di, 1 if di == 0 or dj == 0 else 0) for di, dj in DIRS]
    while buckets:
        d = min(buckets)
        idx = np.unique(np.concatenate(buckets.pop(d)))
        idx = idx[~done[idx] & (A[idx] + isq[B[idx]] == d)]
        done[idx] = True
        a0, b0 = A[idx], B[idx]
        for off, straight in offs:
            t = idx + off
            keep = ~wall[t] & ~done[t]
            t, ca, cb = t[keep], a0[keep] + straight, b0[keep] + (1 - straight)
            better = ~reached[t] | less(ca, cb, A[t], B[t]).astype(bool)
            t, ca, cb = t[better], ca[better], cb[better]
            A[t], B[t], reached[t] = ca, cb, True
            key = ca + isq[cb]
            for k in np.unique(key):
                buckets.setdefault(int(k), []).append(t[key == k])
    out = np.full((ny + 2, W, 2), NONE, np.uint32)
    flat = out.reshape(-1, 2)
    flat[reached, 0], flat[reached, 1] = A[reached], B[reached]
    return np.ascontiguousarray(out[1:-1, 1:-1])


def field_brute_force(blocked, seeds):
    """The definition, as a loop: relax every cell from every neighbour until a whole pass changes nothing (Bellman-Ford)."""
    blocked = np.asarray(blocked, bool)
    ny, nx = blocked.shape
    d = {(i, j): (0, 0) for i, j in seeds if not blocked[j, i]}
    changed = True
    while changed:
        changed = False
        for j in range(ny):
            for i in range(nx):
                if blocked[j, i]:
                    continue
                for di, dj in DIRS:
                    n = (i + di, j + dj)
                    if n not in d:
                        continue
                    cand = (d[n][0] + 1, d[n][1]) if di == 0 or dj == 0 else (d[n][0], d[n][1] + 1)
                    if (i, j) not in d or less(cand[0], cand[1], *d[(i, j)]):
                        d[(i, j)] = cand
                        changed = True
    out = np.full((ny, nx, 2), NONE, np.uint32)
    for (i, j), v in d.items():
        out[j, i] = v
    return out


def path(blocked, fld, start, max_len=None):
    """The walk k_geo_path makes from start = (i, j): ([(i, j)], status)."""
    blocked = np.asarray(blocked, bool)
    ny, nx = blocked.shape
    i, j = int(start[0]), int(start[1])
    if not (0 <= i < nx and 0 <= j < ny):
        return [], PATH_INVALID
    a, b = int(fld[j, i, 0]), int(fld[j, i, 1])
    if blocked[j, i] or (a == NONE and b == NONE):
        return [], PATH_UNREACHABLE
    steps, cells = a + b, []
    for s in range(steps + 1):
        if max_len is not None and len(cells) == max_len:
            return cells, PATH_TRUNCATED
        cells.append((i, j))
        if s == steps:
            break
        for k, (di, dj) in enumerate(DIRS):
            ni, nj = i + di, j + dj
            if not (0 <= ni < nx and 0 <= nj < ny) or blocked[nj, ni]:
                continue
            va, vb = int(fld[nj, ni, 0]), int(fld[nj, ni, 1])
            if (va, vb) != (NONE, NONE) and (va + (1 if k < 4 else 0), vb + (0 if k < 4 else 1)) == (a, b):
                i, j, a, b = ni, nj, va, vb
                break
        else:
            return cells, PATH_NOT_FINAL
    return cells, PATH_OK


def count_steps(cells):
    """(a, b) of a list of (i, j) cells; raises if two consecutive cells are no 8-neighbours."""
    a = b = 0
    for (i0, j0), (i1, j1) in zip(cells[:-1], cells[1:]):
        di, dj = abs(i1 - i0), abs(j1 - j0)
        assert max(di, dj) == 1, f"{(i0, j0)} -> {(i1, j1)} is no step"
        if di + dj == 1:
            a += 1
        else:
            b += 1
    return a, b


def distance_cells(fld):
    """float64 [ny, nx]: a + b sqrt(2), inf where NONE."""
    f = np.asarray(fld, np.uint32).astype(np.float64)
    return np.where(np.asarray(fld)[..., 0] == NONE, np.inf, f[..., 0] + f[..., 1] * SQRT2)


def heap_search(blocked, start, goal):
    """A host heap search from start to goal, (i, j) each, in this project's own words: 8-connected, steps of 1 and sqrt(2) in floats,
    the straight-line distance as the heuristic, corners cut; the list of cells or None.  What scripts/geodesic_bench.py times beside
    the device; its floats decide orderings, so it is no oracle — test_geodesic_ref.py only checks its step counts on small maps."""
    blocked = np.asarray(blocked, bool)
    ny, nx = blocked.shape
    g = {start: 0.0}
    came = {}
    heap = [(0.0, start)]
    while heap:
        _, cur = heapq.heappop(heap)
        if cur == goal:
            cells = [cur]
            while cur in came:
                cur = came[cur]
                cells.append(cur)
            return cells[::-1]
        for di, dj in DIRS:
            n = (cur[0] + di, cur[1] + dj)
            if not (0 <= n[0] < nx and 0 <= n[1] < ny) or blocked[n[1], n[0]]:
                continue
            t = g[cur] + (1.0 if di == 0 or dj == 0 else SQRT2)
            if n not in g or t < g[n]:
                g[n], came[n] = t, cur
                heapq.heappush(heap, (t + math.hypot(n[0] - goal[0], n[1] - goal[1]), n))
    return None


def trajectory_points(cells, scale, min_x, min_y, fixed_z=0.5, sample_step=1):
    """(positions float64 [n, 3], rotations float64 [n, 4]) of a path of (x, y) cells: the cell centre min + (p + 0.5) * scale, every
    sample_step-th cell, yaw = atan2 towards the next sample (the last sample faces itself), rotation [0, 0, sin(yaw / 2), cos(yaw / 2)]."""
    xs = [min_x + (x + 0.5) * scale for x, _ in cells][::sample_step]
    ys = [min_y + (y + 0.5) * scale for _, y in cells][::sample_step]
    pos, rot = [], []
    for k in range(len(xs)):
        n = k + 1 if k + 1 < len(xs) else k
        yaw = math.atan2(ys[n] - ys[k], xs[n] - xs[k])
        pos.append([xs[k], ys[k], fixed_z])
        rot.append([0.0, 0.0, math.sin(yaw / 2.0), math.cos(yaw / 2.0)])
    return np.array(pos, np.float64).reshape(-1, 3), np.array(rot, np.float64).reshape(-1, 4)


# ---- the three kinds of map scripts/geodesic_bench.py times and test_gpu_geodesic.py checks ---------------------------------------------------
def open_room(n=512):
    ob = np.zeros((n, n), bool)
    ob[0], ob[-1], ob[:, 0], ob[:, -1] = True, True, True, True
    return ob


def rooms_with_doors(n=512, rooms=4, door=6, seed=0):
    """rooms x rooms rooms, each wall with one door of `door` cells at a seeded place."""
    rs = np.random.RandomState(seed)
    ob = open_room(n)
    cuts = [k * n // rooms for k in range(1, rooms)]
    for c in cuts:
        ob[c, :] = True
        ob[:, c] = True
    edges = [0] + cuts + [n - 1]
    for c in cuts:
        for lo, hi in zip(edges[:-1], edges[1:]):
            at = int(rs.randint(lo + 2, hi - door - 2))
            ob[c, at:at + door] = False
            at = int(rs.randint(lo + 2, hi - door - 2))
            ob[at:at + door, c] = False
    return ob


def serpentine_maze(n=512, pitch=16):
    """Corridors pitch - 1 cells wide between walls one cell thick, open at alternating ends: the longest shortest walk is about
    n^2 / pitch cells."""
    ob = open_room(n)
    for k, j in enumerate(range(pitch, n - 1, pitch)):
        ob[j, :] = True
        if k % 2 == 0:
            ob[j, n - pitch:n - 1] = False
        else:
            ob[j, 1:pitch] = False
    return ob


def seeded_free_cells(ob, n, seed=0):
    free = np.argwhere(~np.asarray(ob, bool))
    rs = np.random.RandomState(seed)
    return [(int(i), int(j)) for j, i in free[rs.choice(len(free), n, replace=len(free) < n)]]
