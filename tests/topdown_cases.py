"""The top-down seen map's checks (sgs_topdown_map, sgs_topdown_summary), shared by the CPU-emulator tests (test_emu_topdown.py, its
mutants) and the GPU tests (test_gpu_topdown.py): the pictures, a driver of the C ABI over plain buffers, and the assertions against
tests/topdown_ref.py.  Every comparison is exact equality of every count: there is no tolerance anywhere in this feature."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

import jpeg_cases
import topdown_ref as ref
from abi_driver import POISON, SENTINEL, AbiDriver, GpuBuffers      # POISON: grid, out_counts and out before every call

F = np.float32
INF = float("inf")


def _constants():
    """SGS_TOPDOWN_REGION, SLOT_BITS, SLOTS, HASH, MAX_FRAMES, SUM_BLOCKS, THREADS of csrc/sgs_topdown.h."""
    import emu_harness
    hdr = open(os.path.join(emu_harness.PKG, "csrc", "sgs_topdown.h")).read()
    get = lambda name: int(re.search(rf"#define SGS_TOPDOWN_{name} (0x[0-9A-Fa-f]+|\d+)", hdr).group(1), 0)       # noqa: E731
    threads, per_thread, bits = get("THREADS"), get("PER_THREAD"), get("SLOT_BITS")
    assert "SGS_TOPDOWN_REGION (SGS_TOPDOWN_THREADS * SGS_TOPDOWN_PER_THREAD)" in hdr and "SGS_TOPDOWN_SLOTS (1 << SGS_TOPDOWN_SLOT_BITS)" in hdr
    assert "(key * SGS_TOPDOWN_HASH) >> (32 - SGS_TOPDOWN_SLOT_BITS)" in hdr
    return threads * per_thread, bits, 1 << bits, get("HASH"), get("MAX_FRAMES"), get("SUM_BLOCKS"), threads


REGION, SLOT_BITS, SLOTS, HASH, MAX_FRAMES, SUM_BLOCKS, THREADS = _constants()


def slot_of(key):
    return ((int(key) * HASH) & 0xFFFFFFFF) >> (32 - SLOT_BITS)


def chunk_edit(chunk):
    """The edit that makes sgs_topdown_map cut its frames into launches of `chunk` (SGS_TOPDOWN_MAX_FRAMES, csrc/sgs_topdown.h)."""
    return ("#define SGS_TOPDOWN_MAX_FRAMES 65535 ", f"#define SGS_TOPDOWN_MAX_FRAMES {int(chunk)} ")


# ---- pictures: [(depth fp32 [H,W], P fp32 [12], ref.Params)] ----------------------------------------------------------------------------
def look(pos, yaw, pitch):
    from sage_gs import scenes
    return scenes.view_from_yaw(pos, yaw, pitch)


def seen_room(W, H, seed, pitch=-0.55):
    """What a camera at eye height sees of an empty 6 x 5 x 2.8 m room (floor z = 0, four walls, a ceiling), pitched down: the depth
    of the nearest plane along every pixel's ray in fp64, rounded; a few samples replaced by NaN, +inf and 0.  Floor pixels share
    cells in runs, wall pixels pile up in a few cells, the upper wall is in no band, the far corner is past max_z = 3."""
    rs = np.random.RandomState(seed)
    pos = np.array([rs.uniform(1.5, 4.5), rs.uniform(1.5, 3.5), 1.2])
    view = look(pos, rs.uniform(0, 2 * np.pi), pitch)
    fx, fy = 0.6 * max(W, 4), 0.6 * max(H, 4)                  # (a wide field of view along both axes, however narrow the frame)
    P = ref.pix_to_map(fx, fy, W / 2, H / 2, view)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(xx + 0.5 - W / 2) / fx, (yy + 0.5 - H / 2) / fy, np.ones_like(xx)], -1) @ view[:3, :3]      # world direction per unit z
    t = np.full((H, W), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for axis, planes in ((0, (0.0, 6.0)), (1, (0.0, 5.0)), (2, (0.0, 2.8))):
            for c in planes:
                s = (c - pos[axis]) / ray[..., axis]
                t = np.where((s > 0) & (s < t), s, t)
    depth = t.astype(F)
    flat = depth.reshape(-1)
    for k, v in enumerate((np.nan, np.inf, 0.0)[:flat.size // 8]):
        flat[(7 * k + 3) % flat.size] = v
    return depth, P, ref.Params(nx=90, ny=110, origin_x=-0.25, origin_y=-0.25, cell_size=0.05, max_z=3.0)      # x up to 4.25: the wall at x = 6 is outside


SIZES = ((1, 1), (63, 3), (64, 3), (65, 3), (67, 5))                     # wave and row ends
THREE_REGIONS = (100, 100)                                               # 10000 pixels: the region boundaries 4096 and 8192 lie mid-row
NARROW_SIZES = ((1, 4500), (2, 2500), (3, 1500), (5, 900))


def sizes():
    return [seen_room(W, H, 10 + k) for k, (W, H) in enumerate(SIZES)]


def three_regions():
    W, H = THREE_REGIONS
    assert 2 * REGION < W * H <= 3 * REGION and REGION % W != 0 and (2 * REGION) % W != 0
    return [seen_room(W, H, 20), seen_room(W, H, 21, pitch=-1.2)]


def narrow():
    """Frames 1, 2, 3 and 5 pixels wide that cross a region: dozens of image rows per wave, x wrapping at every k."""
    out = []
    for k, (W, H) in enumerate(NARROW_SIZES):
        assert W * H > REGION and (W * H) % REGION != 0
        out.append(seen_room(W, H, 30 + k))
    return out


def _at_positions(W, H, P, p, depth=None):
    return (np.ones((H, W), F) if depth is None else np.asarray(depth, F)), np.asarray(P, F), p


def wall():
    """67 x 70, every pixel in one cell (a = b = c = 0: the point is t), free and then occupied: two regions, one key."""
    out = []
    for h in (0.0, 1.0):
        P = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0.625, 0.375, h]
        out.append(_at_positions(67, 70, P, ref.Params(nx=4, ny=3, origin_x=0.0, origin_y=0.0, cell_size=0.25)))
    return out


def own_cell():
    """97 x 89, every pixel its own cell (u = x, v = y; image row 0 free, the others occupied): 4096 keys meet in a region's 1024 slots — all but the
    slots' owners take the no-slot path."""
    W, H = 97, 89
    assert min(W * H, REGION) >= 2 * SLOTS and W * H > 2 * REGION
    P = [1, 0, 0, 0, 1, 0, 0, 0.5, 0, 0, 0, 0]                                       # h = 0.5 y
    p = ref.Params(nx=W, ny=H, origin_x=0.0, origin_y=0.0, cell_size=1.0, free_lo=-100.0, free_hi=0.0, occ_lo=0.0, occ_hi=100.0)
    return [_at_positions(W, H, P, p)]


def keyed(ids, channel=0, nx=None):
    """A frame whose pixel with ids[y, x] = i >= 0 lands in cell (i, 0) of an nx x 1 grid, channel `channel` (key 2 i + channel), by
    its depth i + 0.5 (a = b = 0, c_0 = 1: p_0 = z; cells of 1 m); ids < 0: NaN, not binned."""
    ids = np.asarray(ids, np.int64)
    assert ids.max() < 2 ** 22
    depth = np.where(ids >= 0, ids + 0.5, np.nan).astype(F)
    P = np.array([0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1.0 if channel else 0.0], F)
    p = ref.Params(nx=int(ids.max()) + 1 if nx is None else nx, ny=1, origin_x=0.0, origin_y=0.0, cell_size=1.0, min_z=0.0, max_z=INF)
    return depth, P, p


def _colliders(n, channel=0):
    """n cells whose keys 2 i + channel topdown_slot sends to one slot, ascending."""
    first = slot_of(2 + channel)
    same = [i for i in range(1, 400000) if slot_of(2 * i + channel) == first][:n]
    assert len(same) == n
    return same


def colliding():
    """Five cells whose keys share a slot, interleaved pixel by pixel: the largest owns the slot, the others have none."""
    out = []
    for channel in (0, 1):
        same = _colliders(5, channel)
        out.append(keyed(np.array(same)[np.arange(9 * 40) % 5].reshape(9, 40), channel))
    return out


MIXED_W, MIXED_H, MIXED_ROWS = 64, 3 * (REGION // 64), REGION // 64       # three regions of REGION / 64 image rows each


def _mixed_cells():
    same = _colliders(2)
    a, b = same
    c = next(i for i in range(2, 20000) if slot_of(2 * i) != slot_of(2 * a))
    assert a < b and slot_of(2 * a) == slot_of(2 * b) != slot_of(2 * c)
    return a, b, c


def mixed_paths():
    """64 x 192, three regions of 64 image rows; cells a < b share a slot, c has another.  Cell a changes path from region to region, so its count
    receives the slot's flush of one workgroup and the no-slot adds of two others:
      region 0   a (columns 10..49 of rows 3..28) in c: a owns its slot
      region 1   a and b interleaved in runs of 1 to 5 pixels: b owns the slot, every run of a goes straight to the grid
      region 2   b in the left half, a in the right half but for the last column (c): a has no slot here either."""
    a, b, c = _mixed_cells()
    W, H, R = MIXED_W, MIXED_H, MIXED_ROWS
    ids = np.full((H, W), c, np.int64)
    ids[3:29, 10:50] = a
    rs = np.random.RandomState(12)
    runs = rs.randint(1, 6, REGION)
    ids[R:2 * R] = np.repeat(np.resize(np.array([a, b]), REGION), runs)[:REGION].reshape(R, W)
    ids[2 * R:, :W // 2] = b
    ids[2 * R:, W // 2:W - 1] = a
    return [keyed(ids)]


def owners(keys):
    """The keys that own a slot in a region holding `keys`: per slot the largest."""
    best = {}
    for k in set(int(v) for v in np.asarray(keys).reshape(-1) if v >= 0):
        best[slot_of(k)] = max(best.get(slot_of(k), -1), k)
    return set(best.values())


def check_mixed_paths_properties():
    """The placement, from the restatement of each region by itself."""
    a, b, c = _mixed_cells()
    depth, P, p = mixed_paths()[0]
    assert depth.shape == (MIXED_H, MIXED_W) and MIXED_W * MIXED_ROWS == REGION
    _, key = ref.classify(depth, P, p)
    part = [key[k * MIXED_ROWS:(k + 1) * MIXED_ROWS] for k in range(3)]
    assert [set(np.unique(q).tolist()) for q in part] == [{2 * a, 2 * c}, {2 * a, 2 * b}, {2 * a, 2 * b, 2 * c}]
    own = [owners(q) for q in part]
    assert 2 * a in own[0] and 2 * a not in own[1] and 2 * a not in own[2] and 2 * b in own[1] and 2 * b in own[2] and 2 * c in own[0] and 2 * c in own[2]
    n = [int((q == 2 * a).sum()) for q in part]
    assert min(n) > 0 and int(ref.topdown(depth[None], P[None], p)[0][0, a, 0]) == sum(n)
    return n


def check_pressure_properties():
    depth, P, p = own_cell()[0]
    cls, key = ref.classify(depth, P, p)
    assert (cls == 3).all() and len(np.unique(key)) == key.size and (key & 1).sum() > 0 and (key & 1 == 0).sum() > 0
    first = key.reshape(-1)[:REGION]
    assert len(owners(first)) <= SLOTS <= len(first) // 2                          # at least half the keys of a region own no slot
    for depth, P, p in colliding():
        _, key = ref.classify(depth, P, p)
        ks = np.unique(key)
        assert len(ks) == 5 and len({slot_of(k) for k in ks}) == 1
    for depth, P, p in wall():
        g, counts = ref.topdown(depth[None], P[None], p)
        assert 67 * 70 > REGION and counts.tolist() == [[0, 0, 0, 67 * 70]] and (g > 0).sum() == 1


# Borders: cells of 0.25 m from the origin, a_0 = b_1 = 0.25, depth 1: u = x + 4 c_0 and v = y + 4 c_1 exactly; h = 0.25 y - 0.5.
BORDER = ref.Params(nx=8, ny=10, origin_x=0.0, origin_y=0.0, cell_size=0.25, min_z=0.5, max_z=4.0, free_lo=-0.25, free_hi=0.25, occ_lo=0.5, occ_hi=1.5)


def borders():
    """[0] points exactly on cell borders, the last column at u == nx exactly; [1] u = x - 0.5: the first column slightly negative;
    [2] the same with v = y - 0.5; rows at h = -0.5, -0.25 (free_lo), 0, 0.25 (free_hi), 0.5 (occ_lo), 0.75, 1, 1.25, 1.5 (occ_hi), 1.75;
    [3] bands that overlap on [0.5, 0.75]: free wins."""
    on = [0.25, 0, 0, 0, 0.25, 0, 0, 0.25, -0.5, 0, 0, 0]
    neg_u = [0.25, 0, -0.125, 0, 0.25, 0, 0, 0.25, -0.5, 0, 0, 0]
    neg_v = [0.25, 0, 0, 0, 0.25, -0.125, 0, 0.25, -0.5, 0, 0, 0]
    return [_at_positions(9, 10, on, BORDER), _at_positions(9, 10, neg_u, BORDER), _at_positions(9, 11, neg_v, BORDER),
            _at_positions(9, 10, on, BORDER.but(free_hi=0.75))]


def check_border_properties():
    pics = borders()
    cls, key = ref.classify(*pics[0])
    assert (cls[:, 8] == 1).all() and (cls[:, :8] != 1).all()                        # u == nx is outside, u == 7 is cell 7
    rows = cls[:, 0].tolist()
    assert rows == [2, 3, 3, 3, 2, 3, 3, 3, 3, 2]                                     # h = occ_lo is NOT occupied; h = occ_hi, free_lo, free_hi are in
    assert (key[1:4, :8] & 1 == 0).all() and (key[5:9, :8] & 1 == 1).all() and (key[3, :8] >> 1 == 3 * 8 + np.arange(8)).all()
    cls, key = ref.classify(*pics[1])
    assert (cls[:, 0] == 1).all() and (cls[1, 1:] == 3).all() and (key[1, 1:] >> 1 == 8 + np.arange(8)).all()      # u = -0.5 is outside, u = 7.5 inside
    cls, key = ref.classify(*pics[2])
    assert (cls[0] == 1).all() and (cls[1:10, 8] == 1).all() and cls[8, 0] == 3 and key[8, 0] == 2 * 56 + 1      # v = -0.5 is outside, v = 7.5 is row 7
    cls, key = ref.classify(*pics[3])
    assert cls[:, 0].tolist() == [2, 3, 3, 3, 3, 3, 3, 3, 3, 2] and (key[4:6, :8] & 1 == 0).all() and (key[6, :8] & 1 == 1).all()


def depth_specials():
    """One row of depths: NaN of both signs, +-inf, +-0, a denormal, a negative, exactly min_z, exactly max_z, just outside both — under
    z in [0.5, 4], then under [0, +inf) (the zeros and the denormal enter: their point is t; +inf gives inf or NaN coordinates)."""
    nan_p, nan_n, den = np.uint32(0x7FC00000).view(F), np.uint32(0xFFC00000).view(F), np.uint32(1).view(F)
    d = np.array([[nan_p, nan_n, np.inf, -np.inf, 0.0, -0.0, den, -1.0, 0.5, 4.0, np.nextafter(F(0.5), F(0)), np.nextafter(F(4), F(5)), 1.0, 2.0]], F)
    P = [0.03125, 0, 0.0625, 0, 0, 0.25, 0, 0, 0, 0.125, 0.125, 0.0]
    p = ref.Params(nx=8, ny=8, origin_x=0.0, origin_y=0.0, cell_size=0.25, min_z=0.5, max_z=4.0)
    return [_at_positions(14, 1, P, p, d), _at_positions(14, 1, P, p.but(min_z=0.0, max_z=INF), d)]


def check_depth_specials_properties():
    (d, P, p), (_, _, q) = depth_specials()
    cls, _ = ref.classify(d, P, p)
    assert cls[0].tolist() == [0] * 8 + [3, 3, 0, 0, 3, 3]
    cls, _ = ref.classify(d, P, q)
    assert cls[0].tolist() == [0, 0, 1, 0, 3, 3, 3, 0, 3, 3, 3, 3, 3, 3]


def nan_matrix():
    """A P holding a NaN (in a_0, then in t_2 with everything else sound): every pixel is counts[1] or counts[0] (a_0), or counts[2] or
    counts[0] (t_2: inside, but a NaN height is in no band)."""
    d, P, p = seen_room(67, 5, 40)
    a, t = P.copy(), P.copy()
    a[0], t[11] = np.nan, np.nan
    return [(d, a, p), (d, t, p)]


SMALL = (sizes, wall, colliding, borders, depth_specials, nan_matrix)
LARGE = (three_regions, narrow, own_cell, mixed_paths)


def check_picture_properties():
    check_pressure_properties()
    check_mixed_paths_properties()
    check_border_properties()
    check_depth_specials_properties()
    for k, (d, P, p) in enumerate(nan_matrix()):
        g, counts = ref.topdown(d[None], P[None], p)
        assert g.sum() == 0 and counts[0, 3] == 0 and counts[0, 0] > 0 and counts[0, 2 if k else 1] > 0 and (k or counts[0, 2] == 0)
    total = np.zeros(4, np.int64)
    for d, P, p in sizes() + three_regions() + narrow():
        g, counts = ref.topdown(d[None], P[None], p)
        total += counts[0]
        assert d.size == 1 or (counts[0, 3] > d.size // 5 and g[..., 0].max() > 1), counts          # cells hit more than once: runs, slots
    assert (total > 0).all()                                                             # every class


# ---- the C ABI over plain buffers ---------------------------------------------------------------------------------------------------------
def c_params(p: ref.Params):
    from sage_gs import _capi
    return _capi.SgsTopdownParams(p.nx, p.ny, p.origin_x, p.origin_y, p.cell_size, p.min_z, p.max_z, p.free_lo, p.free_hi, p.occ_lo, p.occ_hi,
                                  p.flags, p.reserved)


class AbiTopdown(AbiDriver):
    """sgs_topdown_map and sgs_topdown_summary over host buffers; a GPU driver overrides the buffer hooks (GpuTopdown)."""

    def call(self, depth_ptr, W, H, n, stride, P_ptr, params, grid_ptr, counts_ptr, stream=None):
        cp = None if params is None else C.byref(params if not isinstance(params, ref.Params) else c_params(params))
        return int(self.lib.sgs_topdown_map(self.ctx, depth_ptr, int(W), int(H), int(n), int(stride), P_ptr, cp, grid_ptr, counts_ptr, stream))

    def call_summary(self, grid_ptr, nx, ny, min_hits, out_ptr, stream=None):
        return int(self.lib.sgs_topdown_summary(self.ctx, grid_ptr, int(nx), int(ny), int(min_hits), out_ptr, stream))

    def map(self, depth, P, p, stride=None, before=None, slack=64, stream=None):
        """depth fp32 [n,H,W], P fp32 [n,12] -> (grid uint32 [ny,nx,2], counts uint32 [n,4]).  grid holds `before` (default: 0xA5
        bytes) and out_counts 0xA5 bytes before the call, each with `slack` bytes behind it that must stay so.  stride: floats from
        frame to frame (default: a frame); the floats between frames are NaN and 1e30 in turn."""
        depth = np.asarray(depth, F)
        n, H, W = depth.shape
        st = H * W if stride is None else int(stride)
        keep_d, d_ptr = self._frames(jpeg_cases.strided(depth, st))
        keep_p, p_ptr = self._frames(np.asarray(P, F).reshape(n, 12))
        g_bytes, c_bytes = 8 * p.nx * p.ny, 16 * n
        keep_g, g_ptr, g_get = self._bytes(g_bytes + slack)
        if before is not None:
            self._fill(keep_g, np.ascontiguousarray(before, np.uint32).reshape(-1).view(np.uint8))
        keep_c, c_ptr, c_get = self._bytes(c_bytes + slack)
        self.lib.check(self.call(d_ptr, W, H, n, st, p_ptr, p, g_ptr, c_ptr, stream), self.ctx)
        self._sync()
        gb, cb = np.array(g_get()), np.array(c_get())
        assert (gb[g_bytes:] == SENTINEL).all(), "bytes were written behind the grid"
        assert (cb[c_bytes:] == SENTINEL).all(), "bytes were written behind out_counts"
        return gb[:g_bytes].view(np.uint32).reshape(p.ny, p.nx, 2), cb[:c_bytes].view(np.uint32).reshape(n, 4)

    def summary(self, grid, min_hits=1, slack=64):
        g = np.ascontiguousarray(grid, np.uint32)
        ny, nx = g.shape[:2]
        keep_g, g_ptr, _ = self._put(g)
        keep_o, o_ptr, o_get = self._bytes(32 + slack)
        self.lib.check(self.call_summary(g_ptr, nx, ny, min_hits, o_ptr), self.ctx)
        self._sync()
        ob = np.array(o_get())
        assert (ob[32:] == SENTINEL).all(), "bytes were written behind out"
        return [int(v) for v in ob[:32].view(np.uint64)]


class GpuTopdown(GpuBuffers, AbiTopdown):
    """AbiTopdown over torch device buffers, on a Renderer's context."""


def check_against(name, grid, counts, depth, P, p, before=None):
    """A call's grid and counters against the restatement; the assertions name the picture, the cell and the channel."""
    want, want_counts = ref.topdown(depth, P, p, grid=before)
    n, H, W = np.asarray(depth).shape
    assert counts.tolist() == want_counts.tolist(), f"{name}: counts are {counts.tolist()}, the restatement has {want_counts.tolist()}"
    assert (counts.astype(np.int64).sum(1) == H * W).all(), f"{name}: a frame's counters do not sum to its pixels"
    if not np.array_equal(grid, want):
        j, i, ch = (int(v[0]) for v in np.nonzero(grid != want))
        left = " (0xA5 bytes are left in it)" if int(grid[j, i, ch]) == POISON else ""
        raise AssertionError(f"{name}: cell ({i}, {j}) {'occupied' if ch else 'free'} is {int(grid[j, i, ch])}{left}, the restatement has {int(want[j, i, ch])}")
    if before is None or p.flags & ref.CLEAR:
        assert int(grid.astype(np.int64).sum()) == int(counts[:, 3].astype(np.int64).sum()), f"{name}: the grid's total is not the binned pixels"


def check_pictures(drv, makers):
    for make in makers:
        for k, (depth, P, p) in enumerate(make()):
            name = f"{make.__name__}[{k}] {depth.shape[1]}x{depth.shape[0]}"
            grid, counts = drv.map(depth[None], P[None], p)
            check_against(name, grid, counts, depth[None], P[None], p)


# ---- batches, accumulation, the split -------------------------------------------------------------------------------------------------------
def batch_frames():
    """Nine different 67 x 5 frames with nine different matrices, one grid."""
    pics = [seen_room(67, 5, 50 + k, pitch=-0.3 - 0.1 * k) for k in range(9)]
    depth, P = np.stack([q[0] for q in pics]), np.stack([q[1] for q in pics])
    assert len({d.tobytes() for d in depth}) == 9 and len({q.tobytes() for q in P}) == 9
    return depth, P, pics[0][2]


def check_batches(drv):
    """B = 1, 3 and 9 frames with a padded frame_stride whose padding is NaN and 1e30: the grid is the restatement's of those frames
    and every frame's counters are those of the frame alone; the order of the frames does not matter."""
    depth, P, p = batch_frames()
    alone = [drv.map(depth[k:k + 1], P[k:k + 1], p) for k in range(9)]
    for k in range(9):
        check_against(f"batch frame {k} alone", alone[k][0], alone[k][1], depth[k:k + 1], P[k:k + 1], p)
    for B in (1, 3, 9):
        for sel in (slice(0, B), slice(9 - B, 9)):
            grid, counts = drv.map(depth[sel], P[sel], p, stride=5 * 67 + 37)
            check_against(f"B = {B}, frames {list(range(9)[sel])}", grid, counts, depth[sel], P[sel], p)
            for j, k in enumerate(range(9)[sel]):
                assert counts[j].tolist() == alone[k][1][0].tolist(), f"B = {B}: the counters of frame {k} depend on the batch it is issued in"
            assert np.array_equal(grid, sum(alone[k][0].astype(np.uint64) for k in range(9)[sel]).astype(np.uint32))
    back, back_counts = drv.map(depth[::-1], P[::-1], p)
    whole, whole_counts = drv.map(depth, P, p)
    assert np.array_equal(back, whole) and np.array_equal(back_counts[::-1], whole_counts), "the grid depends on the order of the frames"


def check_accumulation(drv):
    """A two-call accumulation (CLEAR, then not) equals the one-call grid; CLEAR over a poisoned grid (every call of check_pictures is
    one) and over a known one; no CLEAR over a known grid adds to it."""
    depth, P, p = batch_frames()
    whole, whole_counts = drv.map(depth, P, p)
    check_against("one call", whole, whole_counts, depth, P, p)
    first, c1 = drv.map(depth[:4], P[:4], p)
    both, c2 = drv.map(depth[4:], P[4:], p.but(flags=0), before=first)
    assert np.array_equal(both, whole), "two accumulating calls differ from the one call"
    assert np.array_equal(np.concatenate([c1, c2]), whole_counts)
    known = (np.arange(2 * p.nx * p.ny, dtype=np.uint32) * 3).reshape(p.ny, p.nx, 2)
    grid, counts = drv.map(depth[:3], P[:3], p.but(flags=0), before=known)
    check_against("no CLEAR over a known grid", grid, counts, depth[:3], P[:3], p.but(flags=0), before=known)
    assert np.array_equal(grid.astype(np.int64) - known, ref.topdown(depth[:3], P[:3], p)[0])
    grid, counts = drv.map(depth[:3], P[:3], p, before=known)
    check_against("CLEAR over a known grid", grid, counts, depth[:3], P[:3], p, before=known)


def check_split(drv, chunk, n_frames=None):
    """2 * chunk + 3 frames of 1 x 1 in one call (chunk: SGS_TOPDOWN_MAX_FRAMES of the library driven): two full launches and a short
    one, each with depth, pix_to_map and out_counts re-based and the grid not.  Frame f's point is t = (0.25 (f % 13), 0.25 (f % 4),
    0.5 (f % 3)) plus its depth (1, 2, 9 > max_z, NaN in turn) along x; frame_stride 3."""
    n = 2 * chunk + 3 if n_frames is None else int(n_frames)
    assert n > chunk
    f = np.arange(n)
    depth = np.array([1, 2, 9, np.nan, 0.5], F)[f % 5].reshape(n, 1, 1)
    P = np.zeros((n, 12), F)
    P[:, 2] = 0.25
    P[:, 9], P[:, 10], P[:, 11] = 0.25 * (f % 13), 0.25 * (f % 4), 0.5 * (f % 3)
    p = ref.Params(nx=16, ny=5, origin_x=0.0, origin_y=0.0, cell_size=0.25, max_z=4.0)
    grid, counts = drv.map(depth, P, p, stride=3)
    period = 13 * 4 * 3 * 5
    per = [ref.topdown(depth[k:k + 1], P[k:k + 1], p) for k in range(min(n, period))]
    want_counts = np.stack([q[1][0] for q in per])[f % period]
    times = np.bincount(f % period, minlength=period)
    want = sum(int(times[k]) * per[k][0].astype(np.int64) for k in range(len(per))).astype(np.uint32)
    same = (counts == want_counts).all(1)
    if not same.all():
        k = int(np.argmin(same))
        raise AssertionError(f"split: frame {k} of {n} (launches of {chunk}): counts are {counts[k].tolist()}, the restatement has {want_counts[k].tolist()}")
    if not np.array_equal(grid, want):
        j, i, ch = (int(v[0]) for v in np.nonzero(grid != want))
        raise AssertionError(f"split: {n} frames (launches of {chunk}): cell ({i}, {j}) {'occupied' if ch else 'free'} is {int(grid[j, i, ch])}, the restatement has {int(want[j, i, ch])}")
    assert want_counts[:, 3].sum() > n // 3 and (want[..., 1] > 0).any() and (want[..., 0] > 0).any()
    return n


def summary_grids():
    rs = np.random.RandomState(3)
    small = rs.randint(0, 6, (7, 9, 2)).astype(np.uint32)                              # hits on both sides of min_hits = 3
    huge = rs.randint(2 ** 31, 2 ** 32, (5, 13, 2), dtype=np.int64).astype(np.uint32)  # sums far past 2^32
    ny, nx = 401, 700
    assert nx * ny > SUM_BLOCKS * THREADS and (nx * ny) % 64 != 0                     # the reduction strides, and its last wave is ragged
    wide = (rs.randint(0, 40, (ny, nx, 2)) * (rs.rand(ny, nx, 2) < 0.3)).astype(np.uint32)
    return {"small": small, "huge": huge, "wide": wide, "one cell": np.array([[[2, 0]]], np.uint32), "full": np.full((3, 2, 2), 0xFFFFFFFF, np.uint32)}


def check_summary(drv):
    for name, g in summary_grids().items():
        for min_hits in (1, 3, 2 ** 32 - 1):
            got, want = drv.summary(g, min_hits), ref.summary(g, min_hits)
            assert got == want, f"summary of {name} at min_hits = {min_hits}: {got}, the restatement has {want}"
    s = ref.summary(summary_grids()["small"], 3)
    assert 0 < s[0] and 0 < s[1] and s[0] + s[1] < 63 and ref.summary(summary_grids()["huge"], 1)[2] > 2 ** 32


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def check_refusals(drv):
    """Every refusal of the header returns SGS_ERR_INVALID with a message that names the argument and leaves the poisoned outputs
    untouched; then the context still works."""
    p = ref.Params(nx=4, ny=3, origin_x=0.0, origin_y=0.0, cell_size=0.25)
    keep_d, d_ptr = drv._frames(np.ones(2 * 64 + 64, F))
    keep_p, p_ptr = drv._frames(np.zeros(24 + 16, F))
    keep_g, g_ptr, g_get = drv._bytes(8 * 12 + 64)
    keep_c, c_ptr, c_get = drv._bytes(2 * 16 + 64)
    keep_o, o_ptr, o_get = drv._bytes(32 + 64)
    nan = float("nan")

    def call(depth=d_ptr, W=8, H=8, n=2, stride=64, P=p_ptr, params=p, grid=g_ptr, counts=c_ptr, **kw):
        return drv.call(depth, W, H, n, stride, P, params.but(**kw) if kw else params, grid, counts)

    bad = [(b"null depth", dict(depth=None)), (b"null pix_to_map", dict(P=None)), (b"null params", dict(params=None)), (b"null grid", dict(grid=None)),
           (b"null out_counts", dict(counts=None)), (b"n_frames = 0", dict(n=0)), (b"n_frames = -1", dict(n=-1)), (b"frame 8 x 0", dict(H=0)),
           (b"frame 0 x 8", dict(W=0)), (b"frame -8 x 8", dict(W=-8)), (b"more than 2^31 - 1 pixels", dict(H=65536, W=32768, stride=2 ** 31, n=1)),
           (b"frame_stride", dict(stride=63)), (b"frame_stride", dict(n=1, stride=63)),
           (b"n_frames * height * width", dict(n=5, H=32768, W=32768, stride=2 ** 30)), (b"n_frames * height * width", dict(n=4, H=32768, W=32768, stride=2 ** 30)),
           (b"nx = 0", dict(nx=0)), (b"ny = -3", dict(ny=-3)), (b"nx = 32768, ny = 32768", dict(nx=32768, ny=32768)),
           (b"cell_size", dict(cell_size=0.0)), (b"cell_size", dict(cell_size=-0.25)), (b"cell_size", dict(cell_size=nan)), (b"cell_size", dict(cell_size=INF)),
           (b"origin", dict(origin_x=nan)), (b"origin", dict(origin_y=-INF)), (b"min_z", dict(min_z=2.0, max_z=1.0)), (b"min_z", dict(min_z=nan)),
           (b"max_z", dict(max_z=nan)), (b"free band", dict(free_lo=0.5, free_hi=0.25)), (b"free band", dict(free_lo=-INF)), (b"free band", dict(free_hi=nan)),
           (b"occupied band", dict(occ_lo=2.0, occ_hi=1.5)), (b"occupied band", dict(occ_hi=INF)), (b"occupied band", dict(occ_lo=nan)),
           (b"unknown flags", dict(flags=2)), (b"unknown flags", dict(flags=0x80000001)), (b"reserved", dict(reserved=1))]
    for word, kw in bad:
        assert call(**kw) == -1, f"{word.decode()} with {kw} was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"sgs_topdown_map" in msg, (word, msg)
    bad = [(b"null grid", dict(grid=None)), (b"null out", dict(out=None)), (b"nx = 0", dict(nx=0)), (b"ny = -1", dict(ny=-1)),
           (b"nx = 32768, ny = 32768", dict(nx=32768, ny=32768)), (b"min_hits = 0", dict(min_hits=0))]

    def call_s(grid=g_ptr, nx=4, ny=3, min_hits=1, out=o_ptr):
        return drv.call_summary(grid, nx, ny, min_hits, out)

    for word, kw in bad:
        assert call_s(**kw) == -1, f"{word.decode()} with {kw} was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"sgs_topdown_summary" in msg, (word, msg)
    drv._sync()
    for get, what in ((g_get, "the grid"), (c_get, "out_counts"), (o_get, "out")):
        assert (np.array(get()) == SENTINEL).all(), f"a refused call wrote to {what}"
    assert call() == 0 and call_s() == 0 and call(max_z=INF, min_z=-INF) == 0          # the context still works; an unbounded range is no error
    drv._sync()
    assert np.array(c_get())[:32].view(np.uint32).tolist() == [0, 0, 0, 64] * 2 and np.array(g_get())[:96].view(np.uint32).sum() == 128


def check_misaligned(drv):
    """depth, pix_to_map, grid and out_counts 1 and 2 bytes off their 4-byte alignment, sgs_topdown_summary's grid likewise and its
    out 4 bytes off its 8: each is refused with SGS_ERR_INVALID and a message that names the argument, before anything is enqueued —
    the poisoned outputs stay untouched."""
    p = ref.Params(nx=4, ny=3, origin_x=0.0, origin_y=0.0, cell_size=0.25)
    pad = 16
    keep_d, d_ptr = drv._frames(np.ones(2 * 64 + pad, F))
    keep_p, p_ptr = drv._frames(np.zeros(24 + pad, F))
    keep_g, g_ptr, g_get = drv._bytes(8 * 12 + 4 * pad)
    keep_c, c_ptr, c_get = drv._bytes(2 * 16 + 4 * pad)
    keep_o, o_ptr, o_get = drv._bytes(32 + 4 * pad)
    assert all(v % 8 == 0 for v in (d_ptr, p_ptr, g_ptr, c_ptr, o_ptr))

    def call(depth=0, P=0, grid=0, counts=0):
        return drv.call(d_ptr + depth, 8, 8, 2, 64, p_ptr + P, p, g_ptr + grid, c_ptr + counts)

    def call_s(grid=0, out=0):
        return drv.call_summary(g_ptr + grid, 4, 3, 1, o_ptr + out)

    bad = [(call, word, {arg: off}) for word, arg in ((b"depth", "depth"), (b"pix_to_map", "P"), (b"grid", "grid"), (b"out_counts", "counts")) for off in (1, 2)]
    bad += [(call_s, b"grid", dict(grid=1)), (call_s, b"grid", dict(grid=2)), (call_s, b"out", dict(out=4)), (call_s, b"out", dict(out=2))]
    for fn, word, kw in bad:
        assert fn(**kw) == -1, f"{word.decode()} off by {kw} bytes was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"aligned" in msg, (word, msg)
    drv._sync()
    for get, what in ((g_get, "the grid"), (c_get, "out_counts"), (o_get, "out")):
        assert (np.array(get()) == SENTINEL).all(), f"a refused call wrote to {what}"
    assert call() == 0 and call(depth=4, P=4, grid=4, counts=4) == 0 and call_s(grid=4, out=8) == 0      # aligned, and aligned again
    drv._sync()
    assert np.array(c_get())[4:36].view(np.uint32).tolist() == [0, 0, 0, 64] * 2
    assert np.array(o_get())[8:40].view(np.uint64).tolist() == [0, 1, 128, 0]


# ---- rendered frames ----------------------------------------------------------------------------------------------------------------------
ROOM_POSES = ((2.0, 2.5, 0.3, -0.5), (3.5, 1.8, 2.2, -0.7), (4.2, 3.4, 4.0, -0.35), (1.6, 3.3, 5.5, -0.9), (3.0, 2.5, 1.2, -1.3))      # x, y, yaw, pitch
ROOM_GRID = ref.Params(nx=160, ny=140, origin_x=-1.0, origin_y=-1.0, cell_size=0.05)


def room_cameras(W, H):
    """(sage_gs Cameras, P fp32 [n,12]) of ROOM_POSES at eye height, the reference's lens."""
    from sage_gs import Camera, scenes
    fx, fy, cx, cy = scenes.reference_intrinsics(W, H)
    cams = [Camera(W, H, fx, fy, cx, cy, look((x, y, 1.2), yaw, pitch)) for x, y, yaw, pitch in ROOM_POSES]
    P = np.stack([ref.pix_to_map(fx, fy, cx, cy, c.view) for c in cams])
    return cams, P


def check_rendered(drv, render, W=160, H=120):
    """render(cameras) -> depth fp32 [n,H,W] of scenes.make_room_mesh(2000) (a 6 x 5 m room, world coordinates, z up) from ROOM_POSES:
    grid and counters equal the restatement, the counter identity holds, and no hit lies outside the room's footprint grown by a cell."""
    cams, P = room_cameras(W, H)
    depth = np.asarray(render(cams), F)
    assert depth.shape == (len(cams), H, W) and np.isfinite(depth).mean() > 0.9
    p = ROOM_GRID
    grid, counts = drv.map(depth, P, p)
    check_against(f"rendered {W}x{H}", grid, counts, depth, P, p)
    assert (counts[:, 3] > W * H // 4).all() and (grid[..., 0] > 0).sum() > 200 and (grid[..., 1] > 0).sum() > 200, counts
    js, is_ = np.nonzero(grid.sum(-1))
    x0, x1, y0, y1 = (p.origin_x + is_.min() * p.cell_size, p.origin_x + (is_.max() + 1) * p.cell_size,
                      p.origin_y + js.min() * p.cell_size, p.origin_y + (js.max() + 1) * p.cell_size)
    c = p.cell_size + 1e-6
    assert x0 >= -c and y0 >= -c and x1 <= 6.0 + c and y1 <= 5.0 + c, f"hits outside the room's footprint: x {x0:.3f}..{x1:.3f}, y {y0:.3f}..{y1:.3f}"
    return grid, counts
