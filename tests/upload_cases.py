"""The scene upload's results — the Z-order permutation (SGS_BUF_SCENE_PERM) and the per-chunk bounds (SGS_BUF_CHUNK_BOUNDS) — held against
tests/upload_ref.py.  Written once and run twice: under the wave64 emulator (test_emu_upload.py, and on seeded faults in
test_emu_upload_mutants.py) and on an MI355X (test_gpu_upload.py).

A frame does not depend on the layout (parity_cases.case_tiling_does_not_depend_on_the_layout), so a wrong upload kernel costs speed and
no pixel: these cases are what sees one.  Every case uploads, renders one 48x32 frame, reads the two buffers, compares them with the
restatement, and asserts that the frame equals the frame of the same scene uploaded with sgs_tuning.morton = 0, bit for bit.

The sizes are the smallest at which each mechanism of the sort exists: its tile is 2048 keys (SGS_RSORT_TILE), a wave owns 512 of them and
walks 64 at a time; k_radix_scan spans 4096 counters (SGS_RSCAN_SPAN) = 16 sort tiles, so at 17 tiles the span sums come into play and one
digit's counters straddle two spans; k_mean_bounds starts at most 512 workgroups of 256 and strides from 131 073 Gaussians on.

A `drv` offers upload(...), upload_compressed(chunks, packed, sh, deg, sh_decode=None), render(cam, stats=False) -> (image, stats),
debug(what, dtype), scene_geom(), chunk_skipped(), set_tuning(morton=...), tuning().
"""
import os
import tempfile

import numpy as np

import oracle_np as onp
import parity_cases as pc
import upload_ref as ur
from sage_gs import _capi

Q = 2097151                                  # 2^21 - 1: the lattice [0, Q]^3 with both corners present has inv == 1.0f, cell == coordinate
W, H = 48, 32
SIZES = (64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, 32768, 32769, 40000, 131073)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------

def _extent(means):
    lo, hi = ur.mean_bounds(means)
    with np.errstate(invalid="ignore"):
        ext = float(np.nanmax(np.where(np.isnan(hi - lo), 0.0, hi - lo)))
    mid = np.where(np.isnan(lo), 0.0, 0.5 * (lo.astype(np.float64) + hi.astype(np.float64)))
    return (ext if ext > 0 else 1.0), mid


def scene_of(means, seed=0):
    """The rest of a degree-0 scene around `means`: scales of 0.2 % to 2 % of the extent (they differ inside every chunk: s_max), upright."""
    means = np.ascontiguousarray(means, np.float32)
    n = len(means)
    rng = np.random.default_rng(1000 + seed)
    ext, _ = _extent(means)
    scales = (ext * np.exp(rng.uniform(np.log(0.002), np.log(0.02), (n, 3)))).astype(np.float32)
    quats = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    opac = rng.uniform(0.2, 1.0, n).astype(np.float32)
    sh = rng.uniform(-1, 1, (n, 1, 3)).astype(np.float32)
    return means, scales, quats, opac, sh, 0


def camera_for(means):
    """48x32, looking along +z at the middle of the finite means from 1.5 extents in front of it."""
    ext, mid = _extent(means)
    view = np.eye(4, dtype=np.float64)
    view[:3, 3] = -(mid - np.array([0.0, 0.0, 1.5 * ext + 1.0]))
    return onp.Camera(W, H, 40.0, 40.0, W / 2.0, H / 2.0, view.astype(np.float32))


def lattice(n, seed, pool=0.5):
    """n integer points of [0, Q]^3 with the two corners present; `pool` of them drawn from 37 points (equal keys: stability shows)."""
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, Q + 1, (n, 3))
    few = rng.integers(0, Q + 1, (37, 3))
    dup = rng.random(n) < pool
    pts[dup] = few[rng.integers(0, 37, int(dup.sum()))]
    return with_corners(pts)


def with_corners(pts):
    pts = np.array(pts, np.int64)
    if len(pts) >= 2:
        k = len(pts) // 3
        pts[k], pts[-1 - k] = (Q, Q, Q), (0, 0, 0)              # (the greater corner first: the input is not sorted)
    return pts.astype(np.float32)


def from_keys(keys):
    """Lattice points with exactly these Morton codes, plus the two corners at the end (greater first)."""
    keys = np.concatenate([np.asarray(keys, np.uint64), np.array([(1 << 63) - 1, 0], np.uint64)])
    return ur.deinterleave(keys).astype(np.float32)


# ---- the checks --------------------------------------------------------------------------------------------------------------------------

def read_upload(drv):
    return drv.debug(_capi.BUF_SCENE_PERM, np.uint32), drv.debug(_capi.BUF_CHUNK_BOUNDS, np.float32).reshape(-1, 8)


def check_perm(perm, means, what, sorted_=True):
    """The permutation of the last rendered scene against the stable sort of the restatement's keys."""
    n = len(means)
    assert perm.shape == (n,), f"{what}: permutation: {perm.shape} for {n} Gaussians"
    want = ur.expected_perm(means, sorted_)
    if np.array_equal(perm, want):
        return want
    keys = ur.morton_keys(means)
    assert np.array_equal(np.sort(perm), np.arange(n)), \
        f"{what}: permutation: not a permutation ({n - len(np.unique(perm))} of {n} indices missing)"
    p = int(np.nonzero(perm != want)[0][0])
    order = keys[perm]
    asc = bool((order[1:] >= order[:-1]).all())
    raise AssertionError(f"{what}: permutation: differs from the stable sort of the restatement's keys at {int((perm != want).sum())} of {n} positions "
                         f"(keys ascending: {asc}); first at position {p}: Gaussian {perm[p]} (key {int(keys[perm[p]]):#x}), expected "
                         f"{want[p]} (key {int(keys[want[p]]):#x})")


def check_upload(drv, means, scales, what, sorted_=True):
    perm, cb = read_upload(drv)
    check_perm(perm, means, what, sorted_)
    held = ur.check_chunk_bounds(means[perm], scales[perm], cb, what)
    return perm, cb, held


def run_scene(drv, scene, what, cam=None, finite_frame=True):
    """Upload (morton = 1), one frame, the two buffers against the restatement; the same in the caller's order (morton = 0: the identity,
    and the bounds of the chunks of THAT order); the two frames equal bit for bit.  Returns (perm, chunk bounds, frame, stats)."""
    means, scales = scene[0], scene[1]
    cam = camera_for(means) if cam is None else cam
    keep = drv.tuning()["morton"]
    assert keep == 1, "the library's default is a sorted upload"
    try:
        drv.upload(*scene)
        img, st = drv.render(cam, stats=False)
        perm, cb, held = check_upload(drv, means, scales, what, sorted_=True)
        drv.set_tuning(morton=0)
        drv.upload(*scene)
        img0, st0 = drv.render(cam, stats=False)
        check_upload(drv, means, scales, f"{what}, morton = 0", sorted_=False)
    finally:
        drv.set_tuning(morton=keep)
    assert st["n_gaussians"] == len(means)
    if finite_frame:
        assert np.isfinite(img).all(), f"{what}: frame: not finite"
    assert (st["n_visible"], st["d_total"]) == (st0["n_visible"], st0["d_total"]) and \
        np.array_equal(np.ascontiguousarray(img).view(np.uint32), np.ascontiguousarray(img0).view(np.uint32)), \
        f"{what}: frame: differs from the frame of the scene uploaded with morton = 0"
    return perm, cb, img, st


def run_means(drv, means, what, seed=0):
    return run_scene(drv, scene_of(means, seed), what)


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------

def case_size(drv, n):
    """A lattice scene of n Gaussians, half of them on 37 points: the sort at this size, and its stability.  64: not sorted."""
    means = lattice(n, seed=n)
    perm, cb, img, st = run_means(drv, means, f"size {n}", seed=n)
    if n <= 64:
        assert np.array_equal(perm, np.arange(n)), f"size {n}: permutation: a scene of one chunk is not sorted"
    else:
        assert not np.array_equal(perm, np.arange(n))
    assert st["n_visible"] > 0 and img.max() > 0.0            # (the frame shows the scene: the comparison of frames compares something)


# ---- lattice keys: independent of how a division rounds -----------------------------------------------------------------------------------

def case_one_digit(drv, j):
    """Keys that differ only in radix digit j (bits 8 j .. 8 j + 7; digit 7 has 7 bits): every value of the digit, shuffled, most twice."""
    rng = np.random.default_rng(40 + j)
    nv = 128 if j == 7 else 256
    base = np.uint64(0x0123456789ABCDEF & ((1 << 63) - 1) & ~(0xFF << (8 * j)))
    v = np.concatenate([rng.permutation(nv), rng.permutation(nv)[: nv // 2 + 11]]).astype(np.uint64)
    means = from_keys(base | (v << np.uint64(8 * j)))
    assert np.array_equal(ur.morton_keys(means)[:-2], base | (v << np.uint64(8 * j)))
    run_means(drv, means, f"keys that differ in digit {j} only", seed=j)


def case_key_bit_62(drv):
    """Pairs of keys that differ in bit 62 alone (the top bit of z), the greater first: only the eighth pass orders them."""
    rng = np.random.default_rng(62)
    low = rng.integers(0, 1 << 62, 700, dtype=np.uint64)
    keys = np.stack([low | np.uint64(1 << 62), low], 1).reshape(-1)
    means = from_keys(keys)
    perm, _, _, _ = run_means(drv, means, "key bit 62")
    k = ur.morton_keys(means)[perm]
    assert (k[: len(k) // 2] >> np.uint64(62) == 0).all() and (k[len(k) // 2:] >> np.uint64(62) == 1).all()


def case_rows_of_lanes(drv, j):
    """Rows of 64 lanes (a wave's step through its quarter of a tile) that share digit j — one run of 64 peers — and rows whose 64 lanes
    hold 64 different values of it — 64 runs of one; the other bits random."""
    rng = np.random.default_rng(70 + j)
    n = 2 * 2048 + 640
    keys = rng.integers(0, 1 << 63, n, dtype=np.uint64) & ~np.uint64(0xFF << (8 * j))
    row, lane = np.arange(n) // 64, np.arange(n) % 64
    nv = 128 if j == 7 else 256
    same = (row * 37) % nv
    different = (lane * (nv // 64) + row) % nv
    digit = np.where(row % 2 == 0, same, different).astype(np.uint64)
    means = from_keys(keys | (digit << np.uint64(8 * j)))
    run_means(drv, means, f"rows of lanes on one value / on 64 values of digit {j}", seed=j)


# ---- stability ----------------------------------------------------------------------------------------------------------------------------

def case_every_mean_equal(drv):
    n = 2 * 2048 + 777
    means = np.tile(np.array([0.25, -1.5, 7.0], np.float32), (n, 1))
    perm, cb, _, _ = run_means(drv, means, "every mean equal")
    assert np.array_equal(perm, np.arange(n)), "every mean equal: permutation: not the identity"


def case_two_points_interleaved(drv):
    """A and B (key 0 and key 2^63 - 1) interleaved so that both occur in every wave quarter of every tile: A's indices ascending, then B's."""
    n = 3 * 2048 + 100
    is_b = (np.arange(n) * 7 % 5) < 2                        # B A A B A | B ... : both within any 5 consecutive inputs
    means = np.where(is_b[:, None], np.float32(Q), np.float32(0)) * np.ones((1, 3), np.float32)
    for t0 in range(0, n, 512):                             # (every wave quarter of every tile holds both)
        assert is_b[t0: t0 + 512].any() and not is_b[t0: t0 + 512].all()
    perm, _, _, _ = run_means(drv, means, "two points interleaved")
    want = np.concatenate([np.nonzero(~is_b)[0], np.nonzero(is_b)[0]])
    assert np.array_equal(perm, want), "two points interleaved: permutation: not A's indices ascending, then B's"


def case_degenerate_axis(drv):
    means = lattice(3000, seed=91)
    means[:, 1] = 12345.0
    assert (ur.axis_cells(means)[:, 1] == 0).all()
    run_means(drv, means, "one degenerate axis")


# ---- real coordinates: these rest on a correctly rounded fp32 division -----------------------------------------------------------------------

def cloud(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-3.1, 2.7, n), rng.uniform(-1.9, 0.4, n), rng.uniform(-7.5, -2.2, n)], 1).astype(np.float32)


def case_random_cloud(drv):
    means = cloud(5000, 5)
    assert (means < 0).any(axis=0).all()
    run_means(drv, means, "random cloud with negative coordinates")


def case_signed_zeros(drv):
    """-0.0 and +0.0 on an otherwise constant axis: the axis has no extent (hi > lo is false), whichever zero the bounds kept."""
    means = cloud(3000, 6)
    means[:, 0] = np.where(np.arange(3000) % 3 == 0, np.float32(-0.0), np.float32(0.0))
    assert np.signbit(means[:, 0]).any() and not np.signbit(means[:, 0]).all()
    assert (ur.axis_cells(means)[:, 0] == 0).all()
    run_means(drv, means, "-0.0 and +0.0 on a constant axis")


# ---- non-finite means -----------------------------------------------------------------------------------------------------------------------

WILD = (np.nan, np.inf, -np.inf, 3.0e38, -3.0e38)


def case_non_finite_means(drv):
    """NaN, +-inf and +-3.0e38f in single coordinates of a few Gaussians: the bounds and the others' keys do not move, their own axis key is
    0, a chunk that holds one is never culled (R = +inf), the frame is finite."""
    n = 3000
    clean = cloud(n, 7)
    means = clean.copy()
    where = [(17 + 211 * k, k % 3) for k in range(14)]
    for k, (i, c) in enumerate(where):
        means[i, c] = WILD[k % len(WILD)]
    means[1500, :] = np.nan                                   # ... and one with no finite coordinate at all
    touched = np.array([i for i, _ in where] + [1500])
    # (the restatement itself: bounds and the others' keys unchanged, the wild coordinates' own cell 0)
    lo, hi = ur.mean_bounds(means)
    for c in range(3):
        tame = np.setdiff1d(np.arange(n), [i for i, cc in where if cc == c] + [1500])
        assert lo[c] == clean[tame, c].min() and hi[c] == clean[tame, c].max()
    others = np.setdiff1d(np.arange(n), touched)
    assert np.array_equal(ur.morton_keys(means)[others], ur.interleave(ur.axis_cells(clean, lo, hi))[others])
    assert all(ur.axis_cells(means)[i, c] == 0 for i, c in where) and ur.morton_keys(means)[1500] == 0
    scene = scene_of(means, 7)
    perm, cb, img, st = run_scene(drv, scene, "non-finite means")
    assert st["n_visible"] > 0 and img.max() > 0.0
    chunk_of = np.empty(n, np.int64); chunk_of[perm] = np.arange(n) // 64
    kept = np.zeros(len(cb), bool); kept[chunk_of[touched]] = True
    assert np.array_equal(np.isposinf(cb[:, 3]), kept), "non-finite means: chunk bounds: R = +inf in exactly the chunks that hold a wild mean"


def case_finite_outlier(drv):
    """One finite outlier at 1e30: it IS in the bounds (every other cell of its axis collapses to 0 or thereabouts); the restatement
    decides the keys.  Its chunk's fp32 squared distance overflows: R = +inf."""
    means = cloud(3000, 8)
    means[1234, 2] = 1.0e30
    scene = list(scene_of(cloud(3000, 8), 8)); scene[0] = means
    cam = camera_for(cloud(3000, 8))
    perm, cb, img, st = run_scene(drv, tuple(scene), "finite outlier at 1e30", cam=cam)
    assert int(np.isposinf(cb[:, 3]).sum()) == 1 and np.isposinf(cb[int(np.nonzero(perm == 1234)[0][0]) // 64, 3])


# ---- the compressed path: k_mean_bounds<true>, k_morton_keys<true> ---------------------------------------------------------------------------

def case_compressed(drv):
    """A quantised scene of 5000 Gaussians through upload_compressed; the restatement runs on the positions (and scales) the device holds
    (SGS_BUF_SCENE_GEOM)."""
    from sage_gs import ply
    n = 5000
    means, scales, quats, opac, sh, deg = scene_of(cloud(n, 9), 9)
    cam = camera_for(means)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene.ply")
        ply.save_compressed_ply(path, means, scales, quats, opac, sh, deg)
        payload = ply.read_compressed_payload(path)
    keep = drv.tuning()["morton"]
    got = {}
    try:
        for morton in (1, 0):
            drv.set_tuning(morton=morton)
            drv.upload_compressed(*payload)
            img, st = drv.render(cam, stats=False)
            g = drv.scene_geom()
            assert g.shape == (n, 11) and np.abs(g[:, 0:3] - means).max() < 0.01
            what = f"compressed upload, morton = {morton}"
            perm, cb, held = check_upload(drv, g[:, 0:3].copy(), g[:, 4:7].copy(), what, sorted_=bool(morton))
            assert held == len(cb)
            got[morton] = (img, st["n_visible"], st["d_total"], perm)
    finally:
        drv.set_tuning(morton=keep)
    assert not np.array_equal(got[1][3], np.arange(n))
    assert got[1][1:3] == got[0][1:3] and got[1][1] > 0 and np.array_equal(got[1][0].view(np.uint32), got[0][0].view(np.uint32)), \
        "compressed upload: frame: differs from the frame of the scene uploaded with morton = 0"


# ---- effect: what the order is for -------------------------------------------------------------------------------------------------------------

def case_effect(drv, n=6000, res=(208, 150)):
    """parity_cases.case_chunk_bounds' scene (a wall ten times the view, in random order): the expected permutation, tight bounds, and
    more chunks skipped in Z-order than in the caller's order."""
    scene, cam = pc.chunk_bounds_scene(n, res)
    keep = drv.tuning()["morton"]
    skipped, frames = {}, {}
    try:
        for morton in (1, 0):
            drv.set_tuning(morton=morton)
            drv.upload(*scene)
            frames[morton], _ = drv.render(cam, stats=False)
            check_upload(drv, scene[0], scene[1], f"case_chunk_bounds' scene, morton = {morton}", sorted_=bool(morton))
            skipped[morton] = int(drv.chunk_skipped().sum())
    finally:
        drv.set_tuning(morton=keep)
    assert np.array_equal(frames[1].view(np.uint32), frames[0].view(np.uint32)), "effect: frame: differs from the frame of the scene uploaded with morton = 0"
    assert skipped[1] > skipped[0], f"effect: {skipped[1]} chunks skipped in Z-order, {skipped[0]} in the caller's (random) order"
    assert skipped[1] > 0.4 * ((n + 63) // 64), skipped
    return skipped


CASES = {f"size_{n}": (lambda drv, n=n: case_size(drv, n)) for n in SIZES}
CASES.update({f"one_digit_{j}": (lambda drv, j=j: case_one_digit(drv, j)) for j in range(8)})
CASES.update({
    "key_bit_62": case_key_bit_62,
    "rows_of_lanes_digit_0": lambda drv: case_rows_of_lanes(drv, 0),
    "rows_of_lanes_digit_5": lambda drv: case_rows_of_lanes(drv, 5),
    "every_mean_equal": case_every_mean_equal,
    "two_points_interleaved": case_two_points_interleaved,
    "degenerate_axis": case_degenerate_axis,
    "random_cloud": case_random_cloud,
    "signed_zeros": case_signed_zeros,
    "non_finite_means": case_non_finite_means,
    "finite_outlier": case_finite_outlier,
    "compressed": case_compressed,
    "effect": case_effect,
})
