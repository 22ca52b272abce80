"""A plain NumPy restatement of what a scene upload computes (csrc/sgs_kernels.h "Upload": k_mean_bounds, k_morton_keys, the radix sort,
k_chunk_bounds) — test infrastructure only; imports nothing of the product.

  bounds        per axis, min and max over the coordinates with |m| < 3.0e38f
  keys          21 bits per axis over those bounds, computed in np.float32 step by step as the kernel does (one correctly rounded
                division, one subtraction, one product: nothing a compiler could contract into an fma), interleaved x, y, z at bits
                0, 1, 2 by a plain loop over the 21 bits
  permutation   np.argsort(keys, kind="stable"): layout position -> original index
  chunk bounds  per 64 consecutive Gaussians of the layout: centre = 0.5f (lo + hi) and s_max, both exact in fp32 and compared bit for
                bit; the radius R by two inequalities against the fp64 distance d of the farthest member from the STORED centre
"""
import numpy as np

F = np.float32
LIMIT = F(3.0e38)                # a coordinate at or beyond it (or NaN) takes no part in the bounds; its axis key is 0
QMAX = F(2097151.0)              # 2^21 - 1
R_KEEP = 3.0e37                  # a radius or a scale at or above it: R = +inf (the chunk is never culled)
# The kernel forms the distance as sqrtf(dx^2 + dy^2 + dz^2) in fp32: above sqrt(FLT_MAX) = 1.8447e19 the squares overflow and R = +inf
# is the only outcome (conservative).  Between the two figures below (sum of squares within 6 % of FLT_MAX) either outcome is accepted.
D_SQUARES_FIT, D_SQUARES_OVERFLOW = 1.8e19, 1.9e19


def finite_mask(means):
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(means, F)) < LIMIT          # (NaN compares False)


def mean_bounds(means):
    """(lo [3], hi [3]) in fp32 over the coordinates with |m| < 3.0e38f; NaN, NaN for an axis without one."""
    m = np.asarray(means, F).reshape(-1, 3)
    ok = finite_mask(m)
    lo, hi = np.full(3, np.nan, F), np.full(3, np.nan, F)
    for c in range(3):
        v = m[ok[:, c], c]
        if len(v):
            lo[c], hi[c] = v.min(), v.max()
    return lo, hi


def axis_cells(means, lo=None, hi=None):
    """uint64 [N, 3]: the 21-bit cell of every coordinate."""
    m = np.asarray(means, F).reshape(-1, 3)
    if lo is None:
        lo, hi = mean_bounds(m)
    ok = finite_mask(m)
    q = np.zeros(m.shape, np.uint64)
    with np.errstate(all="ignore"):
        for c in range(3):
            inv = QMAX / F(hi[c] - lo[c]) if hi[c] > lo[c] else F(0.0)            # (NaN bounds: False, 0)
            assert isinstance(inv, F)
            u = (m[:, c] - lo[c]) * inv
            assert u.dtype == F
            u = np.where(ok[:, c], u, F(0.0))
            u = np.fmin(QMAX, np.fmax(F(0.0), u))                                  # fmaxf(0, NaN) = 0, as the kernel's
            q[:, c] = u.astype(np.uint64)                                          # truncation
    return q


def interleave(q):
    """63-bit Morton code of the cells q [N, 3]: bit b of x at 3 b, of y at 3 b + 1, of z at 3 b + 2."""
    q = np.asarray(q, np.uint64)
    key = np.zeros(len(q), np.uint64)
    one = np.uint64(1)
    for b in range(21):
        for c in range(3):
            key |= ((q[:, c] >> np.uint64(b)) & one) << np.uint64(3 * b + c)
    return key


def deinterleave(keys):
    """The cells [N, 3] of 63-bit Morton codes (the inverse of interleave: for building scenes with chosen keys)."""
    keys = np.asarray(keys, np.uint64)
    q = np.zeros((len(keys), 3), np.uint64)
    one = np.uint64(1)
    for b in range(21):
        for c in range(3):
            q[:, c] |= ((keys >> np.uint64(3 * b + c)) & one) << np.uint64(b)
    return q


def morton_keys(means):
    return interleave(axis_cells(means))


def expected_perm(means, sorted_=True):
    """Layout position -> original index: the stable sort of the keys; the identity for a scene the upload does not sort
    (sgs_tuning.morton = 0, or N <= 64)."""
    n = len(means)
    if not sorted_ or n <= 64:
        return np.arange(n, dtype=np.uint32)
    return np.argsort(morton_keys(means), kind="stable").astype(np.uint32)


def radius_window(d, centre):
    """(least, most) a stored R may be for a chunk whose farthest member lies d (fp64) from the stored centre: R >= d is what correctness
    rests on (a chunk is skipped by its sphere), R <= 1.0002 d + 2e-6 (|cx| + |cy| + |cz|) + 1e-29 — twice the kernel's own padding — is
    what makes the sphere worth having."""
    c = np.abs(np.asarray(centre, np.float64)).sum(axis=-1)
    return d, 1.0002 * d + 2.0e-6 * c + 1.0e-29


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check_chunk_bounds(means_layout, scales_layout, cbound, what=""):
    """cbound [ceil(N/64), 8] (SGS_BUF_CHUNK_BOUNDS) against the scene in LAYOUT order.  Padding lanes of the last chunk take no part.
    A chunk with a non-finite member coordinate has no centre worth comparing (the kernel's fminf / fmaxf skip NaN, inf - inf is NaN);
    it must have R = +inf, which is all the culling test reads of it.  Returns the number of chunks held to the R inequalities."""
    m = np.asarray(means_layout, F).reshape(-1, 3)
    s = np.asarray(scales_layout, F).reshape(-1, 3)
    n = len(m)
    nc = (n + 63) // 64
    cb = np.asarray(cbound, F).reshape(-1, 8)
    assert cb.shape == (nc, 8), f"{what}: chunk bounds: {cb.shape} for {nc} chunks"
    pad = nc * 64 - n
    M = np.concatenate([m, np.full((pad, 3), np.nan, F)]).reshape(nc, 64, 3)
    S = np.concatenate([s, np.full((pad, 3), np.nan, F)]).reshape(nc, 64, 3)
    real = (np.arange(nc * 64) < n).reshape(nc, 64)
    with np.errstate(all="ignore"):
        lo, hi = np.fmin.reduce(M, axis=1), np.fmax.reduce(M, axis=1)                    # NaN (padding) ignored
        centre = F(0.5) * (lo + hi)
        assert centre.dtype == F
        s_max = np.fmax.reduce(np.fmax.reduce(S, axis=2), axis=1)
        has_nan = (np.isnan(M).any(axis=2) & real).any(axis=1)
        wild = ((~np.isfinite(M)).any(axis=2) & real).any(axis=1)                         # NaN or inf among the real members
        # s_max: the largest scale of the real members, bit for bit
        bad = np.nonzero(_bits(cb[:, 4]) != _bits(s_max))[0]
        assert not len(bad), (f"{what}: chunk bounds: s_max of chunk {bad[0]} is {float(cb[bad[0], 4])!r}, the largest scale of its members is "
                              f"{float(s_max[bad[0]])!r} ({len(bad)} of {nc} chunks differ)")
        assert (_bits(cb[:, 5:8]) == 0).all(), f"{what}: chunk bounds: the three spare words are not 0"
        # centre: exact in fp32, bit for bit (chunks of finite members)
        clean = ~wild
        # (the sign of a ZERO centre is not compared: fminf / fmaxf of -0.0 and +0.0 may return either, in the kernel and here alike)
        diff = clean & (_bits(cb[:, 0:3] + F(0.0)) != _bits(centre + F(0.0))).any(axis=1)
        bad = np.nonzero(diff)[0]
        assert not len(bad), (f"{what}: chunk bounds: the centre of chunk {bad[0]} is {cb[bad[0], :3].tolist()}, 0.5f (lo + hi) of its members is "
                              f"{centre[bad[0]].tolist()} ({len(bad)} of {nc} chunks differ)")
        R = cb[:, 3].astype(np.float64)
        # d: fp64 distance of the farthest real member from the STORED centre
        dist = np.sqrt(((M.astype(np.float64) - cb[:, None, 0:3].astype(np.float64)) ** 2).sum(axis=2))
        dist[~real] = 0.0
        d = np.where(clean, np.nanmax(np.where(np.isnan(dist), 0.0, dist), axis=1), np.inf)
    must_inf = wild | (s_max.astype(np.float64) >= R_KEEP) | (d >= D_SQUARES_OVERFLOW)
    bad = np.nonzero(must_inf & ~np.isposinf(R))[0]
    assert not len(bad), (f"{what}: chunk bounds: chunk {bad[0]} (NaN member: {bool(has_nan[bad[0]])}, s_max {float(s_max[bad[0]])!r}, d {float(d[bad[0]])!r}) "
                          f"must never be culled, its R is {float(R[bad[0]])!r} and not +inf")
    held = ~must_inf & (d < D_SQUARES_FIT)
    least, most = radius_window(d, cb[:, 0:3])
    bad = np.nonzero(held & ~(R >= least))[0]
    assert not len(bad), (f"{what}: chunk bounds: R of chunk {bad[0]} is {float(R[bad[0]])!r} < d = {float(d[bad[0]])!r}: a member lies outside the sphere "
                          f"({len(bad)} of {nc} chunks)")
    bad = np.nonzero(held & ~(R <= most))[0]
    assert not len(bad), (f"{what}: chunk bounds: R of chunk {bad[0]} is {float(R[bad[0]])!r}, more than 1.0002 d + 2e-6 |c|_1 + 1e-29 = {float(most[bad[0]])!r} "
                          f"(d = {float(d[bad[0]])!r}): the sphere is not tight ({len(bad)} of {nc} chunks)")
    between = ~must_inf & ~held                                   # (squares at the edge of fp32: +inf or within the window)
    bad = np.nonzero(between & ~(np.isposinf(R) | ((R >= least) & (R <= most))))[0]
    assert not len(bad), f"{what}: chunk bounds: R of chunk {bad[0]} is {float(R[bad[0]])!r}, d = {float(d[bad[0]])!r}"
    return int(held.sum())
