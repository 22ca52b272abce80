"""fp64 NumPy ray caster: the reference the collision-mesh depth kernels (sgs_render_mesh_depth*) are checked against.

Same rays as the kernels — pixel (x, y) samples r = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1) in camera space — the same near / far
rule (near < z <= far) and both faces of every triangle.  The camera's view and the vertices are rounded to fp32 first, as the library
receives them; everything after that is fp64.

Per pixel it returns three depths:
  nominal   the exact answer of this arithmetic: min z over the triangles whose three edge functions sign(det) e_k . r are >= 0;
  lenient   the same with every edge function relaxed by eps_k, and every candidate z lowered by its tolerance:  min z (1 - tol);
  strict    every edge function tightened by eps_k, every candidate raised:                                           min z (1 + tol).
A kernel's value `got` passes when  lenient <= got <= strict  (inf compared exactly: lenient = inf demands inf).  Away from edges the
two agree up to the tolerances, so this is a relative check of ~1e-5; pixels within eps of an edge of some triangle ("edge band") may
take either side's value.

The bounds, from fp32 rounding (u = 2^-24).  The kernel rounds each e_k (computed in fp64 from fp64 vertices) to fp32 — |de_i| <= u |e_i|
— forms r in fp32 — |dr_i| <= u |r_i| (x + 0.5 - cx is exact, the division rounds once) — and evaluates fma(e.x, r.x, fma(e.y, r.y, e.z)):
two more roundings, each <= u times a partial sum bounded by sum_i |e_i r_i|.  To first order the error of e . r is therefore at most
u (1 + 1 + 2) sum_i |e_i r_i| = 4 u sum_i |e_i r_i|; the reference uses eps_k = 5 u sum_i |e_k,i r_i| (one u of slack for the fp64
steps and second-order terms).  That is ~3e-7 |e||r| at most — the "1e-7 relative to |e| |r|" order of the plain estimate, derived.
The depth z = d / (n . r) goes through the same steps (n, d rounded to fp32: 1 u for d, 4 u sum_i |n_i r_i| for the denominator, 1 u
for the division), so its relative error is at most u (2 + 4 G) with G = sum_i |n_i r_i| / |n . r| — G is ~1 for a surface seen face
on and grows as 1 / sin(angle) for grazing ones.  The per-candidate tolerance is tol = 1e-5 + u (3 + 5 G): the 1e-5 of the pass rule
plus the derived term, which only matters for rays within a few degrees of a triangle's plane.

Edge-exact bounds (cast_continuous / check_continuous).  The edge band above is where `check` cannot see a crack: there `strict` is the
next surface behind, or +inf.  The kernels promise more (csrc/sgs_mesh.h): the two triangles of a shared edge build its plane from the
same two fp64 vertices in index order, with a product that is anti-commutative bit for bit, round it to fp32 and flip its sign exactly,
so they evaluate +-the same fp32 value at every pixel, and "e . r >= 0" makes one of them claim it.  Around a vertex the rounded
planes no longer meet in one line; the kernels decide an edge within fp32 rounding of 0 again from its fp64 plane with a margin above
the fp64 rounding (sgs_mesh.h header), and the fp64 planes through a vertex meet in one line up to that margin, so some triangle of the
fan claims the pixel.  Both rules only ever add a triangle whose exact edge values are >= -eps_k.  So for a mesh whose depth field
is continuous across its shared edges and that every ray meets once (a coplanar sheet; a closed box seen from inside):
  claimable   a triangle is a candidate of a pixel when its three edge functions are >= -eps_k and its z is inside (near, far] up to tol:
              exactly the `lenient` candidates above.  A triangle whose fp32 test passes is one of them (the eps_k derivation).
  value       the kernel returns the z of a claiming triangle, so a finite value lies in [min z (1 - tol), max z (1 + tol)] over the
              candidates.  On a sheet the candidates share the plane (up to the fp32 rounding of the vertices: a relative 2^-24, inside
              REL), so this is d / (n . r) within REL + u (3 + 5 G) — the tolerance above, with no edge band.  On the box's seams, where two
              faces that are not coplanar meet, the candidates are the two faces: either face's depth, within the same tolerance.
  need        the pixel must be finite when some candidate passes every edge either outright (s_k >= eps_k) or because the edge is shared
              (s_k >= -eps_k: the neighbour across it takes the pixel if this one does not), with z inside (near, far] by tol.
  outline     except within eps_k of an edge that no other triangle shares (the sheet's own boundary): such a pixel may be +inf or the
              surface, as in `check`.  The closed box has no such edge: every pixel of it is needed, vertices included.
No allowance beyond the module's eps_k and tol enters: the promise is exact, and the rounding it leaves is that of one triangle's value.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
EDGE_K = 5.0
REL = 1.0e-5
TILE = 8


def _rays(cam, xs, ys):
    return np.stack([(xs + 0.5 - cam["cx"]) / cam["fx"], (ys + 0.5 - cam["cy"]) / cam["fy"], np.ones(len(xs))], 1)


def cam_dict(width, height, fx, fy, cx, cy, view):
    return dict(width=int(width), height=int(height), fx=float(np.float32(fx)), fy=float(np.float32(fy)), cx=float(np.float32(cx)),
                cy=float(np.float32(cy)), view=np.asarray(view, np.float32).astype(np.float64).reshape(4, 4))


def of_camera(c, model_to_world=None):
    """cam_dict of a sage_gs Camera (its view composed with model_to_world, rounded to fp32 as the library receives it)."""
    v = np.asarray(c.view, np.float64).reshape(4, 4)
    if model_to_world is not None:
        v = v @ np.asarray(model_to_world, np.float64).reshape(4, 4)
    return cam_dict(c.width, c.height, c.fx, c.fy, c.cx, c.cy, v)


def cast(vertices, triangles, cam, near=0.2, far=1.0e30, pixels=None, chunk=1 << 21):
    """vertices [V,3] (model space), triangles [F,3], cam: cam_dict.  pixels: None (the whole frame) or (ys, xs) arrays.
    Returns dict(nominal, lenient, strict, edge) — float64 [H,W] (or [P]) and the edge-band mask."""
    W, H = cam["width"], cam["height"]
    if pixels is None:
        ys, xs = np.divmod(np.arange(W * H), W)
        shape = (H, W)
    else:
        ys, xs = (np.asarray(a, np.int64) for a in pixels)
        shape = (len(ys),)
    P = len(ys)
    nom = np.full(P, np.inf); lo = np.full(P, np.inf); hi = np.full(P, np.inf); edge = np.zeros(P, bool)
    if len(np.asarray(triangles).reshape(-1, 3)) == 0 or P == 0:
        return dict(nominal=nom.reshape(shape), lenient=lo.reshape(shape), strict=hi.reshape(shape), edge=edge.reshape(shape))
    for pix, t, s, eps, z, tol in _candidates(vertices, triangles, cam, near, xs, ys, chunk):
        ok = np.isfinite(z)
        ins = (s >= 0).all(1) & ok & (z > near) & (z <= far)
        lin = (s >= -eps).all(1) & ok & (z * (1 + tol) > near) & (z * (1 - tol) <= far)
        sin_ = (s >= eps).all(1) & ok & (z * (1 - tol) > near) & (z * (1 + tol) <= far)
        np.minimum.at(nom, pix[ins], z[ins])
        np.minimum.at(lo, pix[lin], (z * (1 - tol))[lin])
        np.minimum.at(hi, pix[sin_], (z * (1 + tol))[sin_])
        edge[pix[lin & ~sin_]] = True
    return dict(nominal=nom.reshape(shape), lenient=lo.reshape(shape), strict=hi.reshape(shape), edge=edge.reshape(shape))


def _candidates(vertices, triangles, cam, near, xs, ys, chunk):
    """The (triangle, pixel) pairs of the conservative pixel rects, in chunks: (pixel index into xs / ys, triangle, s [n,3] = the
    edge functions sign(det) e_k . r, eps [n,3], z = d / (n . r), tol).  Triangles with det == 0 have none."""
    W, H = cam["width"], cam["height"]
    V = np.asarray(vertices, np.float32).astype(np.float64)
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    M = cam["view"]
    Pc = V @ M[:3, :3].T + M[:3, 3]
    p0, p1, p2 = Pc[T[:, 0]], Pc[T[:, 1]], Pc[T[:, 2]]
    E = np.stack([np.cross(p1, p2), np.cross(p2, p0), np.cross(p0, p1)], 1)          # [F,3 edges,3]
    det = np.einsum("ij,ij->i", E[:, 0], p0)
    E *= np.sign(det)[:, None, None]
    N = np.cross(p1 - p0, p2 - p0)
    D = np.einsum("ij,ij->i", N, p0)
    # conservative pixel rect of each triangle: the part with z >= near (1 - 1e-6), projected, plus two pixels
    zc = near * (1.0 - 1.0e-6)
    umin = np.full(len(T), np.inf); umax = np.full(len(T), -np.inf); vmin = umin.copy(); vmax = umax.copy()
    P3 = [p0, p1, p2]
    for k in range(3):
        a, b = P3[k], P3[(k + 1) % 3]
        pts = []
        ka = a[:, 2] >= zc
        pts.append((a, ka))
        cross = ka != (b[:, 2] >= zc)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (zc - a[:, 2]) / (b[:, 2] - a[:, 2])
            q = a + s[:, None] * (b - a)
        q[:, 2] = zc
        pts.append((q, cross))
        for q, ok in pts:
            with np.errstate(divide="ignore", invalid="ignore"):
                u = np.clip(cam["fx"] * q[:, 0] / q[:, 2] + cam["cx"], -4, W + 4)
                v = np.clip(cam["fy"] * q[:, 1] / q[:, 2] + cam["cy"], -4, H + 4)
            umin = np.where(ok, np.minimum(umin, u), umin); umax = np.where(ok, np.maximum(umax, u), umax)
            vmin = np.where(ok, np.minimum(vmin, v), vmin); vmax = np.where(ok, np.maximum(vmax, v), vmax)
    live = (umin <= umax) & (det != 0) & np.isfinite(det)
    x0 = np.clip(np.floor(umin) - 2, 0, W - 1); x1 = np.clip(np.floor(umax) + 2, 0, W - 1)
    y0 = np.clip(np.floor(vmin) - 2, 0, H - 1); y1 = np.clip(np.floor(vmax) + 2, 0, H - 1)
    tid = np.nonzero(live)[0]
    tx0, tx1 = (x0[tid] // TILE).astype(np.int64), (x1[tid] // TILE).astype(np.int64)
    ty0, ty1 = (y0[tid] // TILE).astype(np.int64), (y1[tid] // TILE).astype(np.int64)
    gx = (W + TILE - 1) // TILE
    # pixels of the target set by tile (CSR)
    ptile = (ys // TILE) * gx + xs // TILE
    order = np.argsort(ptile, kind="stable")
    n_t = gx * ((H + TILE - 1) // TILE)
    start = np.searchsorted(ptile[order], np.arange(n_t + 1))
    # (triangle, tile) pairs
    w_ = tx1 - tx0 + 1; area = w_ * (ty1 - ty0 + 1)
    tri_of = np.repeat(tid, area)
    j = np.arange(int(area.sum())) - np.repeat(np.cumsum(area) - area, area)
    wr = np.repeat(w_, area)
    tile = (np.repeat(ty0, area) + j // wr) * gx + np.repeat(tx0, area) + j % wr
    cnt = start[tile + 1] - start[tile]
    keep = cnt > 0
    tri_of, tile, cnt = tri_of[keep], tile[keep], cnt[keep]
    # expand to (triangle, pixel) pairs, in chunks
    cum = np.concatenate([[0], np.cumsum(cnt)])
    total = int(cum[-1])
    for c0 in range(0, total, chunk):
        c1 = min(total, c0 + chunk)
        k = np.arange(c0, c1)
        pr = np.searchsorted(cum, k, side="right") - 1
        pix = order[start[tile[pr]] + (k - cum[pr])]
        t = tri_of[pr]
        r = _rays(cam, xs[pix].astype(np.float64), ys[pix].astype(np.float64))
        e = E[t]                                                    # [n,3,3]
        s = np.einsum("nkc,nc->nk", e, r)
        eps = EDGE_K * U * np.einsum("nkc,nc->nk", np.abs(e), np.abs(r))
        den = np.einsum("nc,nc->n", N[t], r)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = D[t] / den
            g = np.einsum("nc,nc->n", np.abs(N[t]), np.abs(r)) / np.abs(den)
        yield pix, t, s, eps, z, REL + U * (3.0 + 5.0 * g)


def check(got, ref, what=""):
    """The per-pixel pass rule; prints the frame's edge-band count.  Returns (n_fail, n_edge)."""
    got = np.asarray(got, np.float64).reshape(ref["nominal"].shape)
    lo, hi = ref["lenient"], ref["strict"]
    ok = (lo <= got) & (got <= hi)
    n_edge = int(ref["edge"].sum())
    bad = ~ok
    print(f"mesh depth {what}: {got.size} px, edge band {n_edge}, failing {int(bad.sum())}, inf {int(np.isinf(got).sum())}")
    if bad.any():
        i = np.flatnonzero(bad.reshape(-1))[:8]
        raise AssertionError(f"{what}: {int(bad.sum())} pixels outside [lenient, strict]; first {i.tolist()}: got "
                             f"{got.reshape(-1)[i].tolist()} lenient {lo.reshape(-1)[i].tolist()} strict {hi.reshape(-1)[i].tolist()}")
    return int(bad.sum()), n_edge


def sample_pixels(width, height, n=20000, seed=0):
    rng = np.random.default_rng(seed)
    k = rng.choice(width * height, size=min(n, width * height), replace=False)
    return np.divmod(k, width)


def _shared_edges(triangles):
    """[F,3] bool: edge k of a triangle (the one opposite vertex k, as in E above) is shared with another triangle."""
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    ab = np.stack([np.stack([T[:, 1], T[:, 2]], 1), np.stack([T[:, 2], T[:, 0]], 1), np.stack([T[:, 0], T[:, 1]], 1)], 1)   # [F,3,2]
    key = np.sort(ab, axis=2).reshape(-1, 2)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return (cnt[inv.reshape(-1)] >= 2).reshape(-1, 3) & (key[:, 0] != key[:, 1]).reshape(-1, 3)


def cast_continuous(vertices, triangles, cam, near=0.2, far=1.0e30, pixels=None, chunk=1 << 21):
    """The edge-exact bounds of a mesh whose depth field is continuous across every shared edge and that the rays meet once (a coplanar
    sheet; a closed convex box seen from inside).  See "Edge-exact bounds" in the module header.  Returns dict(lo, hi, need, outline,
    shared_band, zeros, vertex): float64 lo / hi and bool masks, [H,W] (or [P]).  vertex: pixels within eps of two edges of one candidate
    (a vertex; counted for the report, not exempt)."""
    W, H = cam["width"], cam["height"]
    if pixels is None:
        ys, xs = np.divmod(np.arange(W * H), W)
        shape = (H, W)
    else:
        ys, xs = (np.asarray(a, np.int64) for a in pixels)
        shape = (len(ys),)
    P = len(ys)
    lo = np.full(P, np.inf); hi = np.full(P, -np.inf)
    need = np.zeros(P, bool); outline = np.zeros(P, bool); band = np.zeros(P, bool); zeros = np.zeros(P, bool); vert = np.zeros(P, bool)
    shared = _shared_edges(triangles)
    if len(shared) and P:
        for pix, t, s, eps, z, tol in _candidates(vertices, triangles, cam, near, xs, ys, chunk):
            ok = np.isfinite(z)
            sh = shared[t]
            within = (s >= -eps).all(1)
            lin = within & ok & (z * (1 + tol) > near) & (z * (1 - tol) <= far)
            hit = ((s >= eps) | (sh & (s >= -eps))).all(1) & ok & (z * (1 - tol) > near) & (z * (1 + tol) <= far)
            near_edge = within[:, None] & (np.abs(s) < eps)
            np.minimum.at(lo, pix[lin], (z * (1 - tol))[lin])
            np.maximum.at(hi, pix[lin], (z * (1 + tol))[lin])
            need[pix[hit]] = True
            outline[pix[(near_edge & ~sh).any(1)]] = True
            band[pix[(near_edge & sh).any(1) & lin]] = True
            zeros[pix[within & (s == 0).any(1)]] = True
            vert[pix[near_edge.sum(1) >= 2]] = True
    need &= ~outline
    return dict(lo=lo.reshape(shape), hi=hi.reshape(shape), need=need.reshape(shape), outline=outline.reshape(shape),
                shared_band=band.reshape(shape), zeros=zeros.reshape(shape), vertex=vert.reshape(shape))


def check_continuous(got, cc, what=""):
    """The edge-exact pass rule (cast_continuous): a finite value lies in [lo, hi]; +inf is allowed only where no pixel is `need`ed; a
    pixel no triangle can claim is +inf.  Prints the counts; returns dict(n_px, shared_band, outline, zeros, need)."""
    got = np.asarray(got, np.float64).reshape(cc["lo"].shape)
    lo, hi, need = cc["lo"], cc["hi"], cc["need"]
    fin = np.isfinite(got)
    ok = np.where(fin, (lo <= got) & (got <= hi), (got == np.inf) & ~need)
    n = dict(n_px=int(got.size), shared_band=int(cc["shared_band"].sum()), outline=int(cc["outline"].sum()), zeros=int(cc["zeros"].sum()),
             need=int(need.sum()), vertex=int(cc["vertex"].sum()))
    bad = ~ok
    print(f"mesh depth (edge-exact) {what}: {n['n_px']} px, need {n['need']}, shared-edge band {n['shared_band']} (exact zeros "
          f"{n['zeros']}), outline band {n['outline']}, vertex band {n['vertex']}, failing {int(bad.sum())}, inf {int((~fin).sum())}")
    if bad.any():
        i = np.flatnonzero(bad.reshape(-1))[:8]
        raise AssertionError(f"{what} (edge-exact): {int(bad.sum())} pixels fail, {int((bad & ~fin & need).sum())} of them +inf where a "
                             f"triangle must claim the pixel; first {i.tolist()}: got {got.reshape(-1)[i].tolist()} lo "
                             f"{lo.reshape(-1)[i].tolist()} hi {hi.reshape(-1)[i].tolist()} shared-edge band "
                             f"{cc['shared_band'].reshape(-1)[i].tolist()}")
    return n
