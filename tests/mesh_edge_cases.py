"""Collision-mesh depth cases that put pixels ON edges, the near / far planes and degenerate input, shared by the emulator tests
(test_emu_mesh_edges.py), the GPU tests (test_gpu_mesh_depth.py) and the mesh mutants (test_mesh_checker_sensitivity.py).

Every case takes a driver — EmuMesh (the wave64 emulator) or GpuMesh (a sage_gs Renderer) — and raises AssertionError when the frames
are wrong.  The meshes are built in code, in camera space, then carried to model space by the inverse of the camera's view:
  lattice sheets  vertices back-projected from pixel centres onto a plane, so that every edge runs through pixel centres.  Under a random
                  rigid view (inexact) e . r lands within a few ulps of 0 at thousands of pixels; under the identity view with fx, fy
                  powers of two and dyadic ray slopes (exact) it is exactly 0 on whole rows, columns and diagonals.
  fan             64 triangles around one vertex that sits exactly on a pixel-centre ray.
  slivers         1 x 100-pixel triangles between pixel rows, the rows' centres exactly on their long edges.
  box             a closed grid_box seen from inside.
All of them are checked with mesh_depth_ref.check_continuous (no edge band) as well as mesh_depth_ref.check.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

import mesh_depth_ref as ref
from sage_gs import _capi, scenes


# ---- drivers -----------------------------------------------------------------------------------------------------------------------

class EmuMesh:
    """sgs_render_mesh_depth* of an emulator library (host pointers: the emulator's 'device' is the host)."""

    def __init__(self, lib):
        self.lib = lib
        self.ctx = C.c_void_p()
        lib.check(lib.sgs_create(0, _capi.BACKEND_HIP, C.byref(self.ctx)))

    def upload(self, V, T):
        v = np.ascontiguousarray(V, np.float32); t = np.ascontiguousarray(T, np.int32)
        h = C.c_void_p()
        rc = self.lib.sgs_mesh_upload(self.ctx, len(v), v.ctypes.data if len(v) else None, len(t), t.ctypes.data if len(t) else None,
                                      0, C.byref(h))
        return rc, h

    def mesh(self, V, T):
        rc, h = self.upload(V, T)
        self.lib.check(rc, self.ctx)
        return h

    def cfg(self, near=0.2, far=1e30, flags=0, stride=1):
        k = self.lib.default_config()
        k.near_z, k.far_z, k.flags, k.tile_row_stride = near, far, flags, stride
        return k

    def render(self, m, cam, rows=(0, -1), cfg=None, fill=-1.0):
        c = _capi.make_camera(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["view"].tolist())
        out = np.full((cam["height"], cam["width"]), fill, np.float32)
        st = _capi.SgsStats()
        rc = self.lib.sgs_render_mesh_depth(self.ctx, m, C.byref(c), C.byref(cfg or self.cfg()), rows[0], rows[1], out.ctypes.data,
                                            C.byref(st), None)
        return rc, out, st.as_dict()

    def batch(self, m, cams, cfg=None):
        arr = (_capi.SgsCamera * len(cams))(*[_capi.make_camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"],
                                                                 c["view"].tolist()) for c in cams])
        out = np.zeros((len(cams), cams[0]["height"], cams[0]["width"]), np.float32)
        st = (_capi.SgsStats * len(cams))()
        self.lib.check(self.lib.sgs_render_mesh_depth_batch(self.ctx, m, arr, len(cams), C.byref(cfg or self.cfg()), out.ctypes.data, st,
                                                            None), self.ctx)
        return out, [s.as_dict() for s in st]

    def err(self):
        return self.lib.sgs_last_error(self.ctx).decode()

    # the interface of the shared cases
    def frame(self, V, T, cam, near=0.2, far=1e30, rows=(0, -1), fill=-1.0):
        m = self.mesh(V, T)
        try:
            rc, out, st = self.render(m, cam, rows=rows, cfg=self.cfg(near=near, far=far), fill=fill)
            self.lib.check(rc, self.ctx)
            return out, st
        finally:
            self.lib.sgs_mesh_free(self.ctx, m)

    def frames(self, V, T, cams, near=0.2, far=1e30):
        m = self.mesh(V, T)
        try:
            return self.batch(m, cams, cfg=self.cfg(near=near, far=far))
        finally:
            self.lib.sgs_mesh_free(self.ctx, m)

    def close(self):
        if self.ctx:
            self.lib.sgs_destroy(self.ctx)
            self.ctx = C.c_void_p()


class GpuMesh:
    """The same interface over a sage_gs Renderer (device frames copied back to the host)."""

    def __init__(self, renderer):
        self.r = renderer

    @staticmethod
    def camera(cam):
        from sage_gs import Camera
        return Camera(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["view"])

    @staticmethod
    def config(near, far):
        from sage_gs import RenderConfig
        return RenderConfig(near=near, far=far)

    def frame(self, V, T, cam, near=0.2, far=1e30, rows=(0, -1), fill=-1.0):
        import torch
        m = self.r.upload_mesh(V, T)
        try:
            out = torch.full((cam["height"], cam["width"]), fill, dtype=torch.float32, device=self.r.device)
            self.r.render_mesh_depth(self.camera(cam), m, config=self.config(near, far), tile_rows=None if rows == (0, -1) else rows, out=out)
            return out.cpu().numpy(), dict(self.r.last_stats)
        finally:
            m.free()

    def frames(self, V, T, cams, near=0.2, far=1e30):
        m = self.r.upload_mesh(V, T)
        try:
            out, st = self.r.render_mesh_depth_batch([self.camera(c) for c in cams], m, config=self.config(near, far), want_stats=True)
            return out.cpu().numpy(), st
        finally:
            m.free()


# ---- cameras and meshes ------------------------------------------------------------------------------------------------------------

def exact_cam(w, h):
    """Identity view, fx = fy = the power of two at most w, principal point at the centre: every pixel-centre ray slope is a half-integer
    over fx, dyadic with at most 12 bits, and so is every vertex built on such a ray at z = 1."""
    f = float(2 ** int(math.log2(w)))
    return ref.cam_dict(w, h, f, f, w / 2, h / 2, np.eye(4))


def random_cam(w, h, seed):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = scenes.reference_intrinsics(w, h)
    view = scenes.view_from_yaw(rng.uniform(-5, 5, 3), rng.uniform(0, 2 * math.pi), rng.uniform(-0.6, 0.6))
    return ref.cam_dict(w, h, fx, fy, cx, cy, view)


def nudged(cam, rng, angle=0.02, shift=0.02):
    """cam turned by a random rotation of about `angle` radians (Rodrigues) and moved by about `shift`."""
    a = rng.normal(0.0, angle, 3)
    th = float(np.linalg.norm(a))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]]) / th
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * K @ K
    D[:3, 3] = rng.normal(0.0, shift, 3)
    return ref.cam_dict(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], D @ cam["view"])


def to_model(cam, P):
    """camera-space points [n,3] -> model space, through the inverse of the camera's (fp32-rounded) view."""
    Mi = np.linalg.inv(cam["view"])
    return P @ Mi[:3, :3].T + Mi[:3, 3]


def _rays_uv(cam, u, v):
    return np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones_like(u)], -1)


def _shuffle(V, T, rng, mixed=True):
    """Flip the index order of a random half of the triangles (mixed winding), permute the triangles and relabel the vertices."""
    T = np.asarray(T, np.int64).copy()
    if mixed:
        flip = rng.random(len(T)) < 0.5
        T[flip] = T[flip][:, ::-1]
    T = T[rng.permutation(len(T))]
    relabel = rng.permutation(len(V))
    V2 = np.empty_like(V)
    V2[relabel] = V
    return V2, relabel[T]


def lattice_sheet(w, h, seed=0, step=4, exact=False, region=None):
    """A sheet whose vertices lie on the rays of pixel centres every `step` pixels over `region` = (x0, x1, y0, y1) (default: the frame
    less two pixels), both diagonal choices at random, mixed winding, triangles permuted.  exact: exact_cam and the plane z = 1 (every
    vertex dyadic); otherwise random_cam(seed) and a tilted plane."""
    rng = np.random.default_rng(seed)
    cam = exact_cam(w, h) if exact else random_cam(w, h, seed)
    x0, x1, y0, y1 = region or (2, w - 3, 2, h - 3)
    xs, ys = np.arange(x0, x1 + 1, step), np.arange(y0, y1 + 1, step)
    u, v = np.meshgrid(xs + 0.5, ys + 0.5, indexing="ij")
    r = _rays_uv(cam, u.reshape(-1), v.reshape(-1))
    if exact:
        P = r
    else:
        n = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), 1.0])
        P = r * (rng.uniform(2.0, 4.0) / (r @ n))[:, None]
    ny = len(ys)
    i, j = np.meshgrid(np.arange(len(xs) - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).reshape(-1); b = a + ny; c = b + 1; d = a + 1
    diag = rng.random(len(a)) < 0.5
    T = np.concatenate([np.where(diag[:, None], np.stack([a, b, c], 1), np.stack([a, b, d], 1)),
                        np.where(diag[:, None], np.stack([a, c, d], 1), np.stack([b, c, d], 1))])
    V, T = _shuffle(to_model(cam, P), T, rng)
    return dict(V=V, T=T, cam=cam, name=f"lattice {'exact' if exact else 'inexact'} step {step} {w}x{h}")


def fan(w, h, n=64, seed=0):
    """n triangles around a centre vertex exactly on the ray of pixel (w/2 + 3, h/2 - 5), on a tilted plane (exact_cam, identity view).
    The ring is not dyadic: the edges through the centre evaluate to rounding noise around 0 at the centre pixel."""
    rng = np.random.default_rng(seed)
    cam = exact_cam(w, h)
    c = 2.0 * _rays_uv(cam, np.array([w // 2 + 3 + 0.5]), np.array([h // 2 - 5 + 0.5]))[0]
    nrm = np.array([0.3, -0.2, 1.0]); nrm /= np.linalg.norm(nrm)
    a = np.cross(nrm, [0.0, 1.0, 0.0]); a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    th = 2 * math.pi * (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n
    rad = 0.25 * c[2] * (1.0 + 0.3 * rng.random(n))
    ring = c + rad[:, None] * (np.cos(th)[:, None] * a + np.sin(th)[:, None] * b)
    V = np.concatenate([c[None], ring])
    T = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1)
    V, T = _shuffle(V, T, rng)
    return dict(V=V, T=T, cam=cam, name=f"fan of {n} {w}x{h}")


def slivers(w, h, rows=24, length=100, seed=0):
    """Strips between consecutive pixel rows (their centres exactly on the strips' shared long edges), each of triangles `length` pixels
    long and 1 pixel tall, the vertices of alternate rows staggered by length / 2 (exact_cam, the plane z = 1)."""
    rng = np.random.default_rng(seed)
    cam = exact_cam(w, h)
    y0 = h // 2 - rows // 2
    V, T, idx = [], [], []
    for k in range(rows + 1):
        us = np.arange(-length, w + length, length) + (length // 2) * (k % 2) + 0.5
        idx.append(np.arange(len(us)) + sum(len(q) for q in V))
        V.append(_rays_uv(cam, us, np.full(len(us), y0 + k + 0.5)))
    for k in range(rows):
        A, B = (idx[k], idx[k + 1]) if k % 2 == 0 else (idx[k + 1], idx[k])           # A: the row that starts further left
        m = min(len(A) - 1, len(B))
        T += [[A[i], A[i + 1], B[i]] for i in range(m)] + [[B[i], A[i + 1], B[i + 1]] for i in range(min(m, len(B) - 1))]
    V, T = _shuffle(np.concatenate(V), np.array(T), rng)
    return dict(V=V, T=T, cam=cam, name=f"slivers 1x{length} px, {rows} rows, {w}x{h}")


def box(w, h, seed=0):
    """A closed grid_box room seen from inside (every edge shared: no outline)."""
    rng = np.random.default_rng(seed)
    V, T = scenes.grid_box((0.0, 0.0, 0.0), (6.0, 5.0, 2.8), (13, 11, 7))
    fx, fy, cx, cy = scenes.reference_intrinsics(w, h)
    pos = (rng.uniform(0.4, 5.6), rng.uniform(0.4, 4.6), rng.uniform(0.4, 2.4))
    cam = ref.cam_dict(w, h, fx, fy, cx, cy, scenes.view_from_yaw(pos, rng.uniform(0, 2 * math.pi), rng.uniform(-1.0, 1.0)))
    return dict(V=V, T=T, cam=cam, name=f"closed box from inside {w}x{h}")


EDGE_CASES = {
    "lattice_inexact": lambda w, h, seed: lattice_sheet(w, h, seed=seed, step=4, exact=False),
    "lattice_exact": lambda w, h, seed: lattice_sheet(w, h, seed=seed, step=4, exact=True),
    "fan": lambda w, h, seed: fan(w, h, seed=seed),
    "slivers": lambda w, h, seed: slivers(w, h, seed=seed),
    "box": lambda w, h, seed: box(w, h, seed=seed),
}


def reference(case, cam=None, pixels=None):
    cam = cam or case["cam"]
    return (ref.cast(case["V"], case["T"], cam, pixels=pixels), ref.cast_continuous(case["V"], case["T"], cam, pixels=pixels))


def check_frame(got, case, cam=None, pixels=None, what=""):
    """Both checks on one frame (or the sampled `pixels` of it); returns check_continuous's counts and the old check's edge band."""
    rc, cc = reference(case, cam, pixels)
    _, n_edge = ref.check(got, rc, what)
    n = ref.check_continuous(got, cc, what)
    n["edge_band"] = n_edge
    n["finite"] = int(np.isfinite(got).sum())
    return n


def check_edge_case(drv, name, w, h, seed=0):
    """One EDGE_CASES frame against both checks.  The exact cases must sample exact zeros of e . r; the box must be finite everywhere."""
    case = EDGE_CASES[name](w, h, seed)
    got, st = drv.frame(case["V"], case["T"], case["cam"])
    assert not np.isnan(got).any(), case["name"]
    n = check_frame(got, case, what=case["name"])
    # the cases' own guards: the exact ones sample e . r == 0 exactly on whole rows / columns / diagonals, the inexact one a wide band
    if name == "lattice_exact":
        assert n["zeros"] > w * h // 4, (case["name"], n)
    if name == "slivers":
        assert n["zeros"] > 12 * w, (case["name"], n)
    if name == "lattice_inexact":
        assert n["shared_band"] > w * h // 4, (case["name"], n)
    if name == "fan":
        cx, cy = w // 2 + 3, h // 2 - 5
        assert np.isfinite(got[cy, cx]), "fan: the pixel on the shared vertex is not claimed"
    if name == "box":
        assert np.isfinite(got).all()
    return case, got, n


# ---- near / far ----------------------------------------------------------------------------------------------------------------------

def _quad(c0, c1, c2, c3):
    return np.array([c0, c1, c2, c3], np.float64), np.array([[0, 1, 2], [0, 2, 3]])


def near_far_mesh(w=128, h=96):
    """Identity view, fx = fy = 32, the principal point half a pixel past the centre (ray slopes (x - w/2) / 32: dyadic); a tilted dyadic plane z = 1 + 2 y (camera space) from z = 0.25 to z = 3 — the ray
    of row y meets it at z = 1 / (1 - 2 ry), ry = (y - h / 2) / fy, so exactly at 0.5 in the row ry = -1/2 and exactly at 2 in the row
    ry = 1/4 — in front of a fronto-parallel wall at z = 8; and a separate quad at z = 4.  Returns (cam, (V, T) of the tilted plane and
    the wall, (V, T) of the quad at z = 4, the rows at z = 0.5 and z = 2)."""
    cam = ref.cam_dict(w, h, 32.0, 32.0, w / 2 + 0.5, h / 2 + 0.5, np.eye(4))
    f = cam["fy"]
    Vp, Tp = _quad((-8.0, -0.375, 0.25), (8.0, -0.375, 0.25), (8.0, 1.0, 3.0), (-8.0, 1.0, 3.0))
    Vw, Tw = _quad((-64.0, -64.0, 8.0), (64.0, -64.0, 8.0), (64.0, 64.0, 8.0), (-64.0, 64.0, 8.0))
    V = np.concatenate([Vp, Vw]); T = np.concatenate([Tp, Tw + 4])
    Vq, Tq = _quad((-4.0, -2.0, 4.0), (4.0, -2.0, 4.0), (4.0, 1.0, 4.0), (-4.0, 1.0, 4.0))
    y_near, y_far = int(h // 2 - f / 2), int(h // 2 + f / 4)
    assert 0 <= y_near < h and 0 <= y_far < h
    return cam, (V, T), (Vq, Tq), y_near, y_far


def case_near_far_exact(drv, w=128, h=96):
    """z == far_z is visible, one ulp lower it is not; z == near_z is not (the surface behind shows)."""
    cam, (V, T), (Vq, Tq), y_near, y_far = near_far_mesh(w, h)
    # the quad at exactly z = far
    got, _ = drv.frame(Vq, Tq, cam, far=4.0)
    ref.check(got, ref.cast(Vq, Tq, cam, far=4.0), "quad at z == far")
    assert (got[np.isfinite(got)] == 4.0).all() and np.isfinite(got).sum() > w * h // 20, "quad at z == far_z: not visible"
    lower = float(np.nextafter(np.float32(4.0), np.float32(0.0)))
    got, _ = drv.frame(Vq, Tq, cam, far=lower)
    assert np.isinf(got).all(), f"quad at z == far_z: {int(np.isfinite(got).sum())} pixels visible with far_z one ulp lower"
    # the tilted plane: the row at exactly z == near shows the wall; the row at exactly z == far is visible, and not one ulp lower
    got, _ = drv.frame(V, T, cam, near=0.5)
    ref.check(got, ref.cast(V, T, cam, near=0.5), "tilted plane, near 0.5")
    assert (got[y_near] == 8.0).all(), f"row at z == near_z: {np.unique(got[y_near])[:4].tolist()} (want the wall at 8)"
    assert (got[y_near + 1] < 0.6).all() and (got[y_near - 1] == 8.0).all()
    got, _ = drv.frame(V, T, cam, near=0.2, far=2.0)
    ref.check(got, ref.cast(V, T, cam, near=0.2, far=2.0), "tilted plane, far 2")
    assert (got[y_far] == 2.0).all(), f"row at z == far_z: {np.unique(got[y_far])[:4].tolist()} (want 2)"
    assert np.isinf(got[y_far + 1]).all()
    got, _ = drv.frame(V, T, cam, near=0.2, far=float(np.nextafter(np.float32(2.0), np.float32(0.0))))
    assert np.isinf(got[y_far]).all() and (got[y_far - 1] < 2.0).all()


def case_far_straddle(drv, w=160, h=120):
    """A triangle from z = 2 to z = 6 through far_z = 4.  The right half of the frame has a wall at z = 3.5 behind it (inside far): there
    the wall hides the triangle past 3.5.  The left half has nothing behind it: there the triangle's part past far_z must be +inf, its
    part in (3.5, 4] visible — the per-pixel far test, not only the setup's cull."""
    cam = exact_cam(w, h)
    Vw, Tw = _quad((0.0, -8.0, 3.5), (8.0, -8.0, 3.5), (8.0, 8.0, 3.5), (0.0, 8.0, 3.5))
    Vt = np.array([[-1.5, -1.0, 2.0], [1.5, -0.5, 6.0], [-0.5, 1.2, 4.5]])
    V = np.concatenate([Vw, Vt]); T = np.concatenate([Tw, [[4, 5, 6]]])
    got, _ = drv.frame(V, T, cam, far=4.0)
    ref.check(got, ref.cast(V, T, cam, far=4.0), "triangle through far, wall on the right")
    tri = ref.cast(Vt, [[0, 1, 2]], cam, far=1e30)["nominal"]
    right = np.arange(w)[None, :] > w // 2 + 1
    left = np.arange(w)[None, :] < w // 2 - 1
    assert ((tri < 3.4) & (got < 3.4)).sum() > 200
    assert (right & (tri > 4.1) & np.isfinite(tri)).sum() > 100 and (got[right & (tri > 3.6) & np.isfinite(tri)] == np.float32(3.5)).all()
    beyond = left & (tri > 4.05) & np.isfinite(tri)
    inside = left & (tri > 3.6) & (tri < 3.95)
    assert beyond.sum() > 100 and np.isinf(got[beyond]).all(), "the part of the triangle beyond far_z is visible"
    assert inside.sum() > 50 and (np.abs(got[inside] / tri[inside] - 1) < 1e-5).all()


def case_collinear_exact(drv, w=128, h=96):
    """Exactly degenerate triangles under exact_cam (identity view, dyadic vertices): three vertices on one pixel row's ray plane, on a
    diagonal, and on a line through the camera — det = 0 exactly in the setup — in front of an exact lattice sheet, and repeated indices.
    The frame is bit for bit the sheet's, without NaN."""
    base = lattice_sheet(w, h, seed=2, step=8, exact=True)
    cam = base["cam"]
    rng = np.random.default_rng(2)
    P = []
    for k in range(24):
        y, x0, dx = int(rng.integers(8, h - 8)), int(rng.integers(4, w // 2)), int(rng.integers(2, 12))
        r0, r1, r3 = (_rays_uv(cam, np.array([x + 0.5]), np.array([yy + 0.5]))[0]
                      for x, yy in ((x0, y), (x0 + dx, y + (k % 2) * dx), (x0 + 3 * dx, y + (k % 2) * 3 * dx)))
        P += [0.5 * r0, 0.5 * r1, 0.5 * r3] if k % 3 else [0.5 * r0, 0.25 * r0, 0.75 * r0]      # a row / a diagonal / through the camera
    P = np.array(P)
    n = len(base["V"])
    Tc = n + np.arange(len(P)).reshape(-1, 3)
    Tc = np.concatenate([Tc, Tc[:, ::-1], np.stack([Tc[:, 0], Tc[:, 0], Tc[:, 1]], 1)])
    p0, p1, p2 = (P[Tc[:len(P) // 3, j] - n] for j in range(3))
    assert (np.einsum("ij,ij->i", np.cross(p1, p2), p0) == 0).all()               # the guard: exactly degenerate in camera space
    want, _ = drv.frame(base["V"], base["T"], cam)
    V = np.concatenate([base["V"], P])
    T = np.concatenate([base["T"], Tc])[rng.permutation(len(base["T"]) + len(Tc))]
    got, _ = drv.frame(V, T, cam)
    assert not np.isnan(got).any()
    assert np.array_equal(got, want), f"collinear triangles changed {int((got != want).sum())} pixels"


# ---- degenerate input --------------------------------------------------------------------------------------------------------------

def junk_triangles(room_V, cam, far, seed=0):
    """Triangles that cannot be hit: repeated indices of room vertices (into room_V), exactly collinear dyadic triples (model space, in
    front of the camera), and triangles wholly behind near_z, wholly beyond `far`, wholly left of the frame (camera space, moved to model
    space).  Returns (extra vertices, triangles indexing room_V + extra, the cull-only subset)."""
    rng = np.random.default_rng(seed)
    nv = len(room_V)
    i = rng.integers(0, nv, 60)
    j = rng.integers(0, nv, 60)
    rep = np.concatenate([np.stack([i[:20], i[:20], j[:20]], 1), np.stack([i[20:40], j[20:40], j[20:40]], 1),
                          np.stack([i[40:], i[40:], i[40:]], 1)])
    extra, tris, cull = [], [], []

    def add(P, model=False):
        base = nv + sum(len(q) for q in extra)
        extra.append(np.asarray(P, np.float64) if model else to_model(cam, np.asarray(P, np.float64)))
        return base + np.arange(len(P))

    # collinear: p, p + d, p + 3 d and p + 2 d, p, p - d, dyadic, around the room's middle
    for k in range(20):
        p = np.array([1.5, 1.25, 0.5]) + rng.integers(0, 16, 3) * 0.1875
        d = rng.integers(-4, 5, 3) * 0.0625
        d[0] = d[0] or 0.125
        ids = add([p, p + d, p + 3 * d, p - d], model=True)
        tris += [[ids[0], ids[1], ids[2]], [ids[2], ids[0], ids[3]]]
    behind = np.stack([rng.uniform(-0.5, 0.5, (20, 3)), rng.uniform(-0.5, 0.5, (20, 3)), rng.uniform(-1.0, 0.15, (20, 3))], -1)
    beyond = rng.uniform(-1, 1, (20, 3, 3)) * [10.0, 10.0, 0.0] + np.array([0.0, 0.0, 1.0]) * rng.uniform(far * 1.01, far * 1.5, (20, 3, 1))
    zl = rng.uniform(0.5, 4.0, (20, 3))
    left = np.stack([-(cam["cx"] / cam["fx"]) * zl * rng.uniform(1.05, 3.0, (20, 3)), rng.uniform(-1, 1, (20, 3)) * zl, zl], -1)
    for group in (behind, beyond, left):
        for tri in group:
            ids = add(tri)
            cull.append(ids.tolist())
    return np.concatenate(extra), np.concatenate([rep, np.array(tris), np.array(cull)]), np.array(cull)


def case_degenerate(drv, room, cam, far=20.0, seed=0):
    """The room with junk_triangles interleaved by permutation renders bit for bit as the room alone, without NaN; the cull-only junk
    adds no visible triangle and no record."""
    V0, T0 = room
    want, st0 = drv.frame(V0, T0, cam, near=0.2, far=far)
    extra, junk, cull = junk_triangles(V0, cam, far, seed)
    V = np.concatenate([V0, extra])
    rng = np.random.default_rng(seed + 1)
    T = np.concatenate([T0, junk])[rng.permutation(len(T0) + len(junk))]
    got, _ = drv.frame(V, T, cam, near=0.2, far=far)
    assert not np.isnan(got).any()
    assert np.array_equal(got, want), f"degenerate triangles changed {int((got != want).sum())} pixels"
    Tc = np.concatenate([T0, cull])[rng.permutation(len(T0) + len(cull))]
    got, st = drv.frame(V, Tc, cam, near=0.2, far=far)
    assert np.array_equal(got, want)
    assert st["n_visible"] == st0["n_visible"] and st["d_total"] == st0["d_total"], (st, st0)
    return want


# ---- more than 1024 tiles ------------------------------------------------------------------------------------------------------------

def many_tiles_mesh(w=528, h=528, seed=3):
    """A step-16 lattice sheet over the whole frame and, in front of it, a step-1 lattice over pixels [200, 232] x [512, 527]: the tiles
    of that patch (tile row 32 of 33, tiles 1056 .. 1088) list more than 512 triangles."""
    a = lattice_sheet(w, h, seed=seed, step=16, exact=True)
    b = lattice_sheet(w, h, seed=seed + 1, step=1, exact=True, region=(200, 232, 512, 527))
    Vb = b["V"] * 0.5                                               # the same rays, at z = 0.5 (a dyadic scale: still exact)
    return dict(V=np.concatenate([a["V"], Vb]), T=np.concatenate([a["T"], b["T"] + len(a["V"])]), cam=a["cam"])


def case_many_tiles(drv, w=528, h=528):
    """More than 1024 tiles (k_mesh_scan's carry across blocks of 1024) and lists longer than 512 records (several LDS chunks of 256 in
    k_mesh_depth, the last one partial), against the reference; the band of tile row 32 — wholly past tile 1024 — equals the full frame."""
    case = many_tiles_mesh(w, h)
    got, st = drv.frame(case["V"], case["T"], case["cam"])
    gx = (w + 15) // 16
    assert st["n_tiles"] > 1024 and 32 * gx >= 1024
    assert st["max_tile_len"] > 512, st
    ref.check(got, ref.cast(case["V"], case["T"], case["cam"]), f"{len(case['T'])} triangles {w}x{h}")
    band, _ = drv.frame(case["V"], case["T"], case["cam"], rows=(32, 33), fill=-5.0)
    assert np.isfinite(band[512:]).sum() > 400 and (band[:512] == -5.0).all()
    assert np.array_equal(band[512:], got[512:]), f"tile row 32: {int((band[512:] != got[512:]).sum())} pixels differ from the band"
    return st
