"""Cases of the collision-mesh object-id channel (sgs_render_mesh_ids*), shared by the emulator tests (test_emu_mesh_ids.py) and the GPU
tests (test_gpu_mesh_ids.py).  Every case takes a driver — EmuIds (the wave64 emulator, through the C ABI) or GpuIds (a sage_gs Renderer)
— and raises AssertionError when the frames are wrong.  The value rule and the checker are in tests/mesh_id_ref.py; cameras are
mesh_depth_ref.cam_dict dictionaries, as in mesh_edge_cases.py.

Every frame a case renders also goes through `_both`: the depth returned beside the ids must equal render_mesh_depth's frame bit for bit
(the "depth identity" of the channel's contract), on every case.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import mesh_depth_ref as ref
import mesh_id_ref as idref
from mesh_edge_cases import GpuMesh
from sage_gs import _capi, scenes

NONE = idref.ID_NONE
FILL_ID, FILL_Z = -7, -7.0
REFUSED = (_capi.SgsError, ValueError)

# room_cameras(make_room_mesh(n), w, h, n_positions=4, n_yaw=4, seed=0): the poses at which the REFERENCE ALONE (mesh_id_ref.admissible,
# labels = make_room_mesh_parts' part) gives >= 90 % decided pixels and >= 6 distinct decided labels — chosen on the CPU; 6 of the 16
# poses qualify, the same six for both meshes (2 000 and 20 000 triangles) and both frames (160x120, 33x17).  The others look at a wall
# with fewer than six objects in view (3 to 5 decided labels); none fails the 90 %.
ROOM_POSES = (0, 3, 4, 8, 12, 15)
MIN_DECIDED, MIN_LABELS = 0.90, 6


# ---- drivers -----------------------------------------------------------------------------------------------------------------------

class EmuIds:
    """sgs_render_mesh_ids* of an emulator library (host pointers: the emulator's 'device' is the host)."""

    def __init__(self, lib):
        self.lib = lib
        self.ctx = C.c_void_p()
        lib.check(lib.sgs_create(0, _capi.BACKEND_HIP, C.byref(self.ctx)))

    def mesh(self, V, T, labels=None):
        v = np.ascontiguousarray(V, np.float32); t = np.ascontiguousarray(T, np.int32)
        h = C.c_void_p()
        self.lib.check(self.lib.sgs_mesh_upload(self.ctx, len(v), v.ctypes.data if len(v) else None, len(t),
                                                t.ctypes.data if len(t) else None, 0, C.byref(h)), self.ctx)
        if labels is not None:
            self.set_labels(h, labels)
        return h

    def set_labels(self, m, labels, on_device=False):
        a = None if labels is None else np.ascontiguousarray(labels, np.int32)
        self.lib.check(self.lib.sgs_mesh_set_labels(self.ctx, m, None if a is None else a.ctypes.data, 0), self.ctx)

    def free(self, m):
        self.lib.sgs_mesh_free(self.ctx, m)

    def _cfg(self, near, far, flags=0, stride=1):
        k = self.lib.default_config()
        k.near_z, k.far_z, k.flags, k.tile_row_stride = near, far, flags, stride
        return k

    @staticmethod
    def _cam(cam):
        return _capi.make_camera(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["view"].tolist())

    def ids(self, m, cam, near=0.2, far=1e30, rows=(0, -1), depth=True, flags=0, stride=1):
        """(ids, depth or None, stats): both buffers pre-filled with FILL_ID / FILL_Z."""
        out = np.full((cam["height"], cam["width"]), FILL_ID, np.int32)
        z = np.full((cam["height"], cam["width"]), FILL_Z, np.float32) if depth else None
        st = _capi.SgsStats()
        c, k = self._cam(cam), self._cfg(near, far, flags, stride)
        self.lib.check(self.lib.sgs_render_mesh_ids(self.ctx, m, C.byref(c), C.byref(k), rows[0], rows[1], z.ctypes.data if depth else None,
                                                    out.ctypes.data, C.byref(st), None), self.ctx)
        return out, z, st.as_dict()

    def depth(self, m, cam, near=0.2, far=1e30, rows=(0, -1)):
        out = np.full((cam["height"], cam["width"]), FILL_Z, np.float32)
        c, k = self._cam(cam), self._cfg(near, far)
        self.lib.check(self.lib.sgs_render_mesh_depth(self.ctx, m, C.byref(c), C.byref(k), rows[0], rows[1], out.ctypes.data, None, None), self.ctx)
        return out

    def ids_batch(self, m, cams, near=0.2, far=1e30):
        arr = (_capi.SgsCamera * len(cams))(*[self._cam(c) for c in cams])
        out = np.full((len(cams), cams[0]["height"], cams[0]["width"]), FILL_ID, np.int32)
        z = np.full(out.shape, FILL_Z, np.float32)
        k = self._cfg(near, far)
        self.lib.check(self.lib.sgs_render_mesh_ids_batch(self.ctx, m, arr, len(cams), C.byref(k), z.ctypes.data, out.ctypes.data, None, None),
                       self.ctx)
        return out, z

    def set_capacity(self, n):
        self.lib.check(self.lib.sgs_mesh_set_record_capacity(self.ctx, int(n)), self.ctx)

    def close(self):
        if self.ctx:
            self.lib.sgs_destroy(self.ctx)
            self.ctx = C.c_void_p()


class GpuIds:
    """The same interface over a sage_gs Renderer (device frames copied back to the host)."""

    def __init__(self, renderer):
        self.r = renderer

    def mesh(self, V, T, labels=None):
        return self.r.upload_mesh(V, T, labels=None if labels is None else np.asarray(labels, np.int32))

    def set_labels(self, m, labels, on_device=False):
        """on_device: hand the library a device tensor, so that ITS check of the range runs (a host array is checked in Python first)."""
        import torch
        if labels is not None:
            labels = np.asarray(labels, np.int32)
            if on_device:
                labels = torch.from_numpy(labels).to(self.r.device)
        self.r.set_mesh_labels(m, labels)

    def free(self, m):
        m.free()

    def ids(self, m, cam, near=0.2, far=1e30, rows=(0, -1), depth=True, flags=0, stride=1):
        import torch
        h, w = cam["height"], cam["width"]
        out = torch.full((h, w), FILL_ID, dtype=torch.int32, device=self.r.device)
        z = torch.full((h, w), FILL_Z, dtype=torch.float32, device=self.r.device) if depth else None
        if flags or stride != 1:                         # what Renderer.render_mesh_ids never asks for: straight to the library
            r = self.r
            cfg = r._c_config(GpuMesh.config(near, far), flags)
            cfg.tile_row_stride = stride
            c = r._c_camera(GpuMesh.camera(cam), m)
            r._lib.check(r._lib.sgs_render_mesh_ids(r._ctx, m.handle, C.byref(c), C.byref(cfg), rows[0], rows[1],
                                                    z.data_ptr() if depth else None, out.data_ptr(), None, r._stream()), r._ctx)
            return out.cpu().numpy(), z.cpu().numpy() if depth else None, {}
        self.r.render_mesh_ids(GpuMesh.camera(cam), m, config=GpuMesh.config(near, far), tile_rows=None if rows == (0, -1) else rows,
                               out=out, out_depth=z)
        return out.cpu().numpy(), z.cpu().numpy() if depth else None, dict(self.r.last_stats)

    def depth(self, m, cam, near=0.2, far=1e30, rows=(0, -1)):
        import torch
        out = torch.full((cam["height"], cam["width"]), FILL_Z, dtype=torch.float32, device=self.r.device)
        self.r.render_mesh_depth(GpuMesh.camera(cam), m, config=GpuMesh.config(near, far), tile_rows=None if rows == (0, -1) else rows, out=out)
        return out.cpu().numpy()

    def ids_batch(self, m, cams, near=0.2, far=1e30):
        ids, z = self.r.render_mesh_ids_batch([GpuMesh.camera(c) for c in cams], m, config=GpuMesh.config(near, far), return_depth=True)
        return ids.cpu().numpy(), z.cpu().numpy()

    def set_capacity(self, n):
        self.r.set_mesh_record_capacity(int(n))

    def close(self):
        pass


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _both(drv, m, cam, what, **kw):
    """One id frame with its depth — which must be render_mesh_depth's frame bit for bit (case 6) — and the ids alone, which must not
    depend on whether the depth is asked for."""
    ids, z, st = drv.ids(m, cam, **kw)
    want = drv.depth(m, cam, **kw)
    assert np.array_equal(_bits(z), _bits(want)), f"{what}: the depth beside the ids differs from render_mesh_depth at {int((_bits(z) != _bits(want)).sum())} pixels"
    alone, none, _ = drv.ids(m, cam, depth=False, **kw)
    assert none is None and np.array_equal(alone, ids), f"{what}: the ids depend on whether the depth is written"
    assert ids.dtype == np.int32
    return ids, z, st


# ---- 1. against the reference --------------------------------------------------------------------------------------------------------

_ROOMS = {}


def room(n):
    """(V, T, part, RoomMesh) of make_room_mesh_parts(n), built once."""
    if n not in _ROOMS:
        V, T, part = scenes.make_room_mesh_parts(n)
        _ROOMS[n] = (V, T, part, scenes.make_room_mesh(n))
    return _ROOMS[n]


_ADM = {}


def room_reference(n, w, h, pose):
    """(cam, admissible sets) of one ROOM_POSES pose: computed once, shared by the tests that need it, never modified."""
    key = (n, w, h, pose)
    if key not in _ADM:
        V, T, part, rm = room(n)
        cam = ref.of_camera(scenes.room_cameras(rm, w, h, n_positions=4, n_yaw=4, seed=0)[pose])
        _ADM[key] = (cam, idref.admissible(V, T, part, cam))
    return _ADM[key]


def case_reference(drv, n, w, h, poses=ROOM_POSES):
    """Every pixel's id is admissible and its depth passes mesh_depth_ref.check; the reference alone decides >= 90 % of the pixels and
    >= 6 distinct labels of every pose (asserted: the check cannot pass by leaving everything undecided)."""
    V, T, part, _ = room(n)
    m = drv.mesh(V, T, part)
    try:
        for pose in poses:
            cam, adm = room_reference(n, w, h, pose)
            what = f"room {n} {w}x{h} pose {pose}"
            ids, z, st = _both(drv, m, cam, what)
            share, n_labels = idref.check(ids, adm, what)
            assert share >= MIN_DECIDED and n_labels >= MIN_LABELS, (what, share, n_labels)
            ref.check(z, adm["ref"], what)
            assert (ids != NONE).all() and st["n_pixels"] == w * h                 # a closed room: no pixel sees out
            assert set(np.unique(ids).tolist()) <= set(range(12))
    finally:
        drv.free(m)


# ---- 2 .. 4: known answers -----------------------------------------------------------------------------------------------------------

def quad_cam(w=64, h=48):
    return ref.cam_dict(w, h, 40.0, 40.0, w / 2, h / 2, np.eye(4))


def quad(z, half=0.8):
    """(V, T) of a square of side 2 * half at depth z, facing the identity camera: triangles (0, 1, 2) and (0, 2, 3)."""
    return np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], np.float64), np.array([[0, 1, 2], [0, 2, 3]])


def _strict_masks(V, T, cam, near=0.2):
    """Per triangle the pixels whose centre is strictly inside it (every edge function > eps), and the pixels no triangle can claim
    (some edge function < -eps for every triangle), with the module's eps."""
    W, H = cam["width"], cam["height"]
    ys, xs = np.divmod(np.arange(W * H), W)
    inside = np.zeros((len(T), W * H), bool)
    claim = np.zeros(W * H, bool)
    for pix, t, s, eps, z, tol in ref._candidates(V, T, cam, near, xs, ys, 1 << 21):
        k = (s > eps).all(1)
        inside[t[k], pix[k]] = True
        claim[pix[(s >= -eps).all(1)]] = True
    return inside.reshape(len(T), H, W), ~claim.reshape(H, W)


def case_known_answer(drv):
    """One quad of two triangles at z = 2, labels 5 and 9: a pixel strictly inside a triangle gets its label and depth 2.0, a pixel
    outside the quad -1 and +inf, a pixel on the diagonal 5 or 9."""
    cam = quad_cam()
    V, T = quad(2.0)
    m = drv.mesh(V, T, [5, 9])
    try:
        ids, z, _ = _both(drv, m, cam, "quad")
        inside, outside = _strict_masks(V, T, cam)
        assert inside[0].sum() > 200 and inside[1].sum() > 200 and outside.sum() > 1000
        assert (ids[inside[0]] == 5).all() and (ids[inside[1]] == 9).all(), "a pixel strictly inside a triangle has another label"
        assert (z[inside[0] | inside[1]] == 2.0).all()
        assert (ids[outside] == NONE).all() and np.isposinf(z[outside]).all(), "a pixel outside the quad is not (-1, +inf)"
        rest = ~(inside[0] | inside[1] | outside)
        assert np.isin(ids[rest], [5, 9, NONE]).all() and ((ids[rest] == NONE) == np.isposinf(z[rest])).all()
        diag = rest & (np.abs(np.add.outer(np.arange(48) - 23.5, -(np.arange(64) - 31.5))) < 0.25)      # pixel centres on y = x (camera)
        assert diag.sum() >= 30 and np.isin(ids[diag], [5, 9]).all(), "a pixel on the diagonal is neither 5 nor 9"
    finally:
        drv.free(m)


def case_tie_rule(drv):
    """The same triangle listed twice (thrice): bit-equal z at every covered pixel, the least label wins whatever the order."""
    cam = quad_cam()
    V, T = quad(2.0)
    covered = None
    for tri, labels, want in (([0, 0], (7, 3), 3), ([0, 0], (3, 7), 3), ([0, 0, 0], (4, 4, 1), 1), ([0, 0, 0], (1, 4, 4), 1)):
        m = drv.mesh(V, T[tri], labels)
        try:
            ids, z, _ = _both(drv, m, cam, f"tie {labels}")
        finally:
            drv.free(m)
        hit = ids != NONE
        assert hit.sum() > 200 and (ids[hit] == want).all(), f"labels {labels}: {np.unique(ids[hit]).tolist()} (want {want})"
        assert (np.isfinite(z) == hit).all()
        assert covered is None or np.array_equal(hit, covered)
        covered = hit


def case_nearest_wins(drv):
    """Two parallel quads at z = 2 (label 1) and z = 3 (label 2), the farther one larger: the nearer label where both are hit, in both
    triangle orders; with the near plane between them, label 2."""
    cam = quad_cam()
    Va, Ta = quad(2.0, 0.4)
    Vb, Tb = quad(3.0, 1.0)
    V = np.concatenate([Va, Vb])
    ins_a, _ = _strict_masks(Va, Ta, cam)
    ins_b, _ = _strict_masks(Vb, Tb, cam)
    a, b = ins_a.any(0), ins_b.any(0)
    assert (a & b).sum() > 200 and (b & ~a).sum() > 200
    for T, labels in ((np.concatenate([Ta, Tb + 4]), [1, 1, 2, 2]), (np.concatenate([Tb + 4, Ta]), [2, 2, 1, 1])):
        m = drv.mesh(V, T, labels)
        try:
            ids, z, _ = _both(drv, m, cam, f"two quads {labels}")
            assert (ids[a] == 1).all() and (z[a] == 2.0).all(), "the farther surface's label where the nearer one is hit"
            _, out_a = _strict_masks(Va, Ta, cam)
            assert (ids[b & out_a] == 2).all() and (z[b & out_a] == 3.0).all()
            ids, z, _ = _both(drv, m, cam, f"two quads {labels}, near 2.5", near=2.5)
            assert (ids[b] == 2).all() and (z[b] == 3.0).all(), "near plane between the quads: not the farther quad's label"
            assert not (ids == 1).any()
        finally:
            drv.free(m)


# ---- 5. independence of issue ----------------------------------------------------------------------------------------------------------

def case_issue_independence(drv, n=2000, w=80, h=60):
    """Bit for bit: a batch of 9 frames (two groups) against the frames alone; a band of tile rows against the full frame, the rows outside
    it untouched in both outputs; a permutation of the triangles that carries the labels along; a record buffer forced small."""
    V, T, part, rm = room(n)
    fx, fy, cx, cy = scenes.reference_intrinsics(w, h)
    cams = [ref.cam_dict(w, h, fx, fy, cx, cy, scenes.view_from_yaw((2.0 + 0.25 * k, 2.5, 1.2), 0.7 * k, 0.1)) for k in range(9)]
    m = drv.mesh(V, T, part)
    try:
        singles = [_both(drv, m, c, f"single {k}") for k, c in enumerate(cams)]
        assert len({s[0].tobytes() for s in singles}) == 9                       # nine different frames
        bi, bz = drv.ids_batch(m, cams)
        for k in range(9):
            assert np.array_equal(bi[k], singles[k][0]), f"batch frame {k}: {int((bi[k] != singles[k][0]).sum())} ids differ from the frame alone"
            assert np.array_equal(_bits(bz[k]), _bits(singles[k][1])), f"batch frame {k}: depth differs"
        full_i, full_z, _ = singles[4]
        r0, r1 = 1, 3
        band_i, band_z, _ = _both(drv, m, cams[4], "band", rows=(r0, r1))
        y0, y1 = 16 * r0, min(16 * r1, h)
        assert np.array_equal(band_i[y0:y1], full_i[y0:y1]) and np.array_equal(_bits(band_z[y0:y1]), _bits(full_z[y0:y1]))
        assert (band_i[:y0] == FILL_ID).all() and (band_i[y1:] == FILL_ID).all(), "the band wrote ids outside its rows"
        assert (band_z[:y0] == FILL_Z).all() and (band_z[y1:] == FILL_Z).all(), "the band wrote depth outside its rows"
        perm = np.random.default_rng(0).permutation(len(T))
        mp = drv.mesh(V, T[perm][:, [1, 2, 0]], part[perm])
        try:
            pi, pz, _ = _both(drv, mp, cams[4], "permuted")
            assert np.array_equal(pi, full_i), f"permuted triangles: {int((pi != full_i).sum())} ids differ"
            assert np.array_equal(_bits(pz), _bits(full_z))
        finally:
            drv.free(mp)
        drv.set_capacity(64)                                                     # too small: the frame is rendered again after growth
        gi, gz, st = drv.ids(m, cams[4])
        assert st["retries"] > 0, st
        assert np.array_equal(gi, full_i) and np.array_equal(_bits(gz), _bits(full_z))
    finally:
        drv.free(m)


# ---- 7. long lists -------------------------------------------------------------------------------------------------------------------

def case_long_list(drv, copies=600):
    """600 copies of a small triangle inside one tile, at increasing depth, labels reversed (the nearest has the largest): the tile's
    list crosses the LDS staging batch of 256 twice, and the nearest copy's label wins at its pixels."""
    cam = quad_cam()
    zs = 1.0 + 0.01 * np.arange(copies)
    r = np.array([[(34.5 - 32) / 40, (18.5 - 24) / 40, 1.0], [(45.5 - 32) / 40, (19.5 - 24) / 40, 1.0], [(38.5 - 32) / 40, (29.5 - 24) / 40, 1.0]])
    V = (zs[:, None, None] * r[None]).reshape(-1, 3)                              # every copy covers the same pixels of tile (2, 1)
    T = np.arange(3 * copies).reshape(-1, 3)
    labels = np.arange(copies)[::-1].copy()
    perm = np.random.default_rng(1).permutation(copies)                           # the nearest is somewhere in the middle of the list
    m = drv.mesh(V, T[perm], labels[perm])
    try:
        ids, z, st = _both(drv, m, cam, "600 copies")
        assert st["max_tile_len"] >= copies > 512, st
        inside, outside = _strict_masks(V[:3], T[:1], cam)
        assert inside[0].sum() > 30
        assert (ids[inside[0]] == copies - 1).all(), f"the nearest copy's label is {copies - 1}; got {np.unique(ids[inside[0]]).tolist()[:8]}"
        assert (np.abs(z[inside[0]] - 1.0) < 1e-6).all() and (ids[outside] == NONE).all()
        ids, z, _ = _both(drv, m, cam, "600 copies, near between", near=float(zs[299] + 0.005))
        assert (ids[inside[0]] == copies - 1 - 300).all()                        # the first 300 copies are cut: the 301st is nearest
    finally:
        drv.free(m)


# ---- 8. defaults and refusals ----------------------------------------------------------------------------------------------------------

def case_defaults_and_refusals(drv):
    """Without labels the id is the triangle's index; labels=None after a set restores that; a negative label is refused (by the library,
    on the device) and the earlier labels still render; interleaved rows and the asynchronous flags are refused as for depth."""
    import pytest
    cam = quad_cam()
    V, T = quad(2.0)
    inside, outside = _strict_masks(V, T, cam)
    m = drv.mesh(V, T)
    try:
        ids, _, _ = _both(drv, m, cam, "default labels")
        assert (ids[inside[0]] == 0).all() and (ids[inside[1]] == 1).all() and (ids[outside] == NONE).all()
        drv.set_labels(m, [11, 4])
        ids, _, _ = _both(drv, m, cam, "labels 11, 4")
        assert (ids[inside[0]] == 11).all() and (ids[inside[1]] == 4).all()
        for bad in ([3, -1], [-5, 2], [2 ** 31 - 1, 0]):
            with pytest.raises(REFUSED, match="labels"):
                drv.set_labels(m, bad, on_device=True)
            again, _, _ = drv.ids(m, cam)
            assert np.array_equal(again, ids), "a refused set_labels changed the mesh's labels"
        drv.set_labels(m, [2 ** 31 - 2, 0])                                       # the largest label there is
        big, _, _ = drv.ids(m, cam)
        assert (big[inside[0]] == 2 ** 31 - 2).all() and (big[inside[1]] == 0).all()
        drv.set_labels(m, None)
        back, _, _ = drv.ids(m, cam)
        assert (back[inside[0]] == 0).all() and (back[inside[1]] == 1).all()
        with pytest.raises(REFUSED, match="interleaved"):
            drv.ids(m, cam, stride=2)
        for fl in (_capi.FLAG_ASYNC, _capi.FLAG_PIPELINED):
            with pytest.raises(REFUSED, match="synchronous"):
                drv.ids(m, cam, flags=fl)
        ok, _, _ = drv.ids(m, cam)                                                # the context still works
        assert np.array_equal(ok, back)
    finally:
        drv.free(m)
    e = drv.mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32))                    # an empty mesh: nothing is hit anywhere
    try:
        ids, z, _ = _both(drv, e, cam, "empty mesh")
        assert (ids == NONE).all() and np.isposinf(z).all()
    finally:
        drv.free(e)
