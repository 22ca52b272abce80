"""Collision-mesh depth (sgs_render_mesh_depth*) under the wave64 emulator: the product's kernels (csrc/sgs_mesh.h) against the fp64
ray caster of tests/mesh_depth_ref.py, the ABI's refusals, and the USDA mesh reader.  CPU only."""
import json
import math
import os

import numpy as np
import pytest

import emu_harness as eh
import mesh_depth_ref as ref
import mesh_edge_cases as mc
from sage_gs import _capi, scenes
from sage_gs import mesh as mesh_io

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    return eh.lib()


Emu = mc.EmuMesh


@pytest.fixture
def emu(lib):
    e = Emu(lib)
    yield e
    e.close()


def _cam(w, h, pos, yaw, pitch=0.0):
    fx, fy, cx, cy = scenes.reference_intrinsics(w, h)
    return ref.cam_dict(w, h, fx, fy, cx, cy, scenes.view_from_yaw(pos, yaw, pitch))


def test_reference_matches_closed_form_box():
    """The reference itself: inside an axis-aligned box room, depth = min over the faces of d / (n . r) among hits with z > near."""
    lo, hi = np.zeros(3), np.array([6.0, 5.0, 2.8], np.float32).astype(np.float64)      # (the caster rounds vertices to fp32)
    V, T = scenes.grid_box(lo, hi, (3, 2, 2))
    for k, (pos, yaw, pitch) in enumerate([((2.0, 1.5, 1.2), 0.3, 0.1), ((4.5, 3.9, 0.7), 2.5, -0.4), ((1.0, 4.0, 2.0), 4.0, 0.6)]):
        cam = _cam(64, 48, pos, yaw, pitch)
        r = ref.cast(V, T, cam, near=0.2)
        ys, xs = np.divmod(np.arange(64 * 48), 64)
        rays = np.stack([(xs + 0.5 - cam["cx"]) / cam["fx"], (ys + 0.5 - cam["cy"]) / cam["fy"], np.ones(len(xs))], 1)
        Rm, t = cam["view"][:3, :3], cam["view"][:3, 3]
        Ri = np.linalg.inv(Rm)                          # (the fp32-rounded view is orthonormal to ~1e-7 only)
        c = -Ri @ t
        d = rays @ Ri.T                                 # world direction per unit camera z
        with np.errstate(divide="ignore"):
            tt = np.where(d > 0, (hi - c) / d, (lo - c) / d)
        want = np.min(np.where(tt > 0, tt, np.inf), axis=1).reshape(48, 64)
        assert np.isfinite(r["nominal"]).all()
        assert np.abs(r["nominal"] / want - 1).max() < 1e-9, k
        assert (r["lenient"] <= want).all() and (want <= r["strict"]).all()


def test_reference_oblique_and_straddling_triangles():
    """One oblique triangle through the camera plane: where the ray meets it (solved by barycentrics) with z > near, depth is z."""
    cam = ref.cam_dict(64, 48, 40.0, 40.0, 32.0, 24.0, np.eye(4))
    V = np.array([[-3.0, -2.0, -1.0], [3.0, -1.0, 4.0], [-1.0, 3.0, 2.5]])
    T = np.array([[0, 1, 2]])
    r = ref.cast(V, T, cam, near=0.2)
    ys, xs = np.divmod(np.arange(64 * 48), 64)
    want = np.full(64 * 48, np.inf)
    for i in range(len(xs)):
        d = np.array([(xs[i] + 0.5 - 32) / 40.0, (ys[i] + 0.5 - 24) / 40.0, 1.0])
        A = np.stack([V[1] - V[0], V[2] - V[0], -d], 1)
        b1, b2, tz = np.linalg.solve(A, -V[0])
        if b1 >= 0 and b2 >= 0 and b1 + b2 <= 1 and tz > 0.2:
            want[i] = tz
    want = want.reshape(48, 64)
    assert np.isfinite(want).sum() > 200 and np.isinf(want).sum() > 200            # it covers part of the frame, and straddles z = 0
    fin = np.isfinite(want) & ~r["edge"]
    assert np.abs(r["nominal"][fin] / want[fin] - 1).max() < 1e-9
    assert (np.isinf(r["nominal"]) == np.isinf(want))[~r["edge"]].all()


@pytest.mark.parametrize("w,h", [(64, 48), (160, 120), (320, 240)])
def test_room_mesh_against_reference(emu, w, h):
    m = scenes.make_room_mesh(3000, seed=2)
    hm = emu.mesh(m.vertices, m.triangles)
    rng = np.random.default_rng(w)
    for k in range(2):
        cam = _cam(w, h, (rng.uniform(1.2, 4.8), rng.uniform(1.2, 3.8), 1.2), rng.uniform(0, 2 * math.pi), rng.uniform(-0.5, 0.5))
        rc, out, st = emu.render(hm, cam)
        emu.lib.check(rc, emu.ctx)
        ref.check(out, ref.cast(m.vertices, m.triangles, cam, near=0.2), f"room {w}x{h} pose {k}")
        assert not np.isinf(out).any()                                              # closed room: no pixel sees out
        assert st["n_visible"] > 0 and st["d_total"] >= st["n_visible"] and st["n_tiles"] == ((w + 15) // 16) * ((h + 15) // 16)
        assert st["n_pixels"] == w * h and st["max_tile_len"] > 0


def test_near_plane_straddling_and_inside_box(emu):
    """Large triangles through the camera plane (a floor and a wall running past the camera), and a camera inside a closed box."""
    V = np.array([[-5, 1.0, -4], [5, 1.0, -4], [0, 1.0, 9], [-2, -3, -3], [-2, 3, 6], [-2, -3, 6]], np.float64)
    T = np.array([[0, 1, 2], [3, 4, 5]])
    cam = ref.cam_dict(96, 64, 50.0, 50.0, 48.0, 32.0, np.eye(4))
    hm = emu.mesh(V, T)
    for near in (0.2, 1.5):
        rc, out, _ = emu.render(hm, cam, cfg=emu.cfg(near=near))
        emu.lib.check(rc, emu.ctx)
        ref.check(out, ref.cast(V, T, cam, near=near), f"straddling near={near}")
        assert np.isfinite(out).sum() > 1000
    Vb, Tb = scenes.grid_box((-1, -1, -1), (1, 1, 1), (1, 1, 1))            # 12 big triangles around the camera
    hb = emu.mesh(Vb, Tb)
    cam = ref.cam_dict(64, 48, 30.0, 30.0, 32.0, 24.0, scenes.view_from_yaw((0.1, -0.2, 0.05), 0.7, 0.3))
    rc, out, _ = emu.render(hb, cam)
    emu.lib.check(rc, emu.ctx)
    ref.check(out, ref.cast(Vb, Tb, cam), "inside a box")
    assert np.isfinite(out).all()


def test_invariants_band_batch_permutation(emu):
    m = scenes.make_room_mesh(2000, seed=5)
    hm = emu.mesh(m.vertices, m.triangles)
    cams = [_cam(80, 60, (2.0 + 0.3 * k, 2.5, 1.2), 0.9 * k, 0.1) for k in range(3)]
    singles = [emu.render(hm, c)[1] for c in cams]
    got, st = emu.batch(hm, cams)
    assert all((got[k] == singles[k]).all() for k in range(3))
    assert st[1]["d_total"] > 0
    rc, band, _ = emu.render(hm, cams[1], rows=(1, 3), fill=-7.0)
    emu.lib.check(rc, emu.ctx)
    assert (band[16:48] == singles[1][16:48]).all() and (band[:16] == -7.0).all() and (band[48:] == -7.0).all()
    perm = np.random.default_rng(0).permutation(len(m.triangles))
    tri = m.triangles[perm][:, [1, 2, 0]]                                   # other order, other first vertex
    hp = emu.mesh(m.vertices, tri)
    assert (emu.render(hp, cams[1])[1] == singles[1]).all()
    # a deliberately small record buffer: the frame is rendered again, identically
    emu.lib.check(emu.lib.sgs_mesh_set_record_capacity(emu.ctx, 64), emu.ctx)
    rc, again, st2 = emu.render(hm, cams[1])
    emu.lib.check(rc, emu.ctx)
    assert st2["retries"] > 0 and (again == singles[1]).all()


def test_empty_mesh_is_all_inf(emu):
    hm = emu.mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    rc, out, st = emu.render(hm, _cam(48, 32, (0, 0, 0), 0.0))
    emu.lib.check(rc, emu.ctx)
    assert np.isinf(out).all() and (out > 0).all() and st["d_total"] == 0 and st["n_visible"] == 0


def test_abi_refusals(emu):
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    rc, h = emu.upload(V, np.array([[0, 1, 3]]))
    assert rc == -1 and not h.value and "indices" in emu.err()
    rc, h = emu.upload(V, np.array([[0, -1, 2]]))
    assert rc == -1 and not h.value
    rc, h = emu.upload(np.array([[0, 0, 0], [1, np.nan, 0], [0, 1, 0]]), np.array([[0, 1, 2]]))
    assert rc == -1 and not h.value and "non-finite" in emu.err()
    rc, h = emu.upload(np.array([[0, 0, 0], [1, np.inf, 0], [0, 1, 0]]), np.array([[0, 1, 2]]))
    assert rc == -1 and not h.value
    hm = emu.mesh(V + [0, 0, 2], np.array([[0, 1, 2]]))
    cam = _cam(32, 32, (0, 0, 0), 0.0)
    assert emu.render(hm, cam, cfg=emu.cfg(stride=2))[0] == -1 and "interleaved" in emu.err()
    assert emu.render(hm, cam, cfg=emu.cfg(flags=_capi.FLAG_ASYNC))[0] == -1 and "synchronous" in emu.err()
    bad = dict(cam, view=cam["view"] @ np.diag([1.01, 1.0, 1.0, 1.0]))
    assert emu.render(hm, bad)[0] == -1 and "rigid" in emu.err()
    assert emu.render(hm, cam, cfg=emu.cfg(near=0.0))[0] == -1
    assert emu.lib.sgs_mesh_set_record_capacity(emu.ctx, 0) == -1
    emu.lib.check(emu.render(hm, cam)[0], emu.ctx)                          # the context still works


USDA = '''#usda 1.0
(
    defaultPrim = "Root"
    metersPerUnit = 0.01
    upAxis = "Z"
)

def Xform "Root"
{
    double3 xformOp:translate = (100, 0, 0)   # centimetres
    uniform token[] xformOpOrder = ["xformOp:translate"]

    def Xform "Inner" (
        kind = "component"
    )
    {
        quatf xformOp:orient = (6.123234e-17, 0, 0, 1)
        float3 xformOp:scale = (2, 2, 2)
        uniform token[] xformOpOrder = ["xformOp:orient", "xformOp:scale"]

        def Mesh "quad"
        {
            int[] faceVertexCounts = [4, 3]
            int[] faceVertexIndices = [0, 1, 2, 3, 1, 4, 2]
            point3f[] points = [(0, 0, 0), (10, 0, 0), (10, 10, 0), (0, 10, 0), (20, 5, 5)]
        }
    }
    def Mesh "tri"
    {
        double3 xformOp:translate = (0, 0, 50)
        uniform token[] xformOpOrder = ["xformOp:translate"]
        int[] faceVertexCounts = [3]
        int[] faceVertexIndices = [0, 1, 2]
        point3f[] points = [(0, 0, 0), (0, 100, 0), (0, 0, 100)]
    }
}
'''


def test_read_usda_mesh(tmp_path):
    p = tmp_path / "m.usda"
    p.write_text(USDA)
    V, T = mesh_io.read_usda_mesh(str(p))
    assert T.tolist() == [[0, 1, 2], [0, 2, 3], [1, 4, 2], [5, 6, 7]]
    # quad: scale 2, then Rz(180), then translate 100 cm; all times 0.01 m
    def place(q):
        return 0.01 * (np.array([100.0, 0, 0]) + np.array([-2 * q[0], -2 * q[1], 2 * q[2]]))
    want = [place(q) for q in [(0, 0, 0), (10, 0, 0), (10, 10, 0), (0, 10, 0), (20, 5, 5)]]
    want += [0.01 * (np.array([100.0, 0, 50]) + np.array(q)) for q in [(0, 0, 0), (0, 100, 0), (0, 0, 100)]]
    assert np.abs(V - np.array(want)).max() < 1e-12


def test_crate_file_is_refused(tmp_path):
    p = tmp_path / "c_collision.usd"
    p.write_bytes(b"PXR-USDC" + bytes(64))
    with pytest.raises(ValueError, match="usdcat"):
        mesh_io.read_usda_mesh(str(p))


def test_collision_transform_of_the_template_is_rz180():
    from sage_gs import adapter
    from test_next_rows import _serialise_prim
    g = json.load(open(os.path.join(HERE, "golden", "usda_golden.json")))
    text = '#usda 1.0\n(\n    metersPerUnit = 1\n    upAxis = "Z"\n)\n\ndef Xform "World"\n{\n' + _serialise_prim(g["gauss"]) + \
        _serialise_prim(g["scene_collision"]) + '}\n'
    parsed = adapter.parse_scene_usda(text)
    M = adapter.collision_model_to_world(parsed)
    Rz = np.diag([-1.0, -1.0, 1.0, 1.0])
    assert np.abs(M - Rz).max() < 1e-6, M
    assert parsed["collision"].endswith("_collision.usd")
