"""Collision-mesh depth on the MI355X (sgs_render_mesh_depth*): frames against the fp64 ray caster of tests/mesh_depth_ref.py,
watertightness, the bit-exact invariants, the record buffer's regrowth, and the Isaac-facing depth (GsCamera, isaac_shim)."""
import math
import os

import numpy as np
import pytest

import mesh_depth_ref as ref
import mesh_edge_cases as mc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def r():
    import torch
    from sage_gs import Renderer
    assert torch.cuda.is_available()
    rr = Renderer("cuda:0")
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def room():
    from sage_gs import scenes
    return scenes.make_room_mesh(50_000, seed=1)


@pytest.fixture(scope="module")
def room_mesh(r, room):
    return r.upload_mesh(room.vertices, room.triangles)


def _cams(room, w, h, n=16, seed=0):
    from sage_gs import scenes
    return scenes.room_cameras(room, w, h, n_positions=4, n_yaw=n // 4, seed=seed)


@pytest.mark.parametrize("w,h", [(320, 240), (640, 480)])
def test_room_whole_frames(r, room, room_mesh, w, h):
    cams = _cams(room, w, h, seed=w)
    got, stats = r.render_mesh_depth_batch(cams, room_mesh, want_stats=True)
    got = got.cpu().numpy()
    for k, c in enumerate(cams):
        ref.check(got[k], ref.cast(room.vertices, room.triangles, ref.of_camera(c), near=0.2), f"room 50k {w}x{h} pose {k}")
        assert not np.isinf(got[k]).any()
        assert stats[k]["n_visible"] > 0 and stats[k]["d_total"] > 0 and stats[k]["n_pixels"] == w * h


def test_room_1080p_sampled(r, room, room_mesh):
    cams = _cams(room, 1920, 1080, seed=7)
    got = r.render_mesh_depth_batch(cams, room_mesh).cpu().numpy()
    for k, c in enumerate(cams):
        ys, xs = ref.sample_pixels(1920, 1080, 20000, seed=k)
        rr = ref.cast(room.vertices, room.triangles, ref.of_camera(c), near=0.2, pixels=(ys, xs))
        ref.check(got[k][ys, xs], rr, f"room 50k 1920x1080 pose {k} (sampled)")


def test_million_triangles_sampled(r):
    from sage_gs import scenes
    big = scenes.make_room_mesh(1_000_000, seed=3)
    assert len(big.triangles) > 900_000
    m = r.upload_mesh(big.vertices, big.triangles)
    for k, c in enumerate(_cams(big, 640, 480, n=4, seed=11)):
        got = r.render_mesh_depth(c, m).cpu().numpy()
        ys, xs = ref.sample_pixels(640, 480, 20000, seed=100 + k)
        ref.check(got[ys, xs], ref.cast(big.vertices, big.triangles, ref.of_camera(c), near=0.2, pixels=(ys, xs)), f"1M pose {k} (sampled)")
        assert not np.isinf(got).any()
    m.free()


def test_watertight_room_and_icosphere(r):
    """A closed subdivided room seen from 32 seeded interior poses has no pixel that sees out; a closed icosphere seen from outside
    covers exactly the reference's pixels outside the edge band."""
    from sage_gs import Camera, scenes
    V, T = scenes.grid_box((0.0, 0.0, 0.0), (6.0, 5.0, 2.8), (97, 83, 41))
    m = r.upload_mesh(V, T)
    rng = np.random.default_rng(1234)
    cams = []
    for k in range(32):
        pos = (rng.uniform(0.3, 5.7), rng.uniform(0.3, 4.7), rng.uniform(0.3, 2.5))
        fx, fy, cx, cy = scenes.reference_intrinsics(640, 480)
        cams.append(Camera(640, 480, fx, fy, cx, cy, scenes.view_from_yaw(pos, rng.uniform(0, 2 * math.pi), rng.uniform(-1.2, 1.2))))
    got = r.render_mesh_depth_batch(cams, m).cpu().numpy()
    assert int(np.isinf(got).sum()) == 0, [int(np.isinf(g).sum()) for g in got]
    for k in (0, 16):                      # the room is a grid_box: every pixel against the edge-exact bounds, seams included
        cc = ref.cast_continuous(V, T, ref.of_camera(cams[k]), near=0.2)
        ref.check_continuous(got[k], cc, f"closed room pose {k}")
        assert cc["need"].all()
    Vs, Ts = scenes.icosphere(6, (0.0, 0.0, 0.0), 1.0)
    assert 70_000 < len(Ts) < 90_000
    ms = r.upload_mesh(Vs, Ts)
    for k in range(4):
        fx, fy, cx, cy = scenes.reference_intrinsics(640, 480)
        yaw = 2 * math.pi * k / 4
        pos = (-3.0 * math.cos(yaw), -3.0 * math.sin(yaw), 0.4 * k - 0.6)
        c = Camera(640, 480, fx, fy, cx, cy, scenes.view_from_yaw(pos, yaw, -math.atan2(pos[2], 3.0)))
        d = r.render_mesh_depth(c, ms).cpu().numpy()
        rr = ref.cast(Vs, Ts, ref.of_camera(c), near=0.2)
        ref.check(d, rr, f"icosphere pose {k}")
        off = ~rr["edge"]
        assert (np.isfinite(d)[off] == np.isfinite(rr["nominal"])[off]).all()
        assert np.isfinite(d).sum() > 20000


def test_bit_exact_invariants(r, room, room_mesh):
    import torch
    cams = _cams(room, 640, 480, n=12, seed=5)
    batch = r.render_mesh_depth_batch(cams, room_mesh).cpu().numpy()          # two groups: 8 + 4
    for k, c in enumerate(cams):
        single = r.render_mesh_depth(c, room_mesh).cpu().numpy()
        assert np.array_equal(single, batch[k]), k
    again = r.render_mesh_depth_batch(cams, room_mesh).cpu().numpy()
    assert np.array_equal(again, batch)
    out = torch.full((480, 640), -3.0, device=r.device)
    r.render_mesh_depth(cams[2], room_mesh, tile_rows=(7, 19), out=out)
    band = out.cpu().numpy()
    assert np.array_equal(band[112:304], batch[2][112:304]) and (band[:112] == -3.0).all() and (band[304:] == -3.0).all()
    perm = np.random.default_rng(9).permutation(len(room.triangles))
    mp = r.upload_mesh(room.vertices, room.triangles[perm][:, [2, 0, 1]])
    assert np.array_equal(r.render_mesh_depth_batch(cams, mp).cpu().numpy(), batch)
    mp.free()


def test_small_record_buffer_regrows(r, room, room_mesh):
    from sage_gs import Renderer
    cams = _cams(room, 640, 480, n=4, seed=21)
    want = r.render_mesh_depth_batch(cams, room_mesh).cpu().numpy()
    r2 = Renderer("cuda:0")
    try:
        r2.set_mesh_record_capacity(1000)
        m2 = r2.upload_mesh(room.vertices, room.triangles)
        got, st = r2.render_mesh_depth_batch(cams, m2, want_stats=True)
        assert st[0]["retries"] > 0 and np.array_equal(got.cpu().numpy(), want)
        d1 = r2.render_mesh_depth(cams[1], m2, timing=True).cpu().numpy()
        assert np.array_equal(d1, want[1]) and r2.last_stats["ms_total"] > 0
        m2.free()
    finally:
        r2.close()


def _golden_pose():
    import json
    g = json.load(open(os.path.join(HERE, "golden", "pose_env_golden.json")))
    c = g["cases"][0]
    return c["start_camera_position"], c["start_orientation"]


def _write_collision(tmp_path):
    """A closed 8 x 6 x 2.8 m room with a box in it, as an ASCII collision layer in the payload's own frame ([-8,0] x [-6,0] x [0,2.8]
    in centimetres: the scene_collision prim's Rz(180) puts it at [0,8] x [0,6]); returns its path and (V, T) in metres, model frame."""
    from sage_gs import scenes
    V1, T1 = scenes.grid_box((-8.0, -6.0, 0.0), (0.0, 0.0, 2.8), (16, 12, 6))
    V2, T2 = scenes.grid_box((-3.0, -2.5, 0.0), (-2.2, -1.7, 1.0), (2, 2, 2))
    V = np.concatenate([V1, V2]); T = np.concatenate([T1, T2 + len(V1)])
    pts = ", ".join(f"({100 * a:.6f}, {100 * b:.6f}, {100 * c:.6f})" for a, b, c in V.astype(np.float32).astype(np.float64))
    text = ('#usda 1.0\n(\n    metersPerUnit = 0.01\n    upAxis = "Z"\n)\n\ndef Xform "Collision"\n{\n    def Mesh "room"\n    {\n'
            f'        int[] faceVertexCounts = [{", ".join(["3"] * len(T))}]\n'
            f'        int[] faceVertexIndices = [{", ".join(str(i) for i in T.reshape(-1))}]\n'
            f'        point3f[] points = [{pts}]\n    }}\n}}\n')
    p = tmp_path / "0042_collision.usda"
    p.write_text(text)
    return p


def test_gs_camera_and_isaac_shim_collision_depth(r, tmp_path):
    import json
    from sage_gs import adapter, isaac_shim, ply
    from sage_gs import mesh as mesh_io
    from test_next_rows import _serialise_prim
    coll = _write_collision(tmp_path)
    Vm, Tm = mesh_io.read_usda_mesh(str(coll))
    g = json.load(open(os.path.join(HERE, "golden", "usda_golden.json")))
    sc = dict(g["scene_collision"], arcs=[["prepend payload", "@./0042_collision.usda@"]])
    (tmp_path / "0042.usdz").write_bytes(b"")
    rng = np.random.default_rng(3)
    n = 64
    ply.save_ply(str(tmp_path / "0042.ply"), rng.normal(size=(n, 3)).astype(np.float32), np.full((n, 3), 0.05, np.float32),
                 np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)), np.full(n, 0.5, np.float32), rng.normal(size=(n, 1, 3)).astype(np.float32), 0)
    stage = tmp_path / "0042.usda"
    stage.write_text('#usda 1.0\n(\n    metersPerUnit = 1\n    upAxis = "Z"\n)\n\ndef Xform "World"\n{\n'
                     '    over "gauss" (\n        prepend references = @./0042.usdz[gauss.usda]@\n    )\n    {\n'
                     '        double3 xformOp:rotateXYZ = (-90, 0, 0)\n        double3 xformOp:scale = (1, 1, 1)\n'
                     '        double3 xformOp:translate = (0, 0, 0)\n'
                     '        uniform token[] xformOpOrder = ["xformOp:translate", "xformOp:rotateXYZ", "xformOp:scale"]\n    }\n'
                     + _serialise_prim(sc) + '}\n')
    parsed = adapter.parse_scene_usda(stage.read_text())
    m2w = adapter.collision_model_to_world(parsed)
    assert np.abs(m2w - np.diag([-1.0, -1.0, 1.0, 1.0])).max() < 1e-6
    pos, orient = _golden_pose()
    # GsCamera with a mesh uploaded by hand ...
    mesh = r.upload_mesh(Vm, Tm, m2w)
    scene = r.upload(ply.to_gaussians(ply.load_ply(str(tmp_path / "0042.ply")), r.device, adapter.asset_model_to_world(parsed)))
    cam = adapter.GsCamera(r, scene, resolution=(640, 480), collision_mesh=mesh)
    cam.set_world_pose(pos, orient)
    rr = ref.cast(Vm, Tm, ref.of_camera(cam._camera(), m2w), near=adapter.MESH_CONFIG.near)
    raw = cam.get_current_frame()["distance_to_image_plane"]
    ref.check(raw, rr, "GsCamera collision depth")
    d = cam.get_depth()
    lo, hi = np.clip(rr["lenient"], 0.1, 6.5), np.clip(rr["strict"], 0.1, 6.5)
    assert d.dtype == np.float32 and ((lo <= d) & (d <= hi)).all() and np.array_equal(d, np.clip(raw, 0.1, 6.5))
    assert not np.isinf(raw).any() and (d < 6.5).any()
    # ... and through the shim: open_stage with collision=True loads the payload and its cameras use it
    isaac_shim.configure(renderer=r, collision=True)
    try:
        assert isaac_shim.open_stage(str(stage))
        c2 = isaac_shim.Camera("/World/Cam", resolution=(640, 480))
        c2.set_world_pose(pos, orient)
        assert np.array_equal(c2.get_depth(), d)
        isaac_shim.get_context().close_stage()
        # a missing payload raises
        (tmp_path / "0042_collision.usda").unlink()
        with pytest.raises(FileNotFoundError):
            isaac_shim.open_stage(str(stage))
    finally:
        isaac_shim.configure(collision=False)
        isaac_shim._state["stage"] = None
        isaac_shim._state["renderer"] = None
    mesh.free(); scene.free()


@pytest.fixture(scope="module")
def gdrv(r):
    return mc.GpuMesh(r)


@pytest.mark.parametrize("name", list(mc.EDGE_CASES))
@pytest.mark.parametrize("w,h", [(640, 480), (1920, 1080)])
def test_edge_cases_alone_and_batched(gdrv, name, w, h):
    """tests/mesh_edge_cases.py's edge-aligned meshes: alone (every pixel at 640x480, 30k sampled at 1920x1080 — partial tiles), then in
    a batch of 12 (groups of 8 + 4) whose first and last frames use the case's own camera (bit for bit the single frame) and whose
    others are slightly moved (two of them checked on sampled pixels)."""
    if w == 640:
        case, single, n = mc.check_edge_case(gdrv, name, w, h, seed=w)
    else:
        case = mc.EDGE_CASES[name](w, h, w)
        single, _ = gdrv.frame(case["V"], case["T"], case["cam"])
        assert not np.isnan(single).any()
        ys, xs = ref.sample_pixels(w, h, 30000, seed=1)
        n = mc.check_frame(single[ys, xs], case, pixels=(ys, xs), what=case["name"] + " (sampled)")
    print(f"[edges] {case['name']}: {len(case['T'])} triangles, {n}")
    rng = np.random.default_rng(w)
    cams = [case["cam"]] + [mc.nudged(case["cam"], rng) for _ in range(10)] + [case["cam"]]
    got, st = gdrv.frames(case["V"], case["T"], cams)
    assert np.array_equal(got[0], single) and np.array_equal(got[11], single)
    for k in (3, 9):
        ys, xs = ref.sample_pixels(w, h, 20000, seed=k)
        mc.check_frame(got[k][ys, xs], case, cam=cams[k], pixels=(ys, xs), what=f"{case['name']} batch frame {k} (sampled)")


def test_room_far_plane(r, room, room_mesh):
    from sage_gs import RenderConfig
    cams = _cams(room, 640, 480, n=4, seed=31)
    got = r.render_mesh_depth_batch(cams, room_mesh, config=RenderConfig(far=3.0)).cpu().numpy()
    for k, c in enumerate(cams):
        ref.check(got[k], ref.cast(room.vertices, room.triangles, ref.of_camera(c), near=0.2, far=3.0), f"room 50k far 3 pose {k}")
        assert (got[k][np.isfinite(got[k])] <= 3.0).all()
    assert np.isinf(got).sum() > 10000 and np.isfinite(got).sum() > 10000


def test_near_far_exact_and_straddling(gdrv):
    mc.case_near_far_exact(gdrv)
    mc.case_far_straddle(gdrv)


def test_degenerate_and_culled_triangles(gdrv, room):
    c = _cams(room, 640, 480, n=4, seed=41)[1]
    mc.case_collinear_exact(gdrv)
    want = mc.case_degenerate(gdrv, (room.vertices, room.triangles), ref.of_camera(c))
    ys, xs = ref.sample_pixels(640, 480, 20000, seed=5)
    ref.check(want[ys, xs], ref.cast(room.vertices, room.triangles, ref.of_camera(c), near=0.2, far=20.0, pixels=(ys, xs)),
              "room 50k far 20 (sampled)")


def test_more_than_1024_tiles(gdrv):
    st = mc.case_many_tiles(gdrv)
    print(f"[tiles] 528x528: {st['n_tiles']} tiles, {st['d_total']} records, longest list {st['max_tile_len']}")
