"""The clearance map on the MI355X (sgs_clearance_map, sgs_clearance_query): clearance_cases' pictures, batches, counters, seen maps
(one accumulated by sgs_topdown_map from rendered depth frames), queries, the reference's own recorded answers and the refusals
through device pointers; 8 maps of 512 x 512 and the column walk's worst case, one obstacle in the corner of 1024 x 1024, against
the two-pass restatement; a caller's stream; 10^5 segments in one call; and the layers above the C ABI — Renderer.clearance_map /
clearance_query, sage_gs.clearance.ClearanceMap and GsCamera.get_exploration_clearance.  Every comparison is exact.  Neither SciPy nor
the reference's tree is used here: the reference's answers come from tests/golden/clearance_golden.json."""
import numpy as np
import pytest

import clearance_cases as cc
import clearance_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    from sage_gs import Renderer
    rr = Renderer("cuda:0")
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def drv(r):
    return cc.GpuClearance(r)


@pytest.fixture(scope="module")
def room(r):
    from sage_gs import scenes
    m = scenes.make_room_mesh(2000)
    mesh = r.upload_mesh(m.vertices, m.triangles)
    yield mesh
    mesh.free()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("size", cc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_on_the_gpu(drv, size):
    cc.check_sizes(drv, [size])


def test_word_boundaries_and_shapes_on_the_gpu(drv):
    cc.check_pictures(drv, {**cc.lane_pictures(), **cc.shape_pictures()})


def test_batches_counters_and_seen_maps_on_the_gpu(drv):
    cc.check_batches(drv)
    cc.check_counters(drv)
    cc.check_seen_maps(drv)


def test_rendered_seen_map_on_the_gpu(r, drv, room):
    import topdown_cases as tc
    grid, _ = tc.check_rendered(tc.GpuTopdown(r), lambda cams: r.render_mesh_depth_batch(cams, room).cpu().numpy())
    cc.check_rendered_seen_map(drv, grid)


def test_queries_on_the_gpu(drv):
    cc.check_rounding(drv)
    cc.check_flags_margins_samples(drv)
    cc.check_non_finite(drv)


def test_the_references_own_answers_on_the_gpu(drv, tmp_path):
    cc.check_golden(drv, tmp_path)


def test_refusals_on_the_gpu(drv):
    cc.check_refusals(drv)


def test_misaligned_buffers_are_refused_on_the_gpu(drv):
    """Refused by the host entry: the misaligned accesses never reach the device."""
    cc.check_misaligned(drv)


def test_eight_maps_of_512x512(r):
    import torch
    rs = np.random.RandomState(11)
    maps = rs.rand(8, 512, 512) < 0.01
    d2, counts = r.clearance_map(torch.from_numpy(maps).to(r.device), max_d2=4)
    assert d2.shape == (8, 512, 512) and counts.shape == (8, 4) and d2.dtype == counts.dtype == torch.int32
    got, got_counts = _u32(d2), _u32(counts)
    for k in range(8):
        want = ref.d2_two_pass(maps[k])
        diff = np.nonzero(got[k] != want)
        assert len(diff[0]) == 0, f"map {k}: {len(diff[0])} cells differ from the restatement, first (i, j) = {(int(diff[1][0]), int(diff[0][0]))}"
        assert got_counts[k].tolist() == ref.counts(want, 4)


def test_one_obstacle_in_the_corner_of_1024x1024(r):
    """The column walk's worst case: every cell walks to the obstacle's row, about 10^9 rows in all."""
    import torch
    ob = np.zeros((1024, 1024), bool)
    ob[1023, 0] = True
    d2, counts = r.clearance_map(torch.from_numpy(ob).to(r.device), max_d2=1000 * 1000)
    want = ref.d2_two_pass(ob)
    assert want[0, 1023] == 2 * 1023 ** 2 and np.array_equal(_u32(d2), want)
    assert _u32(counts).tolist() == ref.counts(want, 1000 * 1000)


def _room_map(n=256, seed=0):
    rs = np.random.RandomState(seed)
    ob = np.zeros((n, n), bool)
    ob[0], ob[-1], ob[:, 0], ob[:, -1] = True, True, True, True
    ob[n // 3, : n // 2] = True
    ob[n // 3, n // 4: n // 4 + 12] = False
    ob[:, 2 * n // 3][n // 2:] = True
    for _ in range(12):
        j, i = rs.randint(4, n - 12, 2)
        ob[j:j + rs.randint(2, 8), i:i + rs.randint(2, 8)] = True
    return ob


def test_hundred_thousand_segments_and_a_callers_stream(r):
    import torch
    from sage_gs.clearance import ClearanceFrame
    ob = _room_map()
    rs = np.random.RandomState(12)
    segs = rs.uniform(-13.5, 0.5, (100000, 4))                                       # map coordinates span [0, 12.75]; negated, unflipped
    segs[::1000, 2] = np.nan
    frame = ClearanceFrame(0.0, 0.0, 12.75, 12.75, 0.05, flip_x=False, flip_y=False, max_d2=4)
    f = ref.Frame(0.0, 0.0, 12.75, 12.75, 0.05, flags=ref.NEGATE, margin=2, max_d2=4, n_samples=10)
    src = torch.from_numpy(ob).to(r.device)
    d2, counts = r.clearance_map(src, max_d2=4)
    out = r.clearance_query(d2, frame, segs)
    torch.cuda.synchronize(r.device)
    want_d2 = ref.d2_two_pass(ob)
    assert np.array_equal(_u32(d2), want_d2)
    want = ref.query_vectorised(want_d2, f, segs)
    assert out.dtype == torch.int64 and out.shape == (100000, 2) and np.array_equal(out.cpu().numpy(), want)
    assert set(np.unique(want[:, 0]).tolist()) == set(range(11)) and (want[::1000, 1] == ref.NONE).all()
    side = torch.cuda.Stream(r.device)
    assert side.cuda_stream != 0 and side.cuda_stream != torch.cuda.current_stream(r.device).cuda_stream
    dev_segs = torch.from_numpy(segs).to(r.device)
    torch.cuda.synchronize(r.device)
    with torch.cuda.stream(side):
        d2_s, counts_s = r.clearance_map(src, max_d2=4)
        out_s = r.clearance_query(d2_s, frame, dev_segs)
    side.synchronize()
    assert torch.equal(d2_s, d2) and torch.equal(counts_s, counts) and torch.equal(out_s, out)


def test_renderer_clearance_map_shapes_and_errors(r):
    import torch
    ob = _room_map(70, 3)
    one = r.clearance_map(torch.from_numpy(ob).to(r.device), max_d2=2)
    assert one[0].shape == (70, 70) and one[1].shape == (4,) and np.array_equal(_u32(one[0]), ref.d2_two_pass(ob))
    as_bytes = r.clearance_map(torch.from_numpy(ob.astype(np.uint8) * 7).to(r.device), max_d2=2)
    assert torch.equal(as_bytes[0], one[0]) and torch.equal(as_bytes[1], one[1])
    g = torch.from_numpy(cc.seen_maps().astype(np.int32)).to(r.device)
    seen, seen_counts = r.clearance_map(g, min_hits=3, unseen_blocks=True)
    assert seen.shape == (2, 11, 70) and seen_counts.shape == (2, 4)
    for k in range(2):
        assert np.array_equal(_u32(seen[k]), ref.d2_two_pass(ref.obstacles(cc.seen_maps()[k], None, 3, True)))
    assert torch.equal(r.clearance_map(g[1], min_hits=3, unseen_blocks=True)[0], seen[1])
    out = (torch.full((70, 70), -3, dtype=torch.int32, device=r.device), torch.full((4,), -3, dtype=torch.int32, device=r.device))
    got = r.clearance_map(torch.from_numpy(ob).to(r.device), max_d2=2, out=out)
    assert got[0].data_ptr() == out[0].data_ptr() and torch.equal(out[0], one[0]) and torch.equal(out[1], one[1])
    for bad in (dict(src=g.float()), dict(src=torch.from_numpy(ob).to(r.device), unseen_blocks=True), dict(src=g, min_hits=0), dict(src=g, kind="mask"),
                dict(src=torch.from_numpy(ob).to(r.device), out=(out[0][:5], out[1])), dict(src=torch.from_numpy(ob)), dict(src=g, kind="edges")):
        with pytest.raises(ValueError):
            r.clearance_map(bad.pop("src"), **bad)
    with pytest.raises(ValueError):
        r.clearance_query(one[0].float(), None, [[0, 0, 1, 1]])


def test_clearance_map_from_semantic_map_reproduces_the_reference(r, tmp_path):
    """ClearanceMap.from_semantic_map on the golden maps: the reference's obstacle_map at every radius and every recorded answer."""
    from sage_gs.clearance import ClearanceMap
    g = cc.golden()
    for e in g["maps"]:
        path = cc.write_golden_map(e, tmp_path)
        pos, segs = np.array(e["positions"]), np.array(e["segments"])
        for radius in g["radii"]:
            key = repr(radius)
            m = ClearanceMap.from_semantic_map(path, robot_radius_m=radius, scale=e["scale"], renderer=r)
            want = np.array([[c == "1" for c in row] for row in e["obstacle_map"][key]], np.uint8)
            assert m.obstacle_map.dtype == np.uint8 and np.array_equal(m.obstacle_map, want), (e["name"], radius)
            info = m.get_collision_info()
            assert info["obstacle_pixels"] == e["obstacle_pixels"][key] and info["map_size"] == e["size"] and info["total_pixels"] == want.size
            assert info["map_bounds"] == {"x": e["bounds"][:2], "y": e["bounds"][2:]} and info["robot_radius_m"] == radius and info["scale"] == e["scale"]
            assert "".join("1" if v else "0" for v in m.check_positions(pos)) == e["position_hits"][key], (e["name"], radius)
            by_ns = "".join("1" if m.check_paths(s[None, :3], s[None, 3:6], int(s[6]))[0] else "0" for s in segs[:6])
            assert by_ns == e["segment_hits"][key][:6]
            ten = segs[:, 6] == 10
            assert "".join("1" if v else "0" for v in m.check_paths(segs[ten][:, :3], segs[ten][:, 3:6])) == "".join(c for c, t in zip(e["segment_hits"][key], ten) if t)
        m = ClearanceMap.from_semantic_map(path, scale=e["scale"], renderer=r)           # the reference's default radius, its single-call forms
        for k in (0, 5, 61, 70, 80):
            want = e["position_hits"]["0.1"][k] == "1"
            assert m.check_collision_3d(pos[k]) is want and m.check_collision_at_position(pos[k][0], pos[k][1]) is want
        for k in (0, 1, 2, 30):
            assert m.check_path_collision_3d(segs[k][:3], segs[k][3:6], num_samples=int(segs[k][6])) is (e["segment_hits"]["0.1"][k] == "1")


def test_exploration_clearance_of_a_room(r, room):
    """A full turn of sixteen poses in the middle of the 6 x 5 m room: the middle of the room is free, a position inside a wall collides, and so does one
    far outside the map; with unseen_blocks the cells never seen block as well."""
    import torch
    from sage_gs import TopdownGrid, adapter, camera as cam_conv, scenes
    from sage_gs.clearance import ClearanceMap
    scene = r.upload(scenes.to_gaussians(scenes.config1(n=256), r.device))
    cam = adapter.GsCamera(r, scene, resolution=(160, 120), collision_mesh=room)
    with pytest.raises(RuntimeError, match="start_exploration_map"):
        cam.get_exploration_clearance()
    g = TopdownGrid(nx=150, ny=130, origin_x=-0.75, origin_y=-0.75)
    cam.start_exploration_map(g)
    for k in range(16):
        cam.set_world_pose(*cam_conv.isaac_pose_from_view(scenes.view_from_yaw((3.0, 2.5, 1.2), 0.2 + 0.4 * k, -0.3)))
        cam.update_exploration_map()
    m = cam.get_exploration_clearance(robot_radius_m=0.1)
    grid = cam.get_exploration_grid()
    want = ref.d2_two_pass(ref.obstacles(_u32(grid), None, 1, False))
    assert np.array_equal(_u32(m.d2), want) and m.frame.max_d2 == 4
    hits = m.check_positions([[3.0, 2.5], [3.0, 1.5], [3.0, 0.0], [6.0, 2.5], [3.0, 5.0], [40.0, 2.5]])      # the middle; three walls; far outside
    assert hits.tolist() == [False, False, True, True, True, True], hits.tolist()
    assert m.check_path_collision_3d([3.0, 2.5, 0.0], [3.0, 1.5, 0.0]) is False and m.check_path_collision_3d([3.0, 2.5, 0.0], [6.0, 2.5, 0.0]) is True
    same = ClearanceMap.from_topdown(g, grid, 0.1, renderer=r)
    assert torch.equal(same.d2, m.d2) and same.get_collision_info() == m.get_collision_info()
    blocked = cam.get_exploration_clearance(robot_radius_m=0.1, unseen_blocks=True)
    assert blocked.get_collision_info()["obstacle_pixels"] > m.get_collision_info()["obstacle_pixels"]
    assert np.array_equal(_u32(blocked.d2), ref.d2_two_pass(ref.obstacles(_u32(grid), None, 1, True)))
    scene.free()
