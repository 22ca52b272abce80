"""The top-down seen map on the MI355X (sgs_topdown_map, sgs_topdown_summary): topdown_cases' pictures, rendered frames, batches,
accumulation, the summary and the refusals through device pointers (misaligned ones among them), a call of 131073 frames that the
entry splits into three launches, a caller's stream, batches of 640 x 480 and 1024 x 768 mesh depth frames against the restatement,
and the layers above the C ABI — Renderer.pix_to_map / topdown_map / topdown_summary and GsCamera's exploration map.  Every
comparison of counts is exact."""
import numpy as np
import pytest

import topdown_cases as tc
import topdown_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    from sage_gs import Renderer
    rr = Renderer("cuda:0")
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def drv(r):
    return tc.GpuTopdown(r)


@pytest.fixture(scope="module")
def room(r):
    from sage_gs import scenes
    m = scenes.make_room_mesh(2000)
    mesh = r.upload_mesh(m.vertices, m.triangles)
    yield mesh
    mesh.free()


@pytest.mark.parametrize("make", tc.SMALL + tc.LARGE, ids=lambda m: m.__name__)
def test_pictures_on_the_gpu(drv, make):
    tc.check_pictures(drv, [make])


def test_hand_computed_case_on_the_gpu(drv):
    import test_topdown_ref
    depth, P, p = test_topdown_ref.hand_case()
    grid, counts = drv.map(depth, P, p)
    assert counts.tolist() == [[1, 1, 1, 5]]
    assert sorted(zip(*(v.tolist() for v in np.nonzero(grid)))) == [(0, 0, 0), (0, 1, 1), (0, 2, 0), (0, 2, 1), (2, 0, 0)] and grid.max() == 1


def test_rendered_room_frames_on_the_gpu(r, drv, room):
    tc.check_rendered(drv, lambda cams: r.render_mesh_depth_batch(cams, room).cpu().numpy())


def test_batches_accumulation_and_summary_on_the_gpu(drv):
    tc.check_batches(drv)
    tc.check_accumulation(drv)
    tc.check_summary(drv)


def test_refusals_on_the_gpu(drv):
    tc.check_refusals(drv)


def test_misaligned_buffers_are_refused_on_the_gpu(drv):
    """Refused by the host entry: the misaligned atomics never reach the device."""
    tc.check_misaligned(drv)


def test_split_launch_of_131073_frames(drv):
    """2 * 65535 + 3 one-pixel frames in one call, at the library's own SGS_TOPDOWN_MAX_FRAMES: two launches of gridDim.y = 65535 and one of 3."""
    assert tc.MAX_FRAMES == 65535 and tc.check_split(drv, tc.MAX_FRAMES) == 131073


@pytest.mark.parametrize("shape", [(640, 480, 16), (1024, 768, 8)], ids=lambda s: f"{s[2]}x{s[0]}x{s[1]}")
def test_batches_of_mesh_depth_frames_against_the_restatement(r, room, shape):
    """One call for the whole batch, the frames as render_mesh_depth_batch leaves them; the default grid moved over the room."""
    import torch
    from sage_gs import TopdownGrid
    W, H, n = shape
    cams = _turn(W, H, n)
    depth = r.render_mesh_depth_batch(cams, room)
    g = TopdownGrid(origin_x=-3.0, origin_y=-3.5)
    P = r.pix_to_map(cams)
    grid, counts = r.topdown_map(depth, P, g)
    assert grid.shape == (256, 256, 2) and counts.shape == (n, 4) and grid.dtype == counts.dtype == torch.int32 and grid.device == depth.device
    p = ref.Params(origin_x=-3.0, origin_y=-3.5)
    want, want_counts = ref.topdown(depth.cpu().numpy(), P.cpu().numpy(), p)
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want_counts), (counts.tolist(), want_counts.tolist())
    assert (want_counts.sum(1) == W * H).all() and (want_counts[:, 3] > W * H // 4).all()
    diff = np.nonzero(grid.cpu().numpy().view(np.uint32) != want)
    assert len(diff[0]) == 0, f"{len(diff[0])} cells differ from the restatement, first (i, j, channel) = {(int(diff[1][0]), int(diff[0][0]), int(diff[2][0]))}"
    assert int(want.max()) > 1000                                                    # cells that thousands of pixels fall into


def _turn(W, H, n, pitch=-0.6):
    from sage_gs import Camera, scenes
    fx, fy, cx, cy = scenes.reference_intrinsics(W, H)
    return [Camera(W, H, fx, fy, cx, cy, scenes.view_from_yaw((2.0 + 0.1 * k, 2.5, 1.2), 2 * np.pi * k / n, pitch)) for k in range(n)]


def test_caller_supplied_stream(r, room):
    """render_mesh_depth_batch, topdown_map and topdown_summary issued on a non-default stream with nothing between them."""
    import torch
    cams = _turn(160, 120, 5)
    grid0, counts0 = r.topdown_map(r.render_mesh_depth_batch(cams, room), cams)
    s0 = r.topdown_summary(grid0, cell_size=0.05)
    torch.cuda.synchronize(r.device)
    side = torch.cuda.Stream(r.device)
    assert side.cuda_stream != 0 and side.cuda_stream != torch.cuda.current_stream(r.device).cuda_stream
    with torch.cuda.stream(side):
        grid, counts = r.topdown_map(r.render_mesh_depth_batch(cams, room), cams)
        s = r.topdown_summary(grid, cell_size=0.05)
    side.synchronize()
    assert torch.equal(grid, grid0) and torch.equal(counts, counts0) and s == s0 and s["seen_cells"] > 500


def test_pix_to_map_against_an_fp64_unprojection(r):
    """Bit for bit the restatement's formula (fp64, rounded once); and the twelve numbers, evaluated in fp64 at a few pixels, land
    where an unprojection written out in fp64 lands, to within the rounding of the twelve numbers to fp32: each carries a relative
    error of at most 2^-24, so the point moves by at most 2^-24 (z (x |a_k| + y |b_k| + |c_k|) + |t_k|) per coordinate."""
    from sage_gs import Camera, scenes
    cams = [Camera(640, 480, 611.0, 608.5, 322.25, 239.5, scenes.view_from_yaw((2.0, 2.5, 1.2), 0.7, -0.4)),
            Camera(640, 480, 244.3, 244.3, 320.0, 240.0, scenes.view_from_yaw((-3.0, 1.5, 0.9), 4.1, 0.2))]
    y_up = np.array([[1.0, 0, 0, 0.5], [0, 0, -1.0, 2.0], [0, 1.0, 0, -0.25]])          # a map whose height is the world's y
    for m in (None, y_up):
        P = r.pix_to_map(cams, m).cpu().numpy()
        assert P.dtype == np.float32 and P.shape == (2, 12)
        for k, c in enumerate(cams):
            assert P[k].tobytes() == ref.pix_to_map(c.fx, c.fy, c.cx, c.cy, c.view, m).tobytes()
            c2w = np.linalg.inv(np.asarray(c.view, np.float64))
            for x, y, z in ((0, 0, 1.0), (639, 479, 6.5), (320, 240, 0.1), (17, 401, 2.75)):
                world = c2w @ np.array([z * (x + 0.5 - c.cx) / c.fx, z * (y + 0.5 - c.cy) / c.fy, z, 1.0])
                want = world[:3] if m is None else m[:, :3] @ world[:3] + m[:, 3]
                q = P[k].astype(np.float64)
                got = np.array([z * (x * q[3 * i] + y * q[3 * i + 1] + q[3 * i + 2]) + q[9 + i] for i in range(3)])
                bound = np.array([2.0 ** -24 * (z * (x * abs(q[3 * i]) + y * abs(q[3 * i + 1]) + abs(q[3 * i + 2])) + abs(q[9 + i])) for i in range(3)])
                assert (np.abs(got - want) <= bound + 1e-12).all(), (k, x, y, z, got, want, bound)
    one = r.pix_to_map(cams[0])
    assert one.shape == (1, 12) and np.array_equal(one.cpu().numpy()[0], r.pix_to_map(cams).cpu().numpy()[0])
    with pytest.raises(ValueError):
        r.pix_to_map(cams, np.eye(3))


def test_topdown_map_with_out_and_without_clear(r, room):
    import torch
    from sage_gs import TopdownGrid
    cams = _turn(160, 120, 5)
    depth = r.render_mesh_depth_batch(cams, room)
    g = TopdownGrid(nx=150, ny=130, origin_x=-0.75, origin_y=-0.75)
    p = ref.Params(nx=150, ny=130, origin_x=-0.75, origin_y=-0.75)
    P = r.pix_to_map(cams)
    want, want_counts = ref.topdown(depth.cpu().numpy(), P.cpu().numpy(), p)
    whole, counts = r.topdown_map(depth, cams, g)
    assert np.array_equal(whole.cpu().numpy().view(np.uint32), want) and np.array_equal(counts.cpu().numpy().view(np.uint32), want_counts)
    out = (torch.full((130, 150, 2), -3, dtype=torch.int32, device=r.device), torch.full((2, 4), -3, dtype=torch.int32, device=r.device))
    got = r.topdown_map(depth[:2], P[:2], g, out=out)                                 # CLEAR over what out held
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr() and torch.equal(out[1], counts[:2])
    rest = torch.empty((3, 4), dtype=torch.int32, device=r.device)
    r.topdown_map(depth[2:], cams[2:], g, out=(out[0], rest), clear=False)            # ... and the other three frames added to it
    assert torch.equal(out[0], whole) and torch.equal(rest, counts[2:])
    one = r.topdown_map(depth[3], cams[3], g)                                         # a single [H,W] frame
    assert torch.equal(one[1][0], counts[3]) and int(one[0].sum()) == int(counts[3, 3])
    s = r.topdown_summary(whole, cell_size=g.cell_size)
    occ, free, fh, oh = ref.summary(want)
    assert s == {"occupied_cells": occ, "free_cells": free, "free_hits": fh, "occupied_hits": oh, "seen_cells": occ + free, "seen_area_m2": (occ + free) * 0.05 ** 2}
    s3 = r.topdown_summary(whole, min_hits=3)
    assert [s3["occupied_cells"], s3["free_cells"], s3["free_hits"], s3["occupied_hits"]] == ref.summary(want, 3) and s3["seen_area_m2"] is None and s3["seen_cells"] < s["seen_cells"]
    for bad in (dict(depth=depth.double()), dict(depth=depth, P=P[:3]), dict(depth=depth, P=cams[:2]), dict(depth=depth, clear=False),
                dict(depth=depth, out=(out[0][:10], rest))):
        with pytest.raises(ValueError):
            r.topdown_map(bad["depth"], bad.get("P", P), g, out=bad.get("out"), clear=bad.get("clear", True))
    with pytest.raises(ValueError):
        r.topdown_summary(whole, min_hits=0)
    with pytest.raises(ValueError):
        r.topdown_summary(whole.float())


def test_gs_camera_exploration_over_a_turn(r, room):
    """Four poses of a turn: the map GsCamera accumulates pose by pose equals the map of the four frames in one batch, and the cells
    seen never decrease."""
    import torch
    from sage_gs import TopdownGrid, adapter, camera as cam_conv, scenes
    scene = r.upload(scenes.to_gaussians(scenes.config1(n=256), r.device))
    cam = adapter.GsCamera(r, scene, resolution=(160, 120), collision_mesh=room)
    g = TopdownGrid(nx=150, ny=130, origin_x=-0.75, origin_y=-0.75)
    with pytest.raises(RuntimeError, match="start_exploration_map"):
        cam.update_exploration_map()
    cam.start_exploration_map(g)
    assert cam.get_exploration()["seen_cells"] == 0
    views = [scenes.view_from_yaw((2.5, 2.5, 1.2), 0.3 + 1.5 * k, -0.6) for k in range(4)]
    seen, cams, frame_counts = [], [], []
    for v in views:
        cam.set_world_pose(*cam_conv.isaac_pose_from_view(v))
        frame_counts.append(cam.update_exploration_map().clone())
        cams.append(cam._camera())
        seen.append(cam.get_exploration())
    depth = r.render_mesh_depth_batch(cams, room, config=adapter.MESH_CONFIG)
    grid, counts = r.topdown_map(depth, cams, g)
    assert torch.equal(cam.get_exploration_grid(), grid) and torch.equal(torch.stack(frame_counts), counts)
    cells = [s["seen_cells"] for s in seen]
    assert all(a <= b for a, b in zip(cells, cells[1:])) and cells[0] > 100 and cells[-1] > cells[0], cells
    assert seen[-1] == r.topdown_summary(grid, cell_size=g.cell_size) and seen[-1]["seen_area_m2"] == cells[-1] * 0.05 ** 2
    assert cam.get_exploration(min_hits=4)["seen_cells"] < cells[-1]
    cam.start_exploration_map(g)                                                     # restarts empty
    assert cam.get_exploration()["seen_cells"] == 0
    with pytest.raises(RuntimeError, match="collision_mesh"):
        adapter.GsCamera(r, scene, resolution=(160, 120)).start_exploration_map()
    scene.free()
