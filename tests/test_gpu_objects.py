"""The visible-object table on the MI355X (sgs_object_table): object_cases' pictures, rendered frames, batches and refusals through device
pointers (misaligned ones among them), a call of 131073 frames that the entry splits into three launches, a table large enough for the
clear's second trip, a caller's stream, a 16-frame 1024 x 768 batch against the restatement, and the layers above the C ABI — Renderer.object_table /
visible_objects, GsCamera.get_visible_objects and its frame dictionary, sweep.run(collision_mesh=).  Every comparison is exact."""
import json
import os

import numpy as np
import pytest

import mesh_id_cases as ic
import object_cases as oc
import object_table_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    from sage_gs import Renderer
    rr = Renderer("cuda:0")
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def drv(r):
    return oc.GpuObjects(r)


@pytest.fixture(scope="module")
def room(r):
    V, T, part, _ = ic.room(2000)
    m = r.upload_mesh(V, T, labels=part)
    yield m
    m.free()


@pytest.mark.parametrize("make", oc.SMALL + oc.PATHS + oc.LARGE, ids=lambda m: m.__name__)
def test_pictures_on_the_gpu(drv, make):
    oc.check_pictures(drv, [make])


def test_rendered_room_frames_on_the_gpu(r, drv):
    oc.check_rendered(drv, ic.GpuIds(r))


def test_batches_strides_and_refusals_on_the_gpu(drv):
    oc.check_batches(drv)
    oc.check_refusals(drv)


def test_misaligned_buffers_are_refused_on_the_gpu(drv):
    """Refused by the host entry: the misaligned 64- and 32-bit atomics never reach the device."""
    oc.check_misaligned(drv)


def test_split_launch_of_131073_frames(drv):
    """2 * 65535 + 3 one-pixel frames in one call, at the library's own SGS_OBJ_MAX_FRAMES: two launches of gridDim.y = 65535 and one of 3."""
    assert oc.check_split(drv, 65535) == 131073


def test_clear_makes_a_second_trip(r):
    """One 1 x 1 frame with n_labels = 65536 * 256 + 5: k_obj_clear runs its most workgroups (65536 of 256 threads) and five threads
    go round their loop a second time.  Every row but the last is the empty row, the last is the one pixel's; compared on the device."""
    import torch
    n_labels = 65536 * 256 + 5
    row_bytes = n_labels * 40
    free = torch.cuda.mem_get_info(r.device)[0]
    if free < 2 * row_bytes:
        pytest.skip(f"the table takes {row_bytes >> 20} MiB and the comparison as much again at most; the card has {free >> 20} MiB free")
    ids = torch.tensor([[n_labels - 1]], dtype=torch.int32, device=r.device)
    depth = torch.tensor([[2.5]], dtype=torch.float32, device=r.device)
    rows, counts = r.object_table(ids, depth, n_labels=n_labels)
    assert rows.shape == (1, n_labels, 10)
    inf_bits, z_bits = 0x7F800000, int(np.float32(2.5).view(np.uint32))
    empty = torch.tensor([0, oc.INT32_MAX, oc.INT32_MAX, 0, 0, inf_bits, 0, 0, 0, 0], dtype=torch.int32, device=r.device)
    assert ref.empty_rows(1).tobytes() == empty.cpu().numpy().tobytes()
    assert torch.equal(rows[0, :-1], empty.expand(n_labels - 1, 10)), "a row that no pixel shows is not the empty row"
    assert rows[0, -1].tolist() == [1, 0, 0, 1, 1, z_bits, 0, 0, 0, 0]
    assert counts.tolist() == [[0, 0]]
    want, want_counts = ref.table(ids.cpu().numpy(), depth.cpu().numpy(), n_labels)
    assert want[-1].tobytes() == rows[0, -1].cpu().numpy().tobytes() and want_counts.tolist() == [0, 0]
    del rows
    torch.cuda.empty_cache()


def test_caller_supplied_stream(r, room):
    """render_mesh_ids_batch and object_table issued on a non-default stream with nothing between them: the table of the default stream."""
    import torch
    cams = _cams(160, 120, 5)
    ids0, depth0 = r.render_mesh_ids_batch(cams, room, return_depth=True)
    rows0, counts0 = r.object_table(ids0, depth0, n_labels=12)
    torch.cuda.synchronize(r.device)
    side = torch.cuda.Stream(r.device)
    assert side.cuda_stream != 0 and side.cuda_stream != torch.cuda.current_stream(r.device).cuda_stream
    with torch.cuda.stream(side):
        ids, depth = r.render_mesh_ids_batch(cams, room, return_depth=True)
        rows, counts = r.object_table(ids, depth, n_labels=12)
    side.synchronize()
    assert torch.equal(ids, ids0) and torch.equal(depth.view(torch.int32), depth0.view(torch.int32))
    assert torch.equal(rows, rows0) and torch.equal(counts, counts0)
    assert int((rows0[:, :, 0] > 0).sum()) >= 15                                      # three labels or more in each of the five frames


def _cams(w, h, n=16):
    from sage_gs import scenes
    return scenes.room_cameras(ic.room(2000)[3], w, h, n_positions=4, n_yaw=4, seed=0)[:n]


def test_sixteen_frames_of_1024x768_against_the_restatement(r, room):
    """One call for the whole batch, the frames 1024 x 768 apart as render_mesh_ids_batch leaves them."""
    ids, depth = r.render_mesh_ids_batch(_cams(1024, 768), room, return_depth=True)
    rows, counts = r.object_table(ids, depth, n_labels=12)
    assert rows.shape == (16, 12, 10) and counts.shape == (16, 2) and rows.device == ids.device
    ids_h, depth_h = ids.cpu().numpy(), depth.cpu().numpy()
    rows_h = rows.cpu().numpy().view(ref.ROW_DTYPE).reshape(16, 12)
    counts_h = counts.cpu().numpy().view(np.uint32)
    assert len({f.tobytes() for f in ids_h}) == 16
    for f in range(16):
        oc.check_frame(f"1024x768 frame {f}", rows_h[f], counts_h[f], ids_h[f], depth_h[f], 12)


def test_renderer_object_table_and_visible_objects(r, room):
    import torch
    from sage_gs import _capi
    ids, depth = r.render_mesh_ids_batch(_cams(160, 120, 5), room, return_depth=True)
    ids_h, depth_h = ids.cpu().numpy(), depth.cpu().numpy()
    want = [ref.table(ids_h[f], depth_h[f], 12)[0] for f in range(5)]
    rows, counts = r.object_table(ids, depth, n_labels=12)
    assert rows.dtype == torch.int32 and np.array_equal(rows.cpu().numpy().view(ref.ROW_DTYPE).reshape(5, 12), np.stack(want))
    out = (torch.full((1, 12, 10), -3, dtype=torch.int32, device=r.device), torch.full((1, 2), -3, dtype=torch.int32, device=r.device))
    one = r.object_table(ids[2], depth[2], n_labels=12, out=out)                     # a single [H,W] frame, into given tensors
    assert one[0].data_ptr() == out[0].data_ptr() and torch.equal(out[0][0], rows[2]) and torch.equal(out[1][0], counts[2])
    no_depth = r.object_table(ids, n_labels=12)[0].cpu().numpy().view(ref.ROW_DTYPE).reshape(5, 12)
    assert np.isposinf(no_depth["z_min"]).all() and np.array_equal(no_depth["n_pixels"], np.stack(want)["n_pixels"])
    sizes = sorted(int(n) for n in np.stack(want)["n_pixels"].reshape(-1) if n > 0)
    cut = sizes[len(sizes) // 2]                                                    # a threshold that some visible labels miss
    for min_pixels in (1, cut):
        vis = r.visible_objects(ids, depth, n_labels=12, min_pixels=min_pixels)
        assert len(vis) == 5
        for f in range(5):
            keep = np.flatnonzero(want[f]["n_pixels"] >= min_pixels)
            assert vis[f].dtype == _capi.VISIBLE_OBJECT_DTYPE and vis[f]["label"].tolist() == keep.tolist(), (f, min_pixels)
            assert (np.diff(vis[f]["label"]) > 0).all()
            for name in ref.FIELDS:
                assert np.array_equal(vis[f][name].view(np.uint32 if name == "z_min" else vis[f][name].dtype),
                                      want[f][name][keep].view(np.uint32 if name == "z_min" else want[f][name].dtype)), (f, name)
    assert any(len(a) < len(b) for a, b in zip(r.visible_objects(ids, depth, n_labels=12, min_pixels=cut), r.visible_objects(ids, depth, n_labels=12)))
    n_out = [int((ids_h[f] >= 4).sum()) for f in range(5)]
    first = next(f for f in range(5) if n_out[f])
    with pytest.raises(ValueError, match=rf"frame {first}: {n_out[first]} pixels .* n_labels = 4"):
        r.visible_objects(ids, depth, n_labels=4)
    for bad in (dict(ids=ids.float()), dict(ids=ids, depth=depth[:2]), dict(ids=ids, depth=depth.double()), dict(ids=ids, n_labels=0)):
        with pytest.raises(ValueError):
            r.object_table(bad["ids"], bad.get("depth"), n_labels=bad.get("n_labels", 12))


def test_gs_camera_visible_objects_and_frame_dictionary(r, room):
    from sage_gs import adapter, camera as cam_conv, scenes
    scene = r.upload(scenes.to_gaussians(scenes.config1(n=256), r.device))
    paths = [f"/World/room/{name}" for name in scenes.ROOM_MESH_PARTS]
    cam = adapter.GsCamera(r, scene, resolution=(160, 120), collision_mesh=room, instance_paths=paths)
    cam.set_world_pose(*cam_conv.isaac_pose_from_view(scenes.view_from_yaw((2.0, 2.5, 1.2), 0.7, 0.1)))
    ids = cam.get_instance_ids()
    depth = cam.get_depth(clip=None)
    objs = cam.get_visible_objects()
    assert [o["label"] for o in objs] == sorted(set(ids[ids >= 0].tolist())) and len(objs) >= 3
    for o in objs:
        ys, xs = np.nonzero(ids == o["label"])
        assert o["path"] == paths[o["label"]] and o["pixels"] == len(xs)
        assert o["bbox"] == (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())), o
        assert o["centre"] == (int(xs.sum()) / len(xs), int(ys.sum()) / len(xs))
        assert np.float32(o["nearest_m"]) == depth[ys, xs].min(), o
    big = cam.get_visible_objects(min_pixels=objs[0]["pixels"] + 1)
    assert objs[0]["label"] not in [o["label"] for o in big] and all(o["pixels"] > objs[0]["pixels"] for o in big)
    assert "bounding_box_2d_tight" not in cam.get_current_frame()
    cam.add_instance_id_segmentation_to_frame()
    cam.add_bounding_box_2d_tight_to_frame()
    frame = cam.get_current_frame()
    box = frame["bounding_box_2d_tight"]
    assert box["data"].dtype == np.dtype([("semanticId", "<u4"), ("x_min", "<i4"), ("y_min", "<i4"), ("x_max", "<i4"), ("y_max", "<i4"), ("occlusionRatio", "<f4")])
    assert box["data"]["semanticId"].tolist() == [o["label"] + 1 for o in objs] and np.isnan(box["data"]["occlusionRatio"]).all()
    assert [tuple(int(v) for v in (b["x_min"], b["y_min"], b["x_max"], b["y_max"])) for b in box["data"]] == [o["bbox"] for o in objs]
    assert box["info"]["idToLabels"] == frame["instance_id_segmentation"]["info"]["idToLabels"]
    with pytest.raises(RuntimeError, match="collision_mesh"):
        adapter.GsCamera(r, scene, resolution=(160, 120)).get_visible_objects()
    with pytest.raises(RuntimeError, match="collision_mesh"):
        adapter.GsCamera(r, scene, resolution=(160, 120)).add_bounding_box_2d_tight_to_frame()
    unnamed = adapter.GsCamera(r, scene, resolution=(160, 120), collision_mesh=room)
    unnamed.set_world_pose(*cam.get_world_pose())
    assert [(o["label"], o["path"], o["bbox"]) for o in unnamed.get_visible_objects()] == [(o["label"], None, o["bbox"]) for o in objs]
    scene.free()


def _pose(x, y, yaw):
    from sage_gs import camera as cam_conv, scenes
    pos, q = cam_conv.isaac_pose_from_view(scenes.view_from_yaw((x, y, 1.2), yaw))
    return {"position": [float(v) for v in pos], "rotation": [float(v) for v in q]}


def test_sweep_lists_the_visible_objects(r, room, tmp_path):
    from sage_gs import scenes, sweep
    from sage_gs.adapter import MESH_CONFIG
    scene = r.upload(scenes.to_gaussians(scenes.config1(n=256), r.device))
    paths = [f"/World/room/{name}" for name in scenes.ROOM_MESH_PARTS]
    data = {"groundtruth_data": [
        {"trajectory_id": "7", "instruction_index": 0, "sampled_points": [dict(point_id=i, **_pose(2.0 + 0.3 * i, 2.5, 0.6 * i)) for i in range(3)]},
        {"trajectory_id": "9", "instruction_index": 1, "sampled_points": [dict(point_id=i, **_pose(3.0, 2.0 + 0.2 * i, 2.0 + 0.9 * i)) for i in range(2)]}]}
    actions = tmp_path / "action_groundtruth.json"
    actions.write_text(json.dumps(data))
    trajs = sweep.load_trajectories(str(actions))
    res = (160, 120)
    kw = dict(resolution=res, chunk=2, encode_workers=2)
    sweep.run(r, scene, trajs, "0042", str(tmp_path / "plain"), **kw)
    sweep.run(r, scene, trajs, "0042", str(tmp_path / "plain2"), collision_mesh=None, **kw)
    plain = (tmp_path / "plain" / "image_metadata.json").read_bytes()
    assert plain == (tmp_path / "plain2" / "image_metadata.json").read_bytes() and b"visible_objects" not in plain
    sweep.run(r, scene, trajs, "0042", str(tmp_path / "objs"), collision_mesh=room, instance_paths=paths, min_object_pixels=64, **kw)
    meta = json.load(open(tmp_path / "objs" / "image_metadata.json"))
    stripped = json.loads(json.dumps(meta))
    for s in stripped["sequences"]:
        del s["visible_objects"]
    assert stripped == json.loads(plain)                                            # everything else is what it is without a mesh

    def alone(tr):
        out = []
        for c in sweep.cameras_for(tr["points"], res):
            ids, depth = r.render_mesh_ids(c, room, config=MESH_CONFIG, return_depth=True)
            rows = r.visible_objects(ids, depth, n_labels=12, min_pixels=64)[0]
            out.append([{"label": int(v["label"]), "path": paths[int(v["label"])], "pixels": int(v["n_pixels"]),
                         "bbox": [int(v["x_min"]), int(v["y_min"]), int(v["x_end"]) - 1, int(v["y_end"]) - 1], "nearest_m": float(v["z_min"])} for v in rows])
        return out

    want = [alone(tr) for tr in trajs]
    assert [s["visible_objects"] for s in meta["sequences"]] == want
    assert sum(len(f) for f in want[0]) >= 6 and all(o["pixels"] >= 64 for f in want[0] + want[1] for o in f)
    # a resumed run skips the frames that exist and still lists their objects
    stamps = {p: os.path.getmtime(p) for p in (tmp_path / "objs" / "images").rglob("*.jpg")}
    assert len(stamps) == 5
    sweep.run(r, scene, trajs, "0042", str(tmp_path / "objs"), collision_mesh=room, instance_paths=paths, min_object_pixels=64, **kw)
    assert {p: os.path.getmtime(p) for p in stamps} == stamps
    assert [s["visible_objects"] for s in json.load(open(tmp_path / "objs" / "image_metadata.json"))["sequences"]] == want
    scene.free()
