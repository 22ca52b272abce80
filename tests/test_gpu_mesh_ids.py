"""Collision-mesh object ids on the MI355X (sgs_render_mesh_ids*): the cases of tests/mesh_id_cases.py through a sage_gs Renderer, the
Python refusals, and the Isaac-facing channel (GsCamera.get_instance_ids / get_current_frame / get_instance_id_png, isaac_shim)."""
import io
import os

import numpy as np
import pytest

import mesh_id_cases as ic

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
def drv(r):
    return ic.GpuIds(r)


@pytest.mark.parametrize("w,h", [(160, 120), (33, 17)])
@pytest.mark.parametrize("n", [2000, 20000])
def test_room_against_reference(drv, n, w, h):
    ic.case_reference(drv, n, w, h)


def test_known_answer(drv):
    ic.case_known_answer(drv)


def test_tie_rule(drv):
    ic.case_tie_rule(drv)


def test_nearest_wins(drv):
    ic.case_nearest_wins(drv)


def test_issue_independence():
    from sage_gs import Renderer
    r2 = Renderer("cuda:0")                       # (its own context: the case shrinks the mesh path's record buffer)
    try:
        ic.case_issue_independence(ic.GpuIds(r2))
    finally:
        r2.close()


def test_long_list(drv):
    ic.case_long_list(drv)


def test_defaults_and_refusals(drv):
    ic.case_defaults_and_refusals(drv)


def test_python_refusals(r):
    import torch
    V, T = ic.quad(2.0)
    m = r.upload_mesh(V, T, labels=np.array([4, 6], np.int32))
    cam = ic.GpuMesh.camera(ic.quad_cam())
    want = r.render_mesh_ids(cam, m).cpu().numpy()
    assert set(np.unique(want).tolist()) == {-1, 4, 6}
    for bad, msg in ((np.array([1, 2, 3], np.int32), "3 labels for a mesh of 2"), (np.array([1], np.int32), "1 labels"),
                     (np.array([1, 2], np.int64), "int32"), (np.array([1.0, 2.0], np.float32), "int32"),
                     (torch.tensor([1, 2], dtype=torch.int64), "int32"), (np.array([1, -2], np.int32), r"\[0, 2\^31 - 2\]")):
        with pytest.raises(ValueError, match=msg):
            r.set_mesh_labels(m, bad)
        assert np.array_equal(r.render_mesh_ids(cam, m).cpu().numpy(), want)       # the labels are as they were
    with pytest.raises(ValueError, match="labels"):
        r.upload_mesh(V, T, labels=np.array([1, 2, 3], np.int32))
    with pytest.raises(ValueError, match="out must be"):
        r.render_mesh_ids(cam, m, out=torch.zeros((48, 64), dtype=torch.float32, device=r.device))
    ids, depth, st = r.render_mesh_ids(cam, m, return_depth=True, stats=True)
    assert ids.dtype == torch.int32 and depth.dtype == torch.float32 and st["n_pixels"] == 64 * 48 and st["d_total"] > 0
    assert torch.equal(depth, r.render_mesh_depth(cam, m))
    bi, bd, bst = r.render_mesh_ids_batch([cam, cam], m, return_depth=True, want_stats=True)
    assert torch.equal(bi[0], ids) and torch.equal(bi[1], ids) and torch.equal(bd[1], depth) and len(bst) == 2
    m.free()


TWO_PRIMS = '''#usda 1.0
(
    metersPerUnit = 1
    upAxis = "Z"
)

def Xform "Collision"
{
    def Xform "wall"
    {
        def Mesh "mesh"
        {
            int[] faceVertexCounts = [4]
            int[] faceVertexIndices = [0, 1, 2, 3]
            point3f[] points = [(-4, 3, -3), (4, 3, -3), (4, 3, 3), (-4, 3, 3)]
        }
    }
    def Mesh "crate"
    {
        int[] faceVertexCounts = [4]
        int[] faceVertexIndices = [0, 1, 2, 3]
        point3f[] points = [(-0.8, 2, -0.8), (0.8, 2, -0.8), (0.8, 2, 0.8), (-0.8, 2, 0.8)]
    }
}
'''


def test_gs_camera_instance_ids(r, tmp_path):
    """GsCamera on a two-prim collision layer: ids, the frame dictionary (this project's own shape) and the 16-bit PNG of id + 1."""
    from PIL import Image
    from sage_gs import adapter, scenes
    from sage_gs import mesh as mesh_io
    p = tmp_path / "two_collision.usda"
    p.write_text(TWO_PRIMS)
    V, T, tri_prim, paths = mesh_io.read_usda_mesh(str(p), return_prims=True)
    assert paths == ["/Collision/wall/mesh", "/Collision/crate"] and tri_prim.tolist() == [0, 0, 1, 1]
    mesh = r.upload_mesh(V, T, labels=tri_prim)
    sc = scenes.config1(n=256)
    scene = r.upload(scenes.to_gaussians(sc, r.device))
    cam = adapter.GsCamera(r, scene, resolution=(160, 120), collision_mesh=mesh, instance_paths=paths)
    from sage_gs import camera as cam_conv
    # look along world +Y from the origin: the crate (1.6 m wide at 2 m) in front of the wall (8 m wide at 3 m)
    view = scenes.view_from_yaw((0.0, 0.0, 0.0), np.pi / 2)
    cam.set_world_pose(*cam_conv.isaac_pose_from_view(view))
    ids = cam.get_instance_ids()
    assert ids.dtype == np.int32 and ids.shape == (120, 160)
    assert set(np.unique(ids).tolist()) == {0, 1} and (ids == 1).sum() > 1000 and (ids == 0).sum() > 5000
    assert ids[60, 80] == 1 and ids[60, 5] == 0
    depth = cam.get_current_frame()["distance_to_image_plane"]
    assert (np.abs(depth[ids == 1] - 2.0) < 1e-4).all() and (np.abs(depth[ids == 0] - 3.0) < 1e-4).all()
    assert "instance_id_segmentation" not in cam.get_current_frame()
    cam.add_instance_id_segmentation_to_frame()
    seg = cam.get_current_frame()["instance_id_segmentation"]
    assert seg["data"].dtype == np.uint32 and np.array_equal(seg["data"], (ids + 1).astype(np.uint32))
    assert seg["info"]["idToLabels"] == {"0": "BACKGROUND", "1": "/Collision/wall/mesh", "2": "/Collision/crate"}
    png = cam.get_instance_id_png()
    im = Image.open(io.BytesIO(png))
    assert im.mode == "I;16" and im.size == (160, 120)
    assert np.array_equal(np.asarray(im).astype(np.int64), ids.astype(np.int64) + 1)
    # a camera turned away sees nothing: -1, 0 in the dictionary and in the PNG
    cam.set_world_pose(*cam_conv.isaac_pose_from_view(scenes.view_from_yaw((0.0, 0.0, 0.0), -np.pi / 2)))
    none = cam.get_instance_ids()
    assert (none == -1).all() and (cam.get_current_frame()["instance_id_segmentation"]["data"] == 0).all()
    assert (np.asarray(Image.open(io.BytesIO(cam.get_instance_id_png()))) == 0).all()
    # too many labels for 16 bits are refused; a camera without a mesh has no such channel
    many = adapter.GsCamera(r, scene, resolution=(160, 120), collision_mesh=mesh, instance_paths=[f"/p{k}" for k in range(65535)])
    with pytest.raises(ValueError, match="16-bit"):
        many.get_instance_id_png()
    with pytest.raises(RuntimeError, match="collision_mesh"):
        adapter.GsCamera(r, scene, resolution=(160, 120)).get_instance_ids()
    mesh.free(); scene.free()


def test_isaac_shim_hands_the_prim_paths_to_its_cameras(r, tmp_path):
    """configure(collision=True): the payload's triangles are labelled by their Mesh prim, named under /World/scene_collision."""
    import json
    from sage_gs import isaac_shim, ply
    from test_next_rows import _serialise_prim
    (tmp_path / "0042_collision.usda").write_text(TWO_PRIMS)
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
    from sage_gs import camera as cam_conv
    from sage_gs import scenes
    isaac_shim.configure(renderer=r, collision=True)
    try:
        assert isaac_shim.open_stage(str(stage))
        cam = isaac_shim.Camera("/World/Cam", resolution=(160, 120))
        # scene_collision turns the payload by Rz(180): the crate and the wall are along world -Y
        cam.set_world_pose(*cam_conv.isaac_pose_from_view(scenes.view_from_yaw((0.0, 0.0, 0.0), -np.pi / 2)))
        ids = cam.get_instance_ids()
        assert set(np.unique(ids).tolist()) == {0, 1} and ids[60, 80] == 1 and ids[60, 5] == 0
        cam.add_instance_id_segmentation_to_frame()
        seg = cam.get_current_frame()["instance_id_segmentation"]
        assert seg["info"]["idToLabels"] == {"0": "BACKGROUND", "1": "/World/scene_collision/wall/mesh", "2": "/World/scene_collision/crate"}
        assert np.array_equal(seg["data"], (ids + 1).astype(np.uint32))
        isaac_shim.get_context().close_stage()
    finally:
        isaac_shim.configure(collision=False)
        isaac_shim._state["stage"] = None
        isaac_shim._state["renderer"] = None
