"""The PNG encoder on the MI355X: the checks of test_emu_png.py (lossless, structure, filters, sizes, against zlib on the same strips,
issue independence, capacity) through the real library, the emulator's bytes against the GPU's, rendered colour and collision-mesh
depth as input, and the layers above the C ABI — Renderer.encode_png, GsCamera.get_png() / get_depth_png()."""
import io

import numpy as np
import pytest

import emu_harness
import jpeg_cases
import png_cases as pc
import png_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    from sage_gs import Renderer
    rr = Renderer("cuda:0")
    yield rr
    rr.close()


def _packed(r, img):
    """The frame's levels as this build packs them (hipcc may fuse x * 255 + 0.5 into one rounding: DESIGN.md §11)."""
    import torch
    packed = r.pack_rgba8(torch.from_numpy(np.ascontiguousarray(img, np.float32)).to(r.device)).cpu().numpy()[..., :3]
    assert np.abs(packed.astype(int) - png_ref.rgb_samples(img).astype(int)).max() <= 1
    return np.ascontiguousarray(packed)


def test_synthetic_set_on_the_gpu(r):
    """Checks 1-5 on the emulator tests' own pictures through the GPU build; the colour reference starts from pack_rgba8."""
    d = pc.GpuPng(r)
    for name, img in pc.colour_set().items():
        h, w = img.shape[:2]
        fig = pc.check_file(d.encode_one(img, "rgb8"), _packed(r, img), d.bound(w, h, "rgb8"), name)
        pc.check_smaller_than_raw(fig, name, noise=name.startswith("noise"))
        if name == "constant_640x48":
            assert fig["bytes"] <= 0.02 * fig["raw"], fig
    for name, img in pc.depth_set().items():
        h, w = img.shape
        fig = pc.check_file(d.encode_one(img, "depth16"), png_ref.depth_samples(img), d.bound(w, h, "depth16"), name)
        pc.check_smaller_than_raw(fig, name)


def test_issue_independence_on_the_gpu(r):
    """Test 6: a batch of 5 different frames yields the bytes each yields alone; two calls yield the same bytes; a permuted batch
    yields permuted files; so does a batch of 64 through Renderer.encode_png."""
    import torch
    d = pc.GpuPng(r)
    frames = np.stack([jpeg_cases.gradient_noise(187, 250, seed=s) * (0.5 + 0.1 * s) for s in range(5)])
    for fmt, fr in (("rgb8", frames), ("depth16", np.ascontiguousarray(frames[..., 0] * 7.0))):
        batch = d.encode(fr, fmt)
        assert batch["rc"] == 0 and len(set(batch["files"])) == 5
        jpeg_cases.check_nothing_written_beyond(batch)
        assert d.encode(fr, fmt)["files"] == batch["files"]
        for i in range(5):
            assert d.encode_one(fr[i], fmt) == batch["files"][i], f"frame {i} depends on the batch it is issued in"
        assert d.encode(fr[[4, 0, 2, 1, 3]], fmt)["files"] == [batch["files"][k] for k in (4, 0, 2, 1, 3)]
        many = torch.from_numpy(fr).to(r.device).repeat(13, *([1] * (fr.ndim - 1)))[:64]
        assert r.encode_png(many, format=fmt) == [batch["files"][i % 5] for i in range(64)]


def test_capacity_on_the_gpu(r):
    d = pc.GpuPng(r)
    frames = np.stack([jpeg_cases.gradient_noise(40, 56, seed=s) for s in range(3)])
    full = d.encode(frames, "rgb8")
    assert full["rc"] == 0
    short = d.encode(frames, "rgb8", capacity=full["needed"] - 1)
    assert short["rc"] == -4 and (short["sizes"] == full["sizes"]).all() and short["needed"] == full["needed"]
    jpeg_cases.check_nothing_written_beyond(short)
    cut = int(full["offsets"][2])
    assert bytes(short["buffer"][:cut]) == bytes(full["buffer"][:cut]) and (short["buffer"][cut:] == pc.SENTINEL).all()
    assert d.encode(frames, "rgb8", capacity=full["needed"])["files"] == full["files"]


def test_gpu_bytes_equal_the_emulators(r):
    """Test 8.  Depth from arbitrary fp32 input (the sample is one multiply and a truncation: nothing for a compiler to contract);
    colour from input on the levels, k / 255 (the level is k_pack_rgba8's x * 255 + 0.5, which hipcc fuses and the host compiler does
    not).  From the samples on the encoder is integer-only, so the files must be equal byte for byte."""
    from sage_gs import _capi
    emu = pc.AbiPng(_capi.Lib(emu_harness.build_emu()))
    d = pc.GpuPng(r)
    try:
        for name, img in pc.depth_set().items():
            assert d.encode_one(img, "depth16") == emu.encode_one(img, "depth16"), f"{name}: the GPU's file is not the emulator's"
        for name, img in pc.colour_set().items():
            on_levels = png_ref.rgb_samples(img).astype(np.float32) / np.float32(255.0)
            assert d.encode_one(on_levels, "rgb8") == emu.encode_one(on_levels, "rgb8"), f"{name}: the GPU's file is not the emulator's"
    finally:
        emu.close()


def test_rendered_colour(r):
    """Test 9, colour: make_room and make_trained_like at 320x240 through checks 1-5; Renderer.encode_png gives the ABI's bytes."""
    from sage_gs import scenes
    d = pc.GpuPng(r)
    for name, make in (("make_room", scenes.make_room), ("make_trained_like", scenes.make_trained_like)):
        sc = make(30_000, seed=6)
        scene = r.upload(scenes.to_gaussians(sc, "cuda:0"))
        cam = scenes.room_cameras(sc, 320, 240, n_positions=1, n_yaw=4, seed=2)[1]
        rgb = r.render(cam, scene)
        img = rgb.cpu().numpy()
        data = d.encode_one(img, "rgb8")
        fig = pc.check_file(data, _packed(r, img), d.bound(320, 240, "rgb8"), f"{name}_320x240")
        pc.check_smaller_than_raw(fig, name)
        assert r.encode_png(rgb) == [data] and r.encode_png(rgb[None]) == [data]
        scene.free()


def test_rendered_mesh_depth(r):
    """Test 9, depth: make_room_mesh at 320x240 and 640x480 from two room_cameras poses (oblique to the walls), one of them behind a
    far plane at the median depth of its own view so that it sees +inf pixels, through Renderer.render_mesh_depth ->
    encode_png(format="depth16") and checks 1-5."""
    from sage_gs import RenderConfig, scenes
    d = pc.GpuPng(r)
    room = scenes.make_room_mesh(50_000, seed=1)
    mesh = r.upload_mesh(room.vertices, room.triangles)
    for (w, h) in ((320, 240), (640, 480)):
        cams = scenes.room_cameras(room, w, h, n_positions=2, n_yaw=8, seed=5)
        for k, cut in ((1, False), (13, True)):
            depth = r.render_mesh_depth(cams[k], mesh)
            if cut:
                far = float(np.median(depth.cpu().numpy()))
                depth = r.render_mesh_depth(cams[k], mesh, config=RenderConfig(far=far))
            host = depth.cpu().numpy()
            if cut:
                assert np.isinf(host).sum() > 1000 and np.isfinite(host).sum() > 1000, "the far plane cuts nothing, or everything"
            files = r.encode_png(depth, format="depth16")
            fig = pc.check_file(files[0], png_ref.depth_samples(host), d.bound(w, h, "depth16"), f"mesh_depth_{w}x{h}_pose{k}")
            pc.check_smaller_than_raw(fig, "mesh depth")
            assert d.encode_one(host, "depth16") == files[0]
    mesh.free()


def test_camera_adapter(r):
    """Test 10: GsCamera(collision_mesh=...).get_depth_png() is exactly the picture the VLM client makes of get_depth();
    get_png() is exactly get_rgba()'s picture."""
    from PIL import Image
    from sage_gs import scenes
    from sage_gs.adapter import GsCamera
    sc = scenes.make_room(30_000, seed=6)
    scene = r.upload(scenes.to_gaussians(sc, "cuda:0"))
    room = scenes.make_room_mesh(20_000, seed=2)
    mesh = r.upload_mesh(room.vertices, room.triangles)
    cam = GsCamera(r, scene, resolution=(640, 480), collision_mesh=mesh)
    cam.initialize()
    cam.set_world_pose((3.0, 2.5, 1.2), (0.92388, 0.0, 0.0, 0.38268))
    im = Image.open(io.BytesIO(cam.get_depth_png())); im.load()
    want = (np.clip(cam.get_depth(), 0, 6.5) * 10000).astype(np.uint16)
    assert im.mode == "I;16" and np.array_equal(np.asarray(im), want)
    assert want.min() >= 1000 and len(np.unique(want)) > 100, "the pose sees nothing"
    near = Image.open(io.BytesIO(cam.get_depth_png(clip=(2.0, 4.0)))); near.load()
    assert np.array_equal(np.asarray(near), (np.clip(cam.get_depth(clip=(2.0, 4.0)), 0, 4.0) * 10000).astype(np.uint16))
    rgb = Image.open(io.BytesIO(cam.get_png())); rgb.load()
    assert rgb.mode == "RGB" and np.array_equal(np.asarray(rgb), cam.get_rgba()[..., :3])
    # without a mesh the depth is the Gaussians' expected depth, +inf where nothing is hit: the same contract
    cam2 = GsCamera(r, scene, resolution=(320, 240))
    cam2.set_world_pose((3.0, 2.5, 1.2), (0.92388, 0.0, 0.0, 0.38268))
    im2 = Image.open(io.BytesIO(cam2.get_depth_png())); im2.load()
    assert np.array_equal(np.asarray(im2), (np.clip(cam2.get_depth(), 0, 6.5) * 10000).astype(np.uint16))
    mesh.free(); scene.free()


def test_coder_pictures_on_the_gpu(r):
    """test_emu_png_coder.py's pictures (code lengths over 15 and 7 bits, few symbols, the run parse at every window edge, the stored /
    dynamic decision and its neighbours): the property from the reference alone, checks 1-5 with the coder's own, and the emulator's
    bytes.  The colour input is on the levels, so the reference's samples are the build's."""
    from sage_gs import _capi
    emu = pc.AbiPng(_capi.Lib(emu_harness.build_emu()))
    d = pc.GpuPng(r)
    try:
        for name, case in pc.coder_set().items():
            want = pc.check_coder_case(name, case)          # before the library's output is looked at
            frame, fmt = case["frame"], case["fmt"]
            h, w = frame.shape[:2]
            data = d.encode_one(frame, fmt)
            samples = _packed(r, frame) if fmt == "rgb8" else png_ref.depth_samples(frame)
            assert np.array_equal(samples, pc.samples_of(frame, fmt))
            fig = pc.check_file(data, samples, d.bound(w, h, fmt), name)
            want.pop("runs", None)
            print(f"[png coder] {name}: reference {want}; file {fig['coding']}")
            assert data == emu.encode_one(frame, fmt), f"{name}: the GPU's file is not the emulator's"
    finally:
        emu.close()


def test_padded_stride_and_long_scan_on_the_gpu(r):
    """test_emu_png_coder.py's test 15 through the GPU build, and its files against the emulator's (input on the levels)."""
    from sage_gs import _capi
    d = pc.GpuPng(r)
    frames = png_ref.rgb_samples(pc.long_scan_frames()).astype(np.float32) / np.float32(255.0)
    batch = jpeg_cases.check_stride_and_long_scan(d.encode, frames, 256, 2, fmt="rgb8")
    for i in (0, 1, 63, 64, 127, 128):
        assert d.encode_one(frames[i], "rgb8") == batch["files"][i], f"frame {i} depends on the batch it is issued in"
    depth = np.stack([pc.depth_levels(9, 5) * np.float32(1 + 0.01 * i) for i in range(257)])
    dbatch = jpeg_cases.check_stride_and_long_scan(d.encode, depth, 256, 1, fmt="depth16")
    emu = pc.AbiPng(_capi.Lib(emu_harness.build_emu()))
    try:
        assert emu.encode(frames, "rgb8")["files"] == batch["files"] and emu.encode(depth, "depth16")["files"] == dbatch["files"]
    finally:
        emu.close()
