"""The JPEG encoder on the MI355X: the checks of test_emu_jpeg.py (coefficients, structure, interoperability, fidelity, issue
independence) on rendered frames through the real library, the emulator's bytes against the GPU's, and the layers above the C ABI —
sweep.run(encoder="gpu"), GsCamera.get_jpeg(), the pipelined ring."""
import io
import json
import os

import numpy as np
import pytest

import emu_harness
import jpeg_cases as jc
import jpeg_ref

pytestmark = pytest.mark.gpu


class GpuJpeg(jc.GpuBuffers, jc.AbiJpeg):
    """jpeg_cases.AbiJpeg over torch device buffers, on a Renderer's context."""


@pytest.fixture(scope="module")
def r():
    from sage_gs import Renderer
    rr = Renderer("cuda:0")
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def rendered(r):
    """name -> fp32 [H,W,3] frames as render returned them: make_room (seed 1, 500 k) at 1024x768 and 640x480 at four poses of the
    sweep's kind each, one make_trained_like frame, one frame over a non-black background."""
    from sage_gs import RenderConfig, scenes
    out = {}
    sc = scenes.make_room(500_000, seed=1)
    scene = r.upload(scenes.to_gaussians(sc, "cuda:0"))
    for (w, h) in ((1024, 768), (640, 480)):
        cams = scenes.room_cameras(sc, w, h, n_positions=2, n_yaw=8, seed=2)
        for k in (0, 3, 9, 14):
            out[f"room_{w}x{h}_pose{k}"] = r.render(cams[k], scene).cpu().numpy()
    out["room_bg_640x480"] = r.render(scenes.room_cameras(sc, 640, 480, n_positions=1, n_yaw=4, seed=5)[1], scene,
                                      config=RenderConfig(background=(0.2, 0.5, 0.9))).cpu().numpy()
    scene.free()
    tl = scenes.make_trained_like(300_000, seed=1)
    scene = r.upload(scenes.to_gaussians(tl, "cuda:0"))
    out["trained_like_640x480"] = r.render(scenes.room_cameras(tl, 640, 480, n_positions=1, n_yaw=4, seed=3)[2], scene).cpu().numpy()
    scene.free()
    return out


def test_rendered_frames_against_reference_and_pil(r, rendered):
    """Test 9 (tests 1-3 and the fidelity figures of 4): the input is the fp32 frame render returned, the reference starts from
    pack_rgba8 of the same frame."""
    import torch
    d = GpuJpeg(r)
    for name, img in rendered.items():
        packed = r.pack_rgba8(torch.from_numpy(img).to(r.device)).cpu().numpy()[..., :3]
        assert np.abs(packed.astype(int) - jc.levels_of(img).astype(int)).max() <= 1
        # every quality and both subsamplings on the first pose of each size, on the trained-like frame and on the one over a background;
        # the other poses keep a subset (the Python parser takes about a second per 1024x768 file)
        full = name.endswith("pose0") or not name.startswith("room_1") and "pose" not in name
        grid = [(q, sub) for q in jc.QUALITIES for sub in jc.SUBSAMPLINGS] if full else [(95, "4:2:0"), (75, "4:4:4"), (100, "4:2:0"), (50, "4:4:4")]
        for q, sub in grid:
            data = d.encode_one(img, q, sub)
            jc.check_file(data, img, q, sub, label=name, u8=packed)
            assert r.encode_jpeg(torch.from_numpy(img).to(r.device), quality=q, subsampling=sub) == [data]


def test_synthetic_set_on_the_gpu(r):
    """The emulator tests' own pictures (partial MCUs, out-of-range input, the longest codes, exact ties) through the GPU build."""
    import torch
    d = GpuJpeg(r)
    for name, img in jc.image_set().items():
        packed = r.pack_rgba8(torch.from_numpy(img).to(r.device)).cpu().numpy()[..., :3]          # (levels on exact boundaries: the GPU's own)
        for q in jc.QUALITIES:
            for sub in jc.SUBSAMPLINGS:
                jc.check_file(d.encode_one(img, q, sub), img, q, sub, label=name, u8=packed)
    jc.check_exact_ties(d.encode_one)


def test_issue_independence_on_the_gpu(r, rendered):
    """Test 5: a batch of 5 different frames yields the bytes each yields alone; two calls yield the same bytes; so does a batch of 64."""
    import torch
    d = GpuJpeg(r)
    names = [n for n in rendered if "640x480" in n][:5]
    frames = np.stack([rendered[n] for n in names])
    assert len(names) == 5
    for q, sub in ((95, "4:2:0"), (75, "4:4:4")):
        batch = d.encode(frames, q, sub)
        assert batch["rc"] == 0 and len(set(batch["files"])) == 5
        jc.check_nothing_written_beyond(batch)
        assert d.encode(frames, q, sub)["files"] == batch["files"]
        for i in range(5):
            assert d.encode_one(frames[i], q, sub) == batch["files"][i], f"frame {i} depends on the batch it is issued in"
        assert d.encode(frames[[4, 0, 2]], q, sub)["files"] == [batch["files"][k] for k in (4, 0, 2)]
    many = torch.from_numpy(frames).to(r.device).repeat(13, 1, 1, 1)[:64]
    files = r.encode_jpeg(many)
    ref5 = d.encode(frames, 95, "4:2:0")["files"]
    assert files == [ref5[i % 5] for i in range(64)]


def test_capacity_on_the_gpu(r, rendered):
    d = GpuJpeg(r)
    frames = np.stack([rendered[n] for n in list(rendered) if "640x480" in n][:3])
    full = d.encode(frames, 95, "4:2:0")
    short = d.encode(frames, 95, "4:2:0", capacity=full["needed"] - 1)
    assert short["rc"] == -4 and (short["sizes"] == full["sizes"]).all()
    jc.check_nothing_written_beyond(short)
    cut = int(full["offsets"][2])
    assert bytes(short["buffer"][:cut]) == bytes(full["buffer"][:cut]) and (short["buffer"][cut:] == jc.SENTINEL).all()
    assert d.encode(frames, 95, "4:2:0", capacity=full["needed"])["files"] == full["files"]


def test_gpu_bytes_equal_the_emulators(r):
    """Test 10, from the LEVELS on: everything after the 8-bit level is written with explicit fmaf and single operations, so hipcc and
    the host compiler of the CPU test build produce the same coefficients and the same file.  Not from arbitrary fp32 input: the level
    itself is k_pack_rgba8's expression x * 255 + 0.5 (it has to be, to show the picture get_rgba() returns), which hipcc fuses into one
    rounding and the host compiler does not, so an input within an ulp of a level boundary can land on either side."""
    from sage_gs import _capi
    # input on the levels themselves (k / 255): how x * 255 + 0.5 is rounded on a level boundary is k_pack_rgba8's own property in each
    # build (one fused rounding under hipcc, two on the host), not the encoder's — everything after the levels is held to equality
    img = (jc.levels_of(jc.gradient_noise(192, 256, 5) * 1.1 - 0.05).astype(np.float32) / np.float32(255.0))
    emu = jc.AbiJpeg(_capi.Lib(emu_harness.build_emu()))
    d = GpuJpeg(r)
    try:
        for q, sub in ((95, "4:2:0"), (100, "4:4:4"), (50, "4:2:0")):
            assert d.encode_one(img, q, sub) == emu.encode_one(img, q, sub), f"q{q} {sub}: the GPU's file is not the emulator's"
    finally:
        emu.close()


def _pose_points(n):
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_golden.json")))
    return [c["points_after"][0] for c in g["cases"]][:n]


def test_sweep_with_the_gpu_encoder(r, tmp_path):
    """Test 11, on the set-up of test_sweep_driver_against_the_oracle: the same file set and metadata as encoder="pil"; every file
    opens in PIL at the right size, is a valid baseline file, and lies within the 3.0 levels (mean absolute difference) of the uint8
    frame handed to on_frame that the existing test allows PIL's q95 files."""
    from PIL import Image
    from sage_gs import scenes, sweep
    sc = scenes.make_room(30_000, seed=6)
    scene = r.upload(scenes.to_gaussians(sc, "cuda:0"))
    pts = [{"point_id": i, "position": p["position"], "rotation": p["rotation"]} for i, p in enumerate(_pose_points(5))]
    gt = {"groundtruth_data": [{"trajectory_id": "3", "instruction_index": 0, "sampled_points": pts},
                               {"trajectory_id": "3", "instruction_index": 1, "sampled_points": pts}]}
    ap = tmp_path / "action_groundtruth.json"; ap.write_text(json.dumps(gt))
    trs = sweep.load_trajectories(str(ap))
    seen = {}
    n_pil = sweep.run(r, scene, trs, "0007", str(tmp_path / "pil"), resolution=(256, 192))
    n_gpu = sweep.run(r, scene, trs, "0007", str(tmp_path / "gpu"), resolution=(256, 192), encoder="gpu", chunk=2,
                      on_frame=lambda tid, i, rgb: seen.__setitem__((tid, i), rgb.copy()))
    n_quiet = sweep.run(r, scene, trs, "0007", str(tmp_path / "gpu_quiet"), resolution=(256, 192), encoder="gpu")
    assert n_pil == n_gpu == n_quiet == 5 and sorted(seen) == [("3", i) for i in range(5)]
    tree = lambda d: sorted((dp[len(str(d)):], f) for dp, _, fs in os.walk(d) for f in fs)
    assert tree(tmp_path / "pil") == tree(tmp_path / "gpu") == tree(tmp_path / "gpu_quiet")
    assert json.load(open(tmp_path / "pil" / "image_metadata.json")) == json.load(open(tmp_path / "gpu" / "image_metadata.json"))
    for i in range(5):
        name = os.path.join("images", "trajectory_3", f"0007_3_{i:03d}.jpg")
        data = open(tmp_path / "gpu" / name, "rb").read()
        assert data == open(tmp_path / "gpu_quiet" / name, "rb").read(), "the file depends on the chunking / on on_frame"
        parsed = jpeg_ref.parse_jpeg(data)
        jc.check_structure(data, parsed, 256, 192, 95, "4:2:0")
        im = np.asarray(Image.open(io.BytesIO(data)))
        pil = np.asarray(Image.open(tmp_path / "pil" / name))
        mad = np.abs(im.astype(int) - seen[("3", i)].astype(int)).mean()
        mad_pil = np.abs(pil.astype(int) - seen[("3", i)].astype(int)).mean()
        print(f"[jpeg sweep] frame {i}: mean |file - frame| = {mad:.3f} levels (PIL's file {mad_pil:.3f}), {len(data)} bytes")
        assert im.shape == (192, 256, 3) and mad < 3.0
    scene.free()


def test_get_jpeg_of_the_camera_adapter(r):
    """Test 12: GsCamera.get_jpeg() decodes to within the same bound of get_rgba()'s frame at the same pose."""
    from PIL import Image
    from sage_gs import scenes
    from sage_gs.adapter import GsCamera
    from sage_gs import camera as cc
    sc = scenes.make_room(30_000, seed=6)
    scene = r.upload(scenes.to_gaussians(sc, "cuda:0"))
    cam = GsCamera(r, scene, resolution=(640, 480))
    cam.initialize()
    pos, orient = cc.datagen_pose(_pose_points(3)[2])
    cam.set_world_pose(pos, orient)
    rgba = cam.get_rgba()
    data = cam.get_jpeg()
    parsed = jpeg_ref.parse_jpeg(data)
    jc.check_structure(data, parsed, 640, 480, 75, "4:2:0")
    im = np.asarray(Image.open(io.BytesIO(data)))
    mad = np.abs(im.astype(int) - rgba[..., :3].astype(int)).mean()
    print(f"[jpeg camera] mean |get_jpeg - get_rgba| = {mad:.3f} levels at quality 75, {len(data)} bytes")
    assert im.shape == (480, 640, 3) and mad < 3.0
    assert len(cam.get_jpeg(quality=95)) > len(data)
    scene.free()


def test_pipelined_ring_gives_the_synchronous_bytes(r):
    """Test 13: chunks encoded asynchronously while the next chunk renders give the bytes of the synchronous call — also when a
    slot is too small and the ring has to grow it."""
    from sage_gs import scenes
    sc = scenes.make_room(100_000, seed=3)
    scene = r.upload(scenes.to_gaussians(sc, "cuda:0"))
    cams = scenes.room_cameras(sc, 320, 240, n_positions=2, n_yaw=12, seed=1)
    ring = r.jpeg_frames((8, 240, 320), quality=90, subsampling="4:4:4", depth=2)
    bufs, handles, want = [None, None], [], []
    chunks = [cams[0:8], cams[8:16], cams[16:21]]
    got = []
    for k, part in enumerate(chunks):
        if len(handles) == 2:
            got.append([bytes(f) for f in handles.pop(0).wait()])
        bufs[k % 2] = r.render_batch(part, scene, out=bufs[k % 2] if bufs[k % 2] is not None and bufs[k % 2].shape[0] >= len(part) else None)
        handles.append(ring.submit(bufs[k % 2], n=len(part)))
        want.append(r.encode_jpeg(bufs[k % 2][:len(part)].clone(), quality=90, subsampling="4:4:4"))
    while handles:
        got.append([bytes(f) for f in handles.pop(0).wait()])
    assert got == want and [len(g) for g in got] == [8, 8, 5]
    for f in got[2]:
        jpeg_ref.parse_jpeg(f)
    # a slot far too small: wait() grows it and encodes again
    small = r.jpeg_frames((2, 240, 320), quality=90, subsampling="4:4:4", depth=2)
    small._grow(0, 1000)
    assert [bytes(f) for f in small.submit(bufs[0][:2].clone()).wait()] == want[2][:2]          # (bufs[0] holds the third chunk)
    scene.free()


def test_padded_stride_and_long_scan_on_the_gpu(r):
    """test_emu_jpeg.py's test 9 through the GPU build, and its files against the emulator's (input on the levels)."""
    from sage_gs import _capi
    d = GpuJpeg(r)
    frames = np.stack([jc.levels_of(jc.gradient_noise(112, 128, seed=s) * (0.6 + 0.02 * s)).astype(np.float32) / np.float32(255.0) for s in range(20)])
    batch = jc.check_stride_and_long_scan(d.encode, frames, 256, 14, quality=75, subsampling="4:4:4")
    for i in (0, 9, 10, 19):
        assert d.encode_one(frames[i], 75, "4:4:4") == batch["files"][i], f"frame {i} depends on the batch it is issued in"
    jc.check_stride_and_long_scan(d.encode, frames[:3], 0, 4, quality=95, subsampling="4:2:0")
    emu = jc.AbiJpeg(_capi.Lib(emu_harness.build_emu()))
    try:
        assert emu.encode(frames, 75, "4:4:4")["files"] == batch["files"], "the GPU's files are not the emulator's"
    finally:
        emu.close()
