"""The image similarity on the MI355X: similarity_cases' checks through the real library (every field of every row equal to the
restatement, on the build's own levels), the GPU's rows against the emulator's bit for bit, a batch of rendered room frames, a call
on a caller's stream, and the layers above the C ABI — Renderer.image_similarity, GsCamera.set_target_image / get_image_similarity."""
import numpy as np
import pytest

import emu_harness
import similarity_cases as sc
import similarity_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    from sage_gs import Renderer
    rr = Renderer("cuda:0")
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def drv(r):
    return sc.GpuSimilarity(r)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_pictures_on_the_gpu(drv, shape):
    """The levels are this build's own (hipcc may fuse x * 255 + 0.5: sgs_pack_rgba8 of the picture says what they are)."""
    sc.check_shape(drv, shape, levels_of=drv.pack)


def test_batches_strides_and_refusals_on_the_gpu(drv):
    sc.check_batches(drv, levels_of=drv.pack)
    sc.check_refusals(drv)


def test_gpu_rows_equal_the_emulators(drv):
    """Frames on the levels (k / 255: where fusing x * 255 + 0.5 changes nothing): bit for bit the emulator's rows, per picture and
    for the batch of nine with padded strides."""
    from sage_gs import _capi
    emu = sc.AbiSimilarity(_capi.Lib(emu_harness.build_emu()))
    try:
        for shape in sc.SHAPES:
            for name, (frame, target) in sc.pictures_of(shape).items():
                if name == "out_of_range":
                    continue
                assert drv.rows(frame[None], target[None]).tobytes() == emu.rows(frame[None], target[None]).tobytes(), (sc.shape_id(shape), name)
        frames, targets = sc.batch_pictures()
        frames = sc.unlevel(ref.levels(frames))
        size = frames[0].size
        assert drv.rows(frames, targets, rgb_stride=size + 37, target_stride=size + 5).tobytes() == \
            emu.rows(frames, targets, rgb_stride=size + 37, target_stride=size + 5).tobytes()
        assert drv.rows(frames, targets[2]).tobytes() == emu.rows(frames, targets[2]).tobytes()
    finally:
        emu.close()


@pytest.fixture(scope="module")
def room_frames(r):
    """16 frames of 1024 x 768 of a small room, on the device, and the levels of frame 0."""
    from sage_gs import scenes
    room = scenes.make_room(20_000)
    cams = scenes.room_cameras(room, 1024, 768, n_positions=4, n_yaw=4, seed=0)[:16]
    scene = r.upload(scenes.to_gaussians(room, "cuda:0"))
    frames = r.render_batch(cams, scene)
    target = r.pack_rgba8(frames[0])[..., :3].contiguous()
    yield frames, target
    scene.free()


def test_rendered_room_batch_against_frame_0(r, room_frames):
    """16 frames of 1024 x 768 (24 x 32 tiles each, the last column and row partial) against frame 0 in one call: the row of frame 0
    is the identical-picture answer; two other frames equal the restatement on the levels sgs_pack_rgba8 shows; every frame's row
    equals the row of the frame issued alone."""
    frames, target = room_frames
    res = r.image_similarity(frames, target)
    nw = (1024 - 10) * (768 - 10)
    assert res.shape == (16,) and (res["n_windows"] == nw).all() and (res["n_pixels"] == 1024 * 768).all()
    assert res["ssim_q"][0].tolist() == [nw * ref.ONE] * 3 and res["sse"][0].tolist() == [0, 0, 0]
    assert res["ssim"][0] == 1.0 and res["mse"][0] == 0.0 and np.isposinf(res["psnr"][0]) and res["ssim_rgb"][0].tolist() == [1.0] * 3
    assert len({x.tobytes() for x in res["ssim_q"]}) > 8, "the room's views do not differ"
    t = target.cpu().numpy()
    for k in (5, 15):
        want = ref.row(r.pack_rgba8(frames[k])[..., :3].cpu().numpy(), t)
        for name in ref.FIELDS:
            assert np.array_equal(res[name][k], want[name]), f"room frame {k}: {name} is {res[name][k].tolist()}, the restatement has {want[name].tolist()}"
        assert res["ssim"][k] == ref.score(want) < 1.0
        mse = float(int(want["sse"].sum())) / (3.0 * 1024 * 768)
        assert res["mse"][k] == mse > 0 and res["psnr"][k] == 10.0 * np.log10(255.0 * 255.0 / mse)
    for k in (1, 9):
        alone = r.image_similarity(frames[k], target)
        assert alone.shape == (1,) and alone[0].tobytes() == res[k].tobytes(), f"the row of frame {k} depends on the batch it is issued in"
    per_frame = r.image_similarity(frames[:3], torch_stack_levels(r, frames[:3]))
    assert (per_frame["ssim"] == 1.0).all() and (per_frame["sse"] == 0).all()


def torch_stack_levels(r, frames):
    import torch
    return torch.stack([r.pack_rgba8(f)[..., :3] for f in frames]).contiguous()


def test_call_on_a_callers_stream(r, drv, room_frames):
    """sgs_image_similarity on a stream that is not the default one: ordered behind that stream's work, the same rows."""
    import torch
    frames, target = room_frames
    want = r.image_similarity(frames[:4], target)
    s = torch.cuda.Stream(device=r.device)
    s.wait_stream(torch.cuda.current_stream(r.device))
    with torch.cuda.stream(s):
        moved = frames[:4].clone()                                                   # made on s: the call must run behind it
        got = r.image_similarity(moved, target)
    s.synchronize()
    assert got.tobytes() == want.tobytes()
    frame, tgt = sc.pictures_of(sc.SHAPES[5])["noise_pair"]
    rows = drv.rows(frame[None], tgt[None], stream=s.cuda_stream)
    sc.check_row("caller's stream", rows[0], ref.levels(frame), tgt)


def test_renderer_image_similarity_arguments(r):
    import torch
    from PIL import Image
    shape = sc.SHAPES[3]
    pics = sc.pictures_of(shape)
    frame, target = pics["smooth_plus_noise"]
    want = ref.row(ref.levels(frame), target)
    f = torch.from_numpy(frame).to(r.device)
    for tgt in (target, Image.fromarray(target), torch.from_numpy(target).to(r.device)):
        got = r.image_similarity(f, tgt)
        assert got.dtype == __import__("sage_gs")._capi.SIMILARITY_DTYPE and got.shape == (1,)
        for name in ref.FIELDS:
            assert np.array_equal(got[name][0], want[name]), name
        assert got["ssim"][0] == ref.score(want) and abs(got["ssim"][0] - ref.ssim_float(ref.levels(frame), target)) <= 6e-4
        assert np.allclose(got["ssim_rgb"][0].mean(), got["ssim"][0], rtol=0, atol=1e-15)
    both = r.image_similarity(torch.stack([f, f]), np.stack([target, pics["noise_pair"][1]]))
    assert both["ssim_q"][0].tolist() == want["ssim_q"].tolist() and both["ssim_q"][1].tolist() != want["ssim_q"].tolist()
    H, W = frame.shape[:2]
    bad = [(f, target[:-1]), (f, target[:, :-1]), (f, target.astype(np.float32)), (f, target[..., :2]), (f.double(), target), (f.cpu(), target),
           ((f * 255).to(torch.uint8), target), (torch.stack([f, f]), np.stack([target] * 3)), (f[:10, :10], target[:10, :10]),
           (f, Image.fromarray(target).resize((W // 2, H // 2)))]
    for fr, tg in bad:
        with pytest.raises(ValueError):
            r.image_similarity(fr, tg)


@pytest.fixture(scope="module")
def cameras(r):
    from sage_gs import camera as cam_conv, scenes
    from sage_gs.adapter import GsCamera
    pose = cam_conv.isaac_pose_from_view(np.eye(4))         # config 1 lies in front of an identity view
    scene = r.upload(scenes.to_gaussians(scenes.config1(), "cuda:0"))
    full = GsCamera(r, scene, resolution=(64, 48))
    small = GsCamera(r, scene, resolution=(64, 48), output_size=(32, 24))
    for c in (full, small):
        c.initialize()
        c.set_world_pose(*pose)
    yield full, small, pose
    scene.free()


def test_camera_image_similarity(r, cameras):
    """GsCamera: the view against its own get_rgba() scores exactly 1; a camera with output_size brings a full-size target to its
    output size once, with its own resample, and compares the picture get_rgba() shows; a moved camera scores what the restatement
    gives for the two pictures."""
    from PIL import Image
    full, small, pose = cameras
    with pytest.raises(RuntimeError):
        full.get_image_similarity()
    goal = full.get_rgba()
    assert len(np.unique(goal[..., :3])) > 20, "the view shows nothing"
    full.set_target_image(goal)                                                      # uint8 [h,w,4]: alpha dropped
    s = full.get_image_similarity()
    assert s["ssim"] == 1.0 and s["sse"].tolist() == [0, 0, 0] and s["n_windows"] == 54 * 38 and s["n_pixels"] == 64 * 48 and np.isposinf(s["psnr"])
    small.set_target_image(Image.fromarray(np.ascontiguousarray(goal[..., :3])))     # 64 x 48 for a 32 x 24 camera: resized here, once
    shown = small.get_rgba()[..., :3]
    assert tuple(small._target.shape) == (24, 32, 3) and np.array_equal(small._target.cpu().numpy(), shown)
    s = small.get_image_similarity()
    assert s["ssim"] == 1.0 and s["sse"].tolist() == [0, 0, 0] and s["n_windows"] == 22 * 14
    pos, orient = pose
    try:
        for c in (full, small):
            c.set_world_pose(np.asarray(pos, np.float32) + np.float32([0.05, 0.02, 0.0]), orient)
        for c, tgt in ((full, goal[..., :3]), (small, shown)):
            s = c.get_image_similarity()
            want = ref.row(c.get_rgba()[..., :3], tgt)
            assert ref.first_difference(s, want) is None and s["ssim"] == ref.score(want) < 1.0 and s["mse"] > 0 and np.isfinite(s["psnr"])
    finally:
        for c in (full, small):
            c.set_world_pose(*pose)
    with pytest.raises(ValueError):
        full.set_target_image(goal.astype(np.float32))
    full.set_target_image(None)
    with pytest.raises(RuntimeError):
        full.get_image_similarity()
