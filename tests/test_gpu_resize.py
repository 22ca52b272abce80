"""The frame resize on the MI355X: resize_cases' checks through the real library (bicubic bit-equal to the restatement and so to
PIL.Image.resize, linear RGB8 bit-equal, linear F32 within its bound, pack / PNG of the resized frame, strides, refusals), the GPU's
values against the emulator's, and the layers above the C ABI — Renderer.resize, GsCamera(output_size=...)."""
import numpy as np
import pytest

import emu_harness
import png_cases
import resize_cases as rc
import resize_ref as ref

pytestmark = pytest.mark.gpu
POSE = None


@pytest.fixture(scope="module")
def r():
    from sage_gs import Renderer
    rr = Renderer("cuda:0")
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def drv(r):
    return rc.GpuResize(r)


@pytest.mark.parametrize("shape", rc.SHAPES, ids=rc.shape_id)
def test_shape_pairs_on_the_gpu(drv, shape):
    """The levels are this build's own (hipcc may fuse x * 255 + 0.5: sgs_pack_rgba8 of the picture says what they are)."""
    rc.check_shape(drv, shape, levels_of=drv.pack)


def test_resized_frames_pack_and_encode_on_the_gpu(r, drv):
    for shape in (rc.SHAPES[0], rc.SHAPES[2], rc.SHAPES[6]):
        rc.check_downstream(drv, png_cases.GpuPng(r), shape, levels_of=drv.pack)


def test_batches_strides_and_refusals_on_the_gpu(drv):
    rc.check_batch_and_strides(drv)
    rc.check_refusals(drv)


def test_gpu_values_equal_the_emulators(drv):
    """Input on the levels (k / 255: where fusing x * 255 + 0.5 changes nothing) and depth: bit for bit the emulator's frames."""
    from sage_gs import _capi
    emu = rc.AbiResize(_capi.Lib(emu_harness.build_emu()))
    try:
        for shape in rc.SHAPES[:6]:
            W, H, w, h = shape
            pic = rc.pictures_of(shape)["checker"]
            dep, clip = rc.depth_pictures(W, H)["inf_holes"]
            for filt in ("bicubic", "linear"):
                assert np.array_equal(drv.one(pic, (w, h), "rgb8", filt), emu.one(pic, (w, h), "rgb8", filt)), (rc.shape_id(shape), filt)
            assert np.array_equal(drv.one(dep, (w, h), "f32", "bicubic", clip), emu.one(dep, (w, h), "f32", "bicubic", clip)), rc.shape_id(shape)
    finally:
        emu.close()


def test_renderer_resize(r):
    """Renderer.resize: single frames and batches of both kinds equal the restatement; `out`; argument checks."""
    import torch
    W, H, w, h = rc.SHAPES[0]
    pics = rc.pictures_of(rc.SHAPES[0])
    frames = torch.from_numpy(np.stack([pics["random"], pics["checker"]])).to(r.device)
    want = np.stack([ref.resize_rgb8(pics[k], w, h)[0] for k in ("random", "checker")])
    got = r.resize(frames, (w, h))
    assert got.shape == (2, h, w, 3) and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(r.resize(frames[1], (w, h)).cpu().numpy(), want[1])
    out = torch.full((h, w, 3), -1.0, device=r.device)
    assert r.resize(frames[0], (w, h), out=out).data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want[0])
    lin = r.resize(frames[0], (w, h), filter="linear").cpu().numpy()
    assert np.array_equal(lin, ref.resize_rgb8(pics["random"], w, h, "linear")[0])
    d, clip = rc.depth_pictures(W, H)["inf_holes"]
    dt = torch.from_numpy(d).to(r.device)
    assert np.array_equal(r.resize(dt, (w, h), kind="depth", clip=clip).cpu().numpy(), ref.bicubic_f32(d, w, h, clip))
    assert np.array_equal(r.resize(dt[None].repeat(3, 1, 1), (w, h), kind="depth", clip=clip)[2].cpu().numpy(), ref.bicubic_f32(d, w, h, clip))
    assert r.encode_png(r.resize(frames, (w, h))) == r.encode_png(torch.from_numpy(want).to(r.device))
    for bad in (dict(kind="rgba"), dict(filter="lanczos"), dict(clip=(0.1, 6.5)), dict(out=torch.empty((h, w, 4), device=r.device))):
        with pytest.raises(ValueError):
            r.resize(frames[0], (w, h), **bad)
    with pytest.raises(ValueError):
        r.resize(frames[0].double(), (w, h))
    with pytest.raises(ValueError):
        r.resize(dt, (w, h))                               # a depth frame as colour
    from sage_gs import _capi
    with pytest.raises(_capi.SgsError):
        r.resize(frames[0], (0, h))


@pytest.fixture(scope="module")
def cameras(r):
    from sage_gs import camera as cam_conv, scenes
    global POSE
    POSE = cam_conv.isaac_pose_from_view(np.eye(4))        # config 1 lies in front of an identity view
    from sage_gs.adapter import GsCamera
    scene = r.upload(scenes.to_gaussians(scenes.config1(), "cuda:0"))
    full = GsCamera(r, scene, resolution=(64, 48))
    small = GsCamera(r, scene, resolution=(64, 48), output_size=(32, 24))
    plain = GsCamera(r, scene, resolution=(64, 48), output_size=None)
    for c in (full, small, plain):
        c.initialize()
        c.set_world_pose(*POSE)
    yield full, small, plain
    scene.free()


def test_camera_output_size_is_pillows_resize_of_the_full_frame(r, cameras):
    """GsCamera(resolution=(64, 48), output_size=(32, 24)): get_rgba() is PIL's resize of the full-resolution get_rgba(), get_depth()
    PIL's resize of the full-resolution get_depth(), bit for bit; the other getters show the same picture."""
    import io
    from PIL import Image
    full, small, _ = cameras
    rgba = full.get_rgba()
    assert rgba.shape == (48, 64, 4) and len(np.unique(rgba[..., :3])) > 20, "the view shows nothing"
    want = np.asarray(Image.fromarray(np.ascontiguousarray(rgba[..., :3])).resize((32, 24)))
    got = small.get_rgba()
    assert got.shape == (24, 32, 4) and (got[..., 3] == 255).all() and np.array_equal(got[..., :3], want)
    assert small.get_output_size() == (32, 24) and small.get_resolution() == (64, 48) and full.get_output_size() == (64, 48)
    depth = full.get_depth()
    assert depth.shape == (48, 64) and depth.dtype == np.float32 and depth.min() >= np.float32(0.1) and depth.max() <= 6.5
    want_d = np.asarray(Image.fromarray(depth).resize((32, 24)))
    got_d = small.get_depth()
    assert got_d.shape == (24, 32) and got_d.dtype == np.float32 and np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    assert np.array_equal(small.get_rgba(copy=False)[..., :3], want)
    im = Image.open(io.BytesIO(small.get_png())); im.load()
    assert im.size == (32, 24) and np.array_equal(np.asarray(im), want)
    assert np.array_equal(r.pack_rgba8(small.get_rgb_tensor()).cpu().numpy()[..., :3], want)
    jp = Image.open(io.BytesIO(small.get_jpeg())); jp.load()
    assert jp.size == (32, 24)
    dp = Image.open(io.BytesIO(small.get_depth_png())); dp.load()
    assert dp.size == (32, 24) and np.array_equal(np.asarray(dp), (np.clip(got_d, 0, 6.5) * 10000).astype(np.uint16))
    frame = small.get_current_frame()
    assert np.array_equal(frame["rgba"][..., :3], want) and frame["distance_to_image_plane"].shape == (24, 32)
    lin = type(small)(r, small._scene, resolution=(64, 48), output_size=(32, 24), resample="linear")
    lin.set_world_pose(*POSE)
    assert np.array_equal(lin.get_rgba()[..., :3], ref.linear_u8(rgba[..., :3], 32, 24))


def test_camera_without_output_size_is_unchanged(r, cameras):
    """output_size=None: get_rgba and get_depth are bit for bit those of a camera made without the argument."""
    full, _, plain = cameras
    assert np.array_equal(plain.get_rgba(), full.get_rgba()) and np.array_equal(plain.get_depth().view(np.uint32), full.get_depth().view(np.uint32))
    assert np.array_equal(plain.get_rgba()[..., :3], r.pack_rgba8(r.render(full._camera(), full._scene)).cpu().numpy()[..., :3])
    assert plain.get_output_size() == plain.get_resolution() == (64, 48)
