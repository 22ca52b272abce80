"""sweep.run(encoder="gpu") without a GPU: a stand-in renderer whose JPEG ring runs the library's own kernels under the wave64 emulator.
The worker threads only write bytes; the RGBA ring is asked for only when a callback wants the uint8 frames; the files are the ones the
encoder makes of the frames, whatever the chunking."""
import io
import os

import numpy as np
import pytest

import emu_harness
import jpeg_cases as jc
import jpeg_ref
from sage_gs import _capi, sweep


@pytest.fixture(scope="module")
def drv():
    d = jc.AbiJpeg(_capi.Lib(emu_harness.build_emu()))
    yield d
    d.close()


def _fake(drv, allow_rgba):
    import torch

    class Handle:
        def __init__(self, files):
            self.files = files

        def wait(self):
            return self.files

    class JpegRing:
        depth = 3

        def __init__(self, quality):
            self.quality, self.live = quality, []

        def submit(self, frames, n):
            files = drv.encode(frames[:n].numpy(), self.quality, "4:2:0")["files"]
            return Handle([memoryview(f) for f in files])

    class RgbaRing:
        def __init__(self, shape):
            self.shape = shape

        def submit(self, buf, n):
            host = np.zeros(self.shape, np.uint8)
            host[:n, :, :, :3] = jc.levels_of(buf[:n].numpy())
            return Handle(host)

    class Fake:
        batches, rgba_rings = [], 0

        def host_frames(self, shape, depth=2):
            assert allow_rgba, "the RGBA copy is made only when on_frame is given"
            Fake.rgba_rings += 1
            return RgbaRing(shape)

        def jpeg_frames(self, shape, quality=95, subsampling="4:2:0", depth=3):
            assert depth == JpegRing.depth and subsampling == "4:2:0"
            return JpegRing(quality)

        def render_batch(self, cams, scene, out=None):
            self.batches.append(len(cams))
            f = torch.zeros((len(cams), cams[0].height, cams[0].width, 3))
            for k, c in enumerate(cams):
                x = float(np.linalg.inv(np.asarray(c.view, np.float64).reshape(4, 4))[0, 3])
                f[k] = torch.from_numpy(jc.gradient_noise(cams[0].height, cams[0].width, seed=int(x)))
            return f

    return Fake()


def _traj(tid, n, x0):
    return {"trajectory_id": tid, "instruction_index": 0,
            "points": [{"point": i, "position": [x0 + i, 0.0, 1.2], "rotation": [0.0, 0.0, 0.0, 1.0]} for i in range(n)]}


def test_sweep_writes_the_encoders_files(drv, tmp_path):
    from PIL import Image
    trs = [_traj("a", 5, 10), _traj("b", 6, 30)]
    fake = _fake(drv, allow_rgba=False)
    n = sweep.run(fake, None, trs, "0042", str(tmp_path / "g"), resolution=(40, 24), chunk=4, quality=80, encoder="gpu", encode_workers=2)
    assert n == 11 and fake.batches == [4, 4, 3]
    seen = {}
    fake2 = _fake(drv, allow_rgba=True)
    sweep.run(fake2, None, trs, "0042", str(tmp_path / "h"), resolution=(40, 24), chunk=8, quality=80, encoder="gpu",
              on_frame=lambda tid, i, rgb: seen.__setitem__((tid, i), rgb.copy()))
    assert type(fake2).rgba_rings == 1 and len(seen) == 11
    for t, cnt, x0 in (("a", 5, 10), ("b", 6, 30)):
        names = [f"0042_{t}_{i:03d}.jpg" for i in range(cnt)]
        assert sorted(os.listdir(tmp_path / "g" / "images" / f"trajectory_{t}")) == names
        for i, name in enumerate(names):
            data = open(tmp_path / "g" / "images" / f"trajectory_{t}" / name, "rb").read()
            assert data == open(tmp_path / "h" / "images" / f"trajectory_{t}" / name, "rb").read()
            frame = jc.gradient_noise(24, 40, seed=x0 + i)
            assert data == drv.encode_one(frame, 80, "4:2:0")
            parsed = jpeg_ref.parse_jpeg(data)
            jc.check_structure(data, parsed, 40, 24, 80, "4:2:0")
            assert Image.open(io.BytesIO(data)).size == (40, 24)
            assert (seen[(t, i)] == jc.levels_of(frame)).all()
    # the same metadata as the PIL path writes
    import json
    fake3 = _fake(drv, allow_rgba=True)
    sweep.run(fake3, None, trs, "0042", str(tmp_path / "p"), resolution=(40, 24), chunk=8, quality=80)
    assert json.load(open(tmp_path / "p" / "image_metadata.json")) == json.load(open(tmp_path / "g" / "image_metadata.json"))
    # write=False needs no encoder at all; an unknown encoder is refused
    fake4 = _fake(drv, allow_rgba=True)
    fake4.jpeg_frames = None
    assert sweep.run(fake4, None, trs, "0042", str(tmp_path / "n"), resolution=(40, 24), encoder="gpu", write=False, force=True) == 11
    with pytest.raises(ValueError):
        sweep.run(fake4, None, trs, "0042", str(tmp_path / "n"), resolution=(40, 24), encoder="nvjpeg")


def test_cli_passes_encoder_and_quality_on(monkeypatch, tmp_path):
    """python -m sage_gs.sweep --encoder gpu --quality 80 reaches run() with both; the defaults are 'pil' and 95."""
    from sage_gs import ply, renderer

    class Scene:
        def free(self):
            pass

    class FakeRenderer:
        def __init__(self, dev):
            pass

        def upload(self, g):
            return Scene()

    calls = []
    monkeypatch.setattr(renderer, "Renderer", FakeRenderer)
    monkeypatch.setattr(ply, "load_ply", lambda path: None)
    monkeypatch.setattr(ply, "to_gaussians", lambda arrays, dev, m2w: None)
    monkeypatch.setattr(sweep, "load_trajectories", lambda path: [])
    monkeypatch.setattr(sweep, "run", lambda *a, **kw: calls.append((a, kw)) or 0)
    base = ["--out", str(tmp_path), "--scene", "s.ply", "--actions", "a.json", "--scene-id", "1", "--device", "cuda:0"]
    sweep.main(base + ["--encoder", "gpu", "--quality", "80"])
    sweep.main(base)
    assert [(kw["encoder"], kw["quality"]) for _, kw in calls] == [("gpu", 80), ("pil", 95)]
    with pytest.raises(SystemExit):
        sweep.main(["--out", "x", "--scene", "s.ply", "--actions", "a.json", "--scene-id", "1", "--encoder", "turbo"])
    with pytest.raises(SystemExit):
        sweep.main(["--out", "x", "--scene", "s.ply", "--actions", "a.json", "--scene-id", "1", "--encoder", "gpu", "--quality", "0"])
