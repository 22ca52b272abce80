"""bench.py's command line on a CPU-only box: `--gpus N` outside a launcher must launch itself as one rank per GPU (round-3 review: the
driver's SCALE step may well be `python bench.py --gpus 8 ...`), and the pose-file sweep deals scenes to instances by a STABLE hash."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import importlib
    return importlib.import_module("bench")


def test_self_launch_argv_is_the_drivers_command_shape():
    b = _bench()
    argv = b.self_launch_argv(8, ["--gpus", "8", "--steps", "20", "--warmup", "5"], port=29517)
    assert argv[0] == sys.executable and argv[1:3] == ["-m", "torch.distributed.run"]
    assert "--nnodes=1" in argv and "--nproc-per-node=8" in argv
    assert argv[argv.index("--master-addr") + 1] == "127.0.0.1" and argv[argv.index("--master-port") + 1] == "29517"
    k = argv.index(os.path.join(ROOT, "bench.py"))
    assert argv[k + 1:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    free = b.self_launch_argv(2, [])                    # a free port is picked when none is given
    assert 1024 < int(free[free.index("--master-port") + 1]) < 65536


def test_gpus_2_outside_a_launcher_relaunches_itself_one_rank_per_gpu():
    """No GPU here, so every rank stops at bench.py's own "needs a GPU" assertion — which it can only reach as a rank of the relaunched
    job (WORLD_SIZE=2): two such failures, not the old "must be launched with torch.distributed.run" exit."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    out = p.stdout + p.stderr
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU box runs the real thing (tests/test_gpu_sharded.py)")
    assert p.returncode != 0
    assert "must be launched with torch.distributed.run" not in out
    assert out.count("bench.py needs a GPU") >= 2, out[-2000:]


def test_scene_instances_are_stable_and_cover_every_scene_once(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))
    from sage_gs import sweep
    ids = [f"{i:04d}" for i in range(1, 41)] + ["0839_b", "scene-α"]
    for i in ids:
        d = tmp_path / "actions" / i
        d.mkdir(parents=True)
        (d / "action_groundtruth.json").write_text('{"groundtruth_data": []}')
    (tmp_path / "actions" / "not_a_scene").mkdir()          # no action file: ignored
    for total in (1, 2, 8):
        shares = [sweep.scenes_of_instance(str(tmp_path / "actions"), k, total) for k in range(total)]
        assert sorted(i for s in shares for i in s) == sorted(ids)                 # every scene exactly once
        assert all(s == sorted(s) for s in shares)
    # known answers (CRC-32, not Python's salted hash): the same in every process, whatever PYTHONHASHSEED says
    assert [sweep.scene_instance(i, 8) for i in ("0001", "0002", "0839", "scene-α")] == [4, 6, 5, 7]
    code = ("import sys; sys.path.insert(0, %r); from sage_gs import sweep; "
            "print([sweep.scene_instance(i, 8) for i in ('0001', '0002', '0839', 'scene-α')])" % os.path.join(ROOT, "sage-3d_official_amd"))
    for seed in ("0", "12345"):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONHASHSEED=seed), capture_output=True, text=True, timeout=120)
        assert out.stdout.strip() == "[4, 6, 5, 7]", out.stdout + out.stderr
    with pytest.raises(ValueError):
        sweep.scenes_of_instance(str(tmp_path / "actions"), 8, 8)
    # scene files: plain, nested, compressed
    root = tmp_path / "scenes"; (root / "0002").mkdir(parents=True)
    (root / "0001.ply").write_bytes(b"x"); (root / "0002" / "3dgs_compressed.ply").write_bytes(b"x")
    assert sweep.find_scene_file(str(root), "0001") == (str(root / "0001.ply"), False)
    assert sweep.find_scene_file(str(root), "0002") == (str(root / "0002" / "3dgs_compressed.ply"), True)
    assert sweep.find_scene_file(str(root), "0003") == (None, False)


def test_dump_frame_writes_float32_and_a_fixed_sample_of_a_large_frame(tmp_path, monkeypatch):
    """--dump-outputs: the last step's frame as float32 .npy (uint8 RGBA frames keep their 0..255 values); a frame over the size limit
    becomes a seeded sample of its pixels, the same pixels in every run."""
    import numpy as np
    import torch
    b = _bench()
    f32 = torch.rand((6, 5, 3), generator=torch.Generator().manual_seed(1))
    b.dump_frame(str(tmp_path / "a"), f32)
    a = np.load(tmp_path / "a" / "frame.npy")
    assert a.dtype == np.float32 and a.shape == (6, 5, 3) and (a == f32.numpy()).all()
    u8 = torch.arange(6 * 5 * 4, dtype=torch.int64).remainder(256).to(torch.uint8).reshape(6, 5, 4)
    b.dump_frame(str(tmp_path / "b"), u8)
    a = np.load(tmp_path / "b" / "frame.npy")
    assert a.dtype == np.float32 and (a == u8.numpy().astype(np.float32)).all()
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 100)
    monkeypatch.setattr(b, "DUMP_SAMPLE_PIXELS", 7)
    for d in ("c", "d"):
        b.dump_frame(str(tmp_path / d), f32)
        assert not (tmp_path / d / "frame.npy").exists()
    s, s2 = np.load(tmp_path / "c" / "frame_sample.npy"), np.load(tmp_path / "d" / "frame_sample.npy")
    assert s.dtype == np.float32 and s.shape == (7, 3) and (s == s2).all()
    px = f32.numpy().reshape(-1, 3)
    assert all(any((row == p).all() for p in px) for row in s)          # pixels of the frame, not made-up values


@pytest.mark.gpu
def test_plain_line_is_the_headline_and_dumps_the_last_steps_frame(tmp_path):
    """A plain run: exactly --steps timed steps, the contract's fields and none of --full's side measurements; --dump-outputs holds the
    frame of the last timed step — the frame the renderer draws for that pose on its own."""
    import json
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "sage-3d_official_amd"))
    from sage_gs import Renderer, scenes
    K, W, n = 5, 2, 300_000
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
                        "--gaussians", str(n), "--dump-outputs", str(tmp_path / "out")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == K and d["warmup"] == W and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and abs(d["ms_per_step"] * K - d["timed_region_ms"]) < 1e-6 * d["timed_region_ms"]
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3
    for side in ("roofline", "latency_ms", "value_100", "also_measured", "cpu_baseline"):
        assert side not in d, side
    assert d["verify"] is None
    got = np.load(tmp_path / "out" / "frame.npy")
    assert got.dtype == np.float32 and got.shape == (1080, 1920, 3) and np.isfinite(got).all()
    sc = scenes.make_room(n, seed=2)
    cams = scenes.room_cameras(sc, 1920, 1080, n_positions=4, n_yaw=64, seed=2)
    r = Renderer("cuda:0")
    gs = r.upload(scenes.to_gaussians(sc, "cuda:0"))
    ref = r.render(cams[((W + K - 1) * 77) % len(cams)], gs).cpu().numpy()
    r.close()
    assert float(np.abs(got - ref).max()) < 1e-5 and float(ref.max()) > 0
