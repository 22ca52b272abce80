"""BASELINE configs[3] logic on ONE GPU: `ShardedRenderer` for real — 2 and 3 ranks (one process each, as deployed)
sharing cuda:0 under gloo, every rank rendering ITS band of tile rows with the HIP library, rank 0 receiving the
gatherv.  The gathered frame must be bit-identical to the frame the same library renders un-sharded.  (On the 8-GPU
node the only difference is the backend string: "nccl" = RCCL over xGMI, one GPU per rank.)"""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, mode, n_gauss, res, q, backend="gloo"):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "sage-3d_official_amd"))
    import torch
    import torch.distributed as dist
    from sage_gs import Renderer, scenes
    from sage_gs.dist import ShardedRenderer, row_partition
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    # gloo: every rank on cuda:0 (a 1-GPU box); nccl (= RCCL): one GPU per rank, exactly bench.py's init call
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        assert torch.cuda.is_available()
        w, h = res
        sc = scenes.make_room(n_gauss, seed=1)
        cams = scenes.room_cameras(sc, w, h, n_positions=1, n_yaw=10, seed=1)
        r = Renderer(dev)
        scene = r.upload(scenes.to_gaussians(sc, dev))
        exchange = "frames" if mode.endswith("+frames") else "slab"      # (the default: one operation per peer and exchange)
        mode = mode.replace("+frames", "")
        rgba8 = mode.startswith("rgba8")
        sr = ShardedRenderer(r, h, w, batch=4, interleave=(mode == "interleave"), balance=mode.endswith("balance"),
                             output="rgba8" if rgba8 else "float32", exchange=exchange)
        ok, notes = True, []
        whole = [r.render(c, scene).clone() for c in cams] if rank == 0 else None      # the un-sharded HIP frames
        if rgba8 and rank == 0:                     # bands travel as bytes: rank 0 must hold pack_rgba8 of the un-sharded frame
            whole = [r.pack_rgba8(f) for f in whole]
        chans = 4 if rgba8 else 3
        # one frame at a time (the latency mode)
        for i in (0, 3):
            f = sr.render(cams[i], scene)
            if rank == 0:
                same = bool((f == whole[i]).all())
                ok = ok and same and tuple(f.shape) == (h, w, chans)
                if not same:
                    notes.append(f"render cam {i}: {(f != whole[i]).sum().item()} values differ")
        # a sweep: batches of 4 (last partial), two exchanges in flight
        r.row_records((h + 15) // 16, reset=True)
        done, bands_seen = [], []
        for c0 in range(0, len(cams), 4):
            ids = list(range(c0, min(len(cams), c0 + 4)))
            g = sr.render_batch([cams[i] for i in ids], scene)
            bands_seen.append(tuple(g.bands))
            if g.mode == "slab":                   # one operation per peer with rows, whatever the batch holds
                ok = ok and g.last_ops <= world - 1 and exchange == "slab" and mode != "interleave"
            done.append((g, ids, sr._turn ^ 1))
            if len(done) == 2:
                g0, ids0, k0 = done.pop(0)
                if sr._pending[k0] is not None:
                    sr._pending[k0].wait(); sr._pending[k0] = None
                if rank == 0:
                    for j, i in enumerate(ids0):
                        same = bool((g0.frame(j) == whole[i]).all())
                        ok = ok and same
                        if not same:
                            notes.append(f"batch cam {i}: {(g0.frame(j) != whole[i]).sum().item()} values differ")
        sr.finish()
        for g0, ids0, _ in done:
            if rank == 0:
                for j, i in enumerate(ids0):
                    same = bool((g0.frame(j) == whole[i]).all())
                    ok = ok and same
                    if not same:
                        notes.append(f"batch(tail) cam {i}: {(g0.frame(j) != whole[i]).sum().item()} values differ")
        if mode.endswith("balance"):
            even = tuple(row_partition((h + 15) // 16, world))
            # (the re-cut bands come from wall-clock band times: whether they differ from the even split is up to the box —
            #  the first batch must be even, the later ones valid partitions; the frames above are the check)
            gy_ = (h + 15) // 16
            ok = ok and bands_seen[0] == even and all(b[0][0] == 0 and b[-1][1] == gy_ and all(b[i][0] == b[i - 1][1] for i in range(1, world))
                                                      for b in bands_seen)
            notes.append(f"bands {bands_seen}")
        st = sr.last_stats
        ok = ok and st is not None and st["n_visible"] > 0
        if rank == 0:
            q.put((ok, notes))
        dist.barrier()
        scene.free(); r.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,mode", [(2, "even"), (3, "even"), (3, "balance"), (2, "interleave"), (3, "interleave"),
                                        (3, "rgba8-balance"), (2, "even+frames"), (3, "balance+frames")])
def test_sharded_renderer_on_one_gpu(world, mode):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, mode, 500_000, (1920, 1080), q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0, f"rank process exited with {p.exitcode}"
    ok, notes = q.get(timeout=10)
    assert ok, notes


@pytest.mark.parametrize("world,mode", [(2, "even"), (2, "balance"), (2, "rgba8-balance"), (8, "even"), (2, "balance+frames"), (8, "even+frames")])
def test_sharded_renderer_on_rccl_when_the_box_has_gpus(world, mode):
    """The same check on the backend the 8-GPU node uses: "nccl" = RCCL, one GPU per rank — two ranks (and, where the box has them, up to eight) —
    the gathered frame bit-identical to the un-sharded one.  RCCL refuses two ranks on one device, so on a 1-GPU box this SKIPS, loudly: the
    N > 1 RCCL exchange is then only covered by bench.py's own `verify` step on the multi-GPU node."""
    import torch
    n_dev = torch.cuda.device_count()
    if n_dev < 2:
        pytest.skip(f"RCCL with N > 1 ranks needs N GPUs; this box has {n_dev} — the exchange itself runs here under gloo "
                    f"(test_sharded_renderer_on_one_gpu, test_bench_multi_rank_line_verifies_itself_on_one_gpu) and on RCCL at world size 1 "
                    f"(test_rccl_world_size_one_smoke)")
    if world > 2 and n_dev < 3:
        pytest.skip(f"the {world}-rank case needs more than the {n_dev} GPUs of this box")
    import torch.multiprocessing as mp
    world = min(world, n_dev)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, mode, 500_000, (1920, 1080), q, "nccl")) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0, f"rank process exited with {p.exitcode}"
    ok, notes = q.get(timeout=10)
    assert ok, notes


def _nccl_worker(port, q):
    """world size 1 on RCCL: communicator creation, a device all_reduce, ShardedRenderer on device tensors."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "sage-3d_official_amd"))
    import torch
    import torch.distributed as dist
    from sage_gs import Renderer, scenes
    from sage_gs.dist import ShardedRenderer
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)       # exactly bench.py's call
    try:
        t = torch.full((4,), 3.0, device=dev)
        dist.all_reduce(t)                                                     # a device collective on the communicator
        torch.cuda.synchronize()
        ok = bool((t == 3.0).all()) and dist.get_backend() == "nccl"
        sc = scenes.make_room(60_000, seed=1)
        cams = scenes.room_cameras(sc, 640, 480, n_positions=1, n_yaw=6, seed=1)
        r = Renderer(dev)
        scene = r.upload(scenes.to_gaussians(sc, dev))
        whole = [r.render(c, scene).clone() for c in cams]
        notes = []
        for out in ("float32", "rgba8"):
            sr = ShardedRenderer(r, 480, 640, batch=4, balance=True, output=out)
            f = sr.render(cams[0], scene)
            want = [r.pack_rgba8(w) for w in whole] if out == "rgba8" else whole
            ok = ok and bool((f == want[0]).all())
            for c0 in (0, 4):                                                  # two batches: the second one re-cuts the bands
                ids = list(range(c0, min(6, c0 + 4)))
                g = sr.render_batch([cams[i] for i in ids], scene)
                sr.finish()
                for j, i in enumerate(ids):
                    same = bool((g.frame(j) == want[i]).all())
                    ok = ok and same
                    if not same:
                        notes.append(f"{out} cam {i} differs")
        dist.barrier()
        torch.cuda.synchronize()
        q.put((ok, notes))
        scene.free(); r.close()
    finally:
        dist.destroy_process_group()


def test_rccl_world_size_one_smoke():
    """The "nccl" (= RCCL) branch of bench.py / sage_gs.dist has no multi-GPU box to run on here; at world size 1 at least
    communicator creation, a device-tensor all_reduce, the cost all-reduce of the balanced bands and the ShardedRenderer
    calls execute on ROCm, with frames identical to the un-sharded ones."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_worker, args=(_free_port(), q))
    p.start()
    p.join(600)
    assert p.exitcode == 0, f"the RCCL process exited with {p.exitcode}"
    ok, notes = q.get(timeout=10)
    assert ok, notes


def test_bench_multi_rank_line_verifies_itself_on_one_gpu():
    """`python bench.py --gpus 2` end to end — the command the driver launches on a multi-GPU node — with both ranks on this box's one GPU under gloo
    (SGS_BENCH_SHARE_GPU=1: the only difference to the node is the backend string): the self-launch, the N > 1 code path, the self-check that
    runs before anything is timed (gathered frames == rank 0's un-sharded renders, bit for bit, through all three exchanges) and the JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SGS_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "2", "--gaussians", "300000",
                        "--full", "--no-secondary", "--no-cpu-baseline", "--no-lowres", "--preheat-ms", "0"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0 and d["metric_version"] >= 4
    v = d["verify"]
    # (10 = the single-frame exchange + 3 frames through each of the two gatherv shapes + 3 through the uint8 gather)
    assert v["ok"] and v["frames_checked"] == 10 and v["mismatching_pixels"] == 0 and v["ranks"] == 2
    assert v["p2p_ops_rank0_per_exchange_of_3_frames"] == {"slab": 1, "frames": 3}
    c = d["collective"]
    assert "fp32 bands" in d["config"]["parallelism"] and c["ranks"] == 2
    # --exchange auto: both shapes were timed before the sweep, one was chosen (the same on every rank, or the exchange would have hung), and
    # the gatherv alone was timed in both shapes afterwards with the operations rank 0 posted
    assert c["exchange"] == c["exchange_probe"]["chosen"] in ("slab", "frames")
    assert set(c["gather_us_per_frame"]) == {"slab", "frames"} and c["p2p_ops_rank0_per_exchange_of_8_frames"] == {"slab": 1, "frames": 8}
    assert "[verify]" in p.stderr and "bit-identical" in p.stderr
