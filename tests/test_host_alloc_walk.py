"""The allocation-failure walk of the library's host side (tests/host_alloc_walk.cpp says what it checks): csrc/sgs_api.hip and the
walk program, compiled against the emulator with AddressSanitizer into one stand-alone program, which refuses every device / pinned
allocation of a script of calls in turn.  The failure points are dealt to a few child processes (one thread each: the script's grids
are a handful of workgroups); every child must exit with status 0 and print no sanitizer report (bad accesses, leaks at exit)."""
import os
import re
import subprocess

import emu_harness

WALK_SRC = os.path.join(emu_harness.ROOT, "tests", "host_alloc_walk.cpp")
BUILD_LIMIT_S = 900
WALK_LIMIT_S = 1800


def test_every_allocation_may_fail(tmp_path):
    exe = str(tmp_path / "host_alloc_walk")
    subprocess.run(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fopenmp", "-fsanitize=address", "-I", emu_harness.EMU_DIR,
                    os.path.join(emu_harness.PKG, "csrc", "sgs_api.hip"), WALK_SRC, "-o", exe], check=True, timeout=BUILD_LIMIT_S)
    env = dict(os.environ, OMP_NUM_THREADS="1")
    # the unfailed script alone: how many allocations there are to refuse
    first = subprocess.run([exe, "0", "0"], env=env, capture_output=True, text=True, timeout=WALK_LIMIT_S)
    assert first.returncode == 0, first.stderr[-4000:]
    n = int(re.search(r"(\d+) allocations", first.stderr).group(1))
    assert n > 100, first.stderr                       # (the script reaches every entry point that allocates)
    workers = max(1, min(8, os.cpu_count() or 1))
    step = -(-n // workers)
    procs = [(k, subprocess.Popen([exe, str(k), str(min(k + step, n))], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
             for k in range(0, n, step)]
    walked = 0
    for k, p in procs:
        try:
            out, _ = p.communicate(timeout=WALK_LIMIT_S)
        except subprocess.TimeoutExpired:
            for _, q in procs:
                q.kill()
            raise
        assert p.returncode == 0, f"failure points from {k}: exit status {p.returncode}\n{out[-6000:]}"
        assert "Sanitizer" not in out, out[-6000:]
        walked += int(re.search(r"0 of (\d+) failure points wrong", out).group(1))
    assert walked == n, (walked, n)                    # no k is skipped
