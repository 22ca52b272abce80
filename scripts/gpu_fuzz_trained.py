#!/usr/bin/env python3
"""Random scenes with trained-3DGS statistics (scenes.make_trained_like, SH degree 3, the asset's -90 degree model transform) at random sizes, resolutions
and poses through the full oracle comparison:  python scripts/gpu_fuzz_trained.py FIRST LAST   (the case: tests/fuzz_cases.py trained_seed)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "sage-3d_official_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import conftest, fuzz_cases
from test_gpu_parity import GpuDriver
drv = GpuDriver()
a, b = int(sys.argv[1]), int(sys.argv[2])
bad = []
for seed in range(a, b):
    try:
        fuzz_cases.trained_seed(drv, seed)
    except Exception as e:                                   # noqa: BLE001
        bad.append(seed); print("FAIL", seed, repr(e)[:500], flush=True)
print(f"trained-like seeds [{a},{b}): {len(bad)} failures {bad}")
