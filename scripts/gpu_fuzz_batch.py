#!/usr/bin/env python3
"""sgs_render_batch* against the same frames rendered alone, bit for bit, on random indoor scenes (scenes.make_room / make_trained_like) with
random camera sets — runs of neighbouring headings (the groups the library projects with ONE grid over the scene's chunks,
k_preprocess_shared), views that share nothing (every frame its own live list), and mixes of both — at random resolutions (some small
enough for fine tiles), whole frames and bands of tile rows:   python scripts/gpu_fuzz_batch.py FIRST LAST   (the case: tests/fuzz_cases.py batch_seed)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "sage-3d_official_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
import fuzz_cases
from sage_gs import Renderer

r = Renderer(torch.device("cuda", 0))
a, b = int(sys.argv[1]), int(sys.argv[2])
bad, frames = [], 0
for seed in range(a, b):
    try:
        frames += fuzz_cases.batch_seed(r, seed)
    except Exception as e:                                   # noqa: BLE001
        bad.append(seed); print("FAIL", seed, repr(e)[:400], flush=True)
print(f"batch seeds [{a},{b}): {frames} frames, {len(bad)} failures {bad}")
r.close()
