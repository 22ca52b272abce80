"""NumPy restatement of the top-down seen map (sgs_topdown_map, sgs_topdown_summary; include/sage_gs.h) — this project's own definition.
np.float32 elementwise arithmetic in the order the header writes it (NumPy rounds every fp32 multiply and add once and fuses nothing),
masks, np.add.at.  tests/test_topdown_ref.py holds it to a pixel-by-pixel Python loop and to a hand-computed case; the kernels
(csrc/sgs_topdown.h) are held to it, every count exactly."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

F = np.float32
CLEAR = 1


@dataclass(frozen=True)
class Params:
    """sgs_topdown_params, with sgs_topdown_params_default's values."""
    nx: int = 256
    ny: int = 256
    origin_x: float = -6.4
    origin_y: float = -6.4
    cell_size: float = 0.05
    min_z: float = 0.1
    max_z: float = 6.5
    free_lo: float = -0.15
    free_hi: float = 0.15
    occ_lo: float = 0.15
    occ_hi: float = 1.5
    flags: int = CLEAR
    reserved: int = 0

    def but(self, **kw):
        return replace(self, **kw)


def classify(depth, P, p: Params):
    """One frame: depth fp32 [H,W], P fp32 [12] -> (cls int8 [H,W]: 0 z out of range, 1 outside the grid, 2 in no band, 3 binned;
    key int64 [H,W]: 2 (j nx + i) + channel where cls == 3, -1 elsewhere)."""
    z = np.asarray(depth, F)
    P = np.asarray(P, F).reshape(12)
    H, W = z.shape
    fx = np.arange(W).astype(F)[None, :]
    fy = np.arange(H).astype(F)[:, None]
    with np.errstate(all="ignore"):
        d = [(fx * P[3 * k] + fy * P[3 * k + 1]) + P[3 * k + 2] for k in range(3)]
        pk = [z * d[k] + P[9 + k] for k in range(3)]
        inv = F(1.0) / F(p.cell_size)
        u = (pk[0] - F(p.origin_x)) * inv
        v = (pk[1] - F(p.origin_y)) * inv
        h = pk[2]
        in_z = (F(p.min_z) <= z) & (z <= F(p.max_z))
        inside = (u >= F(0)) & (u < F(p.nx)) & (v >= F(0)) & (v < F(p.ny))
        free = (F(p.free_lo) <= h) & (h <= F(p.free_hi))
        occ = ~free & (F(p.occ_lo) < h) & (h <= F(p.occ_hi))
    assert all(a.dtype == F for a in d + pk + [u, v])
    cls = np.where(~in_z, 0, np.where(~inside, 1, np.where(~(free | occ), 2, 3))).astype(np.int8)
    binned = cls == 3
    i = np.where(binned, u, F(0)).astype(np.int64)
    j = np.where(binned, v, F(0)).astype(np.int64)
    key = np.where(binned, 2 * (j * p.nx + i) + occ.astype(np.int64), -1)
    return cls, key


def topdown(depth, P, p: Params, grid=None):
    """depth fp32 [n,H,W], P fp32 [n,12] -> (grid uint32 [ny,nx,2], counts uint32 [n,4]).  grid: what the grid held before the call;
    with CLEAR (or None) it starts from zero."""
    depth = np.asarray(depth, F)
    n = depth.shape[0]
    flat = np.zeros(2 * p.nx * p.ny, np.uint32)
    if grid is not None and not (p.flags & CLEAR):
        flat[:] = np.asarray(grid, np.uint32).reshape(-1)
    counts = np.zeros((n, 4), np.uint32)
    for f in range(n):
        cls, key = classify(depth[f], np.asarray(P, F).reshape(n, 12)[f], p)
        counts[f] = np.bincount(cls.reshape(-1), minlength=4)
        np.add.at(flat, key[key >= 0], np.uint32(1))
    return flat.reshape(p.ny, p.nx, 2), counts


def summary(grid, min_hits=1):
    """sgs_topdown_summary's four numbers as Python ints."""
    g = np.asarray(grid, np.uint32)
    fr, oc = g[..., 0].astype(np.uint64), g[..., 1].astype(np.uint64)
    return [int((oc >= min_hits).sum()), int(((oc < min_hits) & (fr >= min_hits)).sum()), int(fr.sum()), int(oc.sum())]


def pix_to_map(fx, fy, cx, cy, view, model_to_map=None):
    """The twelve numbers of a pinhole camera (+Z forward, +X right, +Y down; view: world -> camera, rigid) in fp64, rounded once:
    map_from_cam . [(1/fx, 0, (0.5 - cx)/fx); (0, 1/fy, (0.5 - cy)/fy); (0, 0, 1)], then the camera's position in the map."""
    c2w = np.linalg.inv(np.asarray(view, np.float64).reshape(4, 4))
    m = np.eye(4)
    if model_to_map is not None:
        m[:3] = np.asarray(model_to_map, np.float64).reshape(3, 4)
    c2m = m @ c2w
    K = np.array([[1.0 / fx, 0.0, (0.5 - cx) / fx], [0.0, 1.0 / fy, (0.5 - cy) / fy], [0.0, 0.0, 1.0]])
    return np.concatenate([(c2m[:3, :3] @ K).reshape(9), c2m[:3, 3]]).astype(F)
