"""Collision-mesh depth where pixels lie on shared edges, on the near / far planes, with degenerate input and with more than 1024 tiles,
under the wave64 emulator (cases: tests/mesh_edge_cases.py; checks: mesh_depth_ref.check and the edge-exact check_continuous).  CPU only."""
import math

import numpy as np
import pytest

import emu_harness as eh
import mesh_depth_ref as ref
import mesh_edge_cases as mc
from sage_gs import scenes


@pytest.fixture(scope="module")
def drv():
    d = mc.EmuMesh(eh.lib())
    yield d
    d.close()


def test_continuous_check_rejects_cracks_that_check_accepts():
    """NumPy only: the pixel-centre lattice sheet with +inf on its edge band is a frame full of cracks.  check() accepts it (strict is
    +inf there); check_continuous() rejects it — and accepts the crack-free frame."""
    case = mc.lattice_sheet(128, 96, seed=0, step=4, exact=False)
    rc, cc = mc.reference(case)
    n_edge = int(rc["edge"].sum())
    assert n_edge > 5000 and np.isinf(rc["strict"][rc["edge"]]).all()
    cracked = np.where(rc["edge"], np.inf, rc["nominal"]).astype(np.float32)
    assert ref.check(cracked, rc, "cracked lattice")[0] == 0
    with pytest.raises(AssertionError, match="must claim"):
        ref.check_continuous(cracked, cc, "cracked lattice")
    n = ref.check_continuous(rc["nominal"].astype(np.float32), cc, "lattice, fp64 nominal")
    assert n["shared_band"] > 5000 and n["need"] > 9000
    # the box: a crack that shows nothing, and a seam pixel set to the farther of its faces' values, +1e-4: both rejected
    box = mc.box(96, 64, seed=1)
    rb, cb = mc.reference(box)
    got = rb["nominal"].astype(np.float32)
    ref.check_continuous(got, cb, "box, fp64 nominal")
    bad = got.copy(); bad[10, 10] = np.inf
    with pytest.raises(AssertionError):
        ref.check_continuous(bad, cb, "box with a hole")
    bad = got.copy(); bad[20, 30] = np.float32(cb["hi"][20, 30] * (1 + 1e-4))
    with pytest.raises(AssertionError):
        ref.check_continuous(bad, cb, "box, one pixel too deep")


@pytest.mark.parametrize("name", list(mc.EDGE_CASES))
@pytest.mark.parametrize("w,h", [(128, 96), (200, 136)])
def test_edge_case(drv, name, w, h):
    mc.check_edge_case(drv, name, w, h, seed=w)


def test_edge_cases_batch_equals_single(drv):
    """The lattice sheet in a batch of 10 (groups of 8 + 2): its own camera at frames 0 and 9 (bit for bit the single frame), slightly
    moved cameras elsewhere, every frame under both checks."""
    case = mc.lattice_sheet(96, 64, seed=4, step=4, exact=False)
    single, _ = drv.frame(case["V"], case["T"], case["cam"])
    rng = np.random.default_rng(4)
    cams = [case["cam"]]
    for k in range(8):
        cams.append(mc.nudged(case["cam"], rng))
    cams.append(case["cam"])
    got, st = drv.frames(case["V"], case["T"], cams)
    assert np.array_equal(got[0], single) and np.array_equal(got[9], single)
    for k in range(1, 9):
        mc.check_frame(got[k], case, cam=cams[k], what=f"lattice batch frame {k}")
    assert all(s["d_total"] > 0 for s in st)


def test_room_far_plane(drv):
    """far_z = 3 cuts the room: the far walls vanish, the near furniture stays."""
    m = scenes.make_room_mesh(3000, seed=2)
    rng = np.random.default_rng(7)
    fx, fy, cx, cy = scenes.reference_intrinsics(160, 120)
    for k in range(2):
        cam = ref.cam_dict(160, 120, fx, fy, cx, cy, scenes.view_from_yaw((rng.uniform(1.2, 4.8), rng.uniform(1.2, 3.8), 1.2),
                                                                          rng.uniform(0, 2 * math.pi), rng.uniform(-0.5, 0.5)))
        got, _ = drv.frame(m.vertices, m.triangles, cam, far=3.0)
        ref.check(got, ref.cast(m.vertices, m.triangles, cam, near=0.2, far=3.0), f"room far 3, pose {k}")
        assert np.isinf(got).sum() > 500 and np.isfinite(got).sum() > 500 and (got[np.isfinite(got)] <= 3.0).all()


def test_near_far_exact(drv):
    mc.case_near_far_exact(drv)


def test_triangle_through_far_plane(drv):
    mc.case_far_straddle(drv)


def test_degenerate_and_culled_triangles(drv):
    m = scenes.make_room_mesh(2000, seed=5)
    fx, fy, cx, cy = scenes.reference_intrinsics(96, 72)
    cam = ref.cam_dict(96, 72, fx, fy, cx, cy, scenes.view_from_yaw((2.5, 2.0, 1.2), 0.7, 0.1))
    want = mc.case_degenerate(drv, (m.vertices, m.triangles), cam)
    ref.check(want, ref.cast(m.vertices, m.triangles, cam, near=0.2, far=20.0), "room, far 20")


def test_exactly_collinear_triangles(drv):
    mc.case_collinear_exact(drv)


def test_more_than_1024_tiles(drv):
    st = mc.case_many_tiles(drv)
    print(f"528x528: {st['n_tiles']} tiles, {st['d_total']} records, longest list {st['max_tile_len']}")


@pytest.mark.parametrize("seed", [128, 5, 6])
def test_inexact_lattice_vertex_pixels_are_claimed(drv, seed):
    """Pixels whose ray passes within fp32 rounding of a shared lattice vertex: the rounded edge planes through it can all show one strict
    sign there, and the kernel's fp64 recheck must still find the fan's triangle (seed 128 loses 3 of them without it)."""
    case = mc.lattice_sheet(128, 96, seed=seed, step=4, exact=False)
    got, _ = drv.frame(case["V"], case["T"], case["cam"])
    cc = ref.cast_continuous(case["V"], case["T"], case["cam"])
    at_vertex = cc["vertex"] & cc["need"]
    assert at_vertex.sum() > 300
    assert np.isfinite(got[at_vertex]).all(), f"{int(np.isinf(got[at_vertex]).sum())} of {int(at_vertex.sum())} vertex pixels fall through"
    ref.check_continuous(got, cc, f"lattice inexact seed {seed}")
