"""The top-down seen map (sgs_topdown_map, sgs_topdown_summary; csrc/sgs_topdown.h) under the wave64 emulator: the kernels' own source,
on the CPU, through the C ABI.  Every picture of tests/topdown_cases.py against the NumPy restatement (tests/topdown_ref.py, itself
held to a Python loop and a hand-computed case by test_topdown_ref.py), every count exactly; mesh depth frames rendered by
sgs_render_mesh_depth_batch; batches with a padded stride, accumulation with and without SGS_TOPDOWN_CLEAR; the summary; the refusals,
misaligned buffers among them; and the split of a call into launches of SGS_TOPDOWN_MAX_FRAMES frames, on a build whose constant is 4."""
import ctypes as C

import numpy as np
import pytest

import emu_harness
import topdown_cases as tc
import topdown_ref as ref
from sage_gs import _capi

SPLIT_CHUNK = 4


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(the emulator library, a build of a copy of csrc/ whose SGS_TOPDOWN_MAX_FRAMES is 4), compiled side by side."""
    path, proc = emu_harness.start_emu_copy(tmp_path_factory.mktemp("topdown_split"), {"sgs_topdown.h": [tc.chunk_edit(SPLIT_CHUNK)]})
    main = emu_harness.build_emu()
    assert proc.wait() == 0, "the copy with launches of 4 frames does not compile"
    return main, path


@pytest.fixture(scope="module")
def lib(libs):
    return _capi.Lib(libs[0])


@pytest.fixture(scope="module")
def drv(lib):
    d = tc.AbiTopdown(lib)
    yield d
    d.close()


@pytest.fixture(scope="module")
def split_drv(libs):
    d = tc.AbiTopdown(_capi.Lib(libs[1]))
    yield d
    d.close()


def test_the_pictures_are_what_they_are_built_for():
    tc.check_picture_properties()


@pytest.mark.parametrize("make", tc.SMALL + tc.LARGE, ids=lambda m: m.__name__)
def test_pictures(drv, make):
    tc.check_pictures(drv, [make])


def test_hand_computed_case(drv):
    import test_topdown_ref
    depth, P, p = test_topdown_ref.hand_case()
    grid, counts = drv.map(depth, P, p)
    assert counts.tolist() == [[1, 1, 1, 5]]
    assert sorted(zip(*(v.tolist() for v in np.nonzero(grid)))) == [(0, 0, 0), (0, 1, 1), (0, 2, 0), (0, 2, 1), (2, 0, 0)] and grid.max() == 1


def test_rendered_room_frames(drv, lib):
    import mesh_edge_cases
    from sage_gs import scenes
    m = scenes.make_room_mesh(2000)
    e = mesh_edge_cases.EmuMesh(lib)
    try:
        tc.check_rendered(drv, lambda cams: e.frames(m.vertices, m.triangles, [__import__("mesh_depth_ref").of_camera(c) for c in cams])[0])
    finally:
        e.close()


def test_batches_and_padded_strides(drv):
    tc.check_batches(drv)


def test_accumulation_and_clear(drv):
    tc.check_accumulation(drv)


def test_summary(drv):
    tc.check_summary(drv)


def test_refusals(drv):
    tc.check_refusals(drv)


def test_misaligned_buffers_are_refused(drv):
    tc.check_misaligned(drv)


def test_split_launch_with_chunks_of_4_frames(split_drv):
    """sgs_topdown_map cuts n_frames into launches of SGS_TOPDOWN_MAX_FRAMES (gridDim.y): with the constant at 4, 11 one-pixel frames
    take two full launches and a short one; then the batches of 1, 3 and 9 frames, the last of which is cut 4 + 4 + 1."""
    assert tc.check_split(split_drv, SPLIT_CHUNK) == 2 * SPLIT_CHUNK + 3
    tc.check_batches(split_drv)


def test_binding_mirrors_the_structs(lib):
    fields = [("nx", 0, 4), ("ny", 4, 4), ("origin_x", 8, 4), ("origin_y", 12, 4), ("cell_size", 16, 4), ("min_z", 20, 4), ("max_z", 24, 4),
              ("free_lo", 28, 4), ("free_hi", 32, 4), ("occ_lo", 36, 4), ("occ_hi", 40, 4), ("flags", 44, 4), ("reserved", 48, 4)]
    assert [(n, getattr(_capi.SgsTopdownParams, n).offset, getattr(_capi.SgsTopdownParams, n).size) for n, _ in _capi.SgsTopdownParams._fields_] == fields
    assert C.sizeof(_capi.SgsTopdownParams) == 52 and C.sizeof(_capi.SgsTopdownSummary) == 32 and _capi.TOPDOWN_CLEAR == ref.CLEAR == 1
    assert [n for n, _ in _capi.SgsTopdownSummary._fields_] == ["occupied_cells", "free_cells", "free_hits", "occupied_hits"]
    assert {"sgs_topdown_params_default", "sgs_topdown_map", "sgs_topdown_summary"} <= set(_capi.EXPORTS)
    d = _capi.SgsTopdownParams()
    lib.sgs_topdown_params_default(C.byref(d))
    want = ref.Params()
    for n, _ in _capi.SgsTopdownParams._fields_:
        assert getattr(d, n) == (np.float32(getattr(want, n)) if isinstance(getattr(want, n), float) else getattr(want, n)), n
    header = open(__import__("os").path.join(__import__("emu_harness").ROOT, "include", "sage_gs.h")).read()
    assert "#define SGS_TOPDOWN_CLEAR 1u" in header and "#define SGS_VERSION 114" in header
