"""The clearance map (sgs_clearance_map, sgs_clearance_query; csrc/sgs_clearance.h) under the wave64 emulator: the kernels' own
source, on the CPU, through the C ABI.  Every picture of tests/clearance_cases.py against the NumPy restatement
(tests/clearance_ref.py, itself held to a Python loop and to SciPy by test_clearance_ref.py), every cell and counter exactly; batches
with a padded, poisoned stride; the seen-map source, a grid sgs_topdown_map made from rendered depth frames among them; the queries,
the reference's own recorded answers among them (tests/golden/clearance_golden.json); the refusals; the binding's layout."""
import ctypes as C

import numpy as np
import pytest

import emu_harness
import clearance_cases as cc
import clearance_ref as ref
from sage_gs import _capi


@pytest.fixture(scope="module")
def lib():
    return _capi.Lib(emu_harness.build_emu())


@pytest.fixture(scope="module")
def drv(lib):
    d = cc.AbiClearance(lib)
    yield d
    d.close()


@pytest.mark.parametrize("size", cc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes(drv, size):
    cc.check_sizes(drv, [size])


def test_word_boundaries(drv):
    cc.check_pictures(drv, cc.lane_pictures())


def test_shapes(drv):
    cc.check_pictures(drv, cc.shape_pictures())


def test_batches_and_padded_strides(drv):
    cc.check_batches(drv)


def test_counters(drv):
    cc.check_counters(drv)


def test_seen_maps(drv):
    cc.check_seen_maps(drv)


def test_rendered_seen_map(drv, lib):
    import mesh_edge_cases
    import topdown_cases as tc
    from sage_gs import scenes
    m = scenes.make_room_mesh(2000)
    e = mesh_edge_cases.EmuMesh(lib)
    t = tc.AbiTopdown(lib)
    try:
        grid, _ = tc.check_rendered(t, lambda cams: e.frames(m.vertices, m.triangles, [__import__("mesh_depth_ref").of_camera(c) for c in cams])[0], W=80, H=60)
    finally:
        e.close()
        t.close()
    cc.check_rendered_seen_map(drv, grid[20:110, 10:140])


def test_query_rounding(drv):
    cc.check_rounding(drv)


def test_query_flags_margins_samples(drv):
    cc.check_flags_margins_samples(drv)


def test_query_non_finite(drv):
    cc.check_non_finite(drv)


def test_the_references_own_answers(drv, tmp_path):
    cc.check_golden(drv, tmp_path)


def test_refusals(drv):
    cc.check_refusals(drv)


def test_misaligned_buffers_are_refused(drv):
    cc.check_misaligned(drv)


def test_binding_mirrors_the_structs(lib):
    P, F = _capi.SgsClearanceParams, _capi.SgsClearanceFrame
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("nx", 0, 4), ("ny", 4, 4), ("source", 8, 4), ("flags", 12, 4), ("min_hits", 16, 4), ("max_d2", 20, 4), ("reserved", 24, 4)]
    assert [(n, getattr(F, n).offset, getattr(F, n).size) for n, _ in F._fields_] == [
        ("min_x", 0, 8), ("min_y", 8, 8), ("sum_x", 16, 8), ("sum_y", 24, 8), ("scale", 32, 8), ("flags", 40, 4), ("margin", 44, 4),
        ("max_d2", 48, 4), ("n_samples", 52, 4), ("reserved", 56, 8)]
    assert C.sizeof(P) == 28 and C.sizeof(F) == 64
    assert (_capi.CLEARANCE_NONE, _capi.CLEARANCE_SRC_MASK8, _capi.CLEARANCE_SRC_TOPDOWN, _capi.CLEARANCE_UNSEEN_BLOCKS) == (ref.NONE, ref.SRC_MASK8, ref.SRC_TOPDOWN, ref.UNSEEN_BLOCKS)
    assert (_capi.CLEARANCE_NEGATE, _capi.CLEARANCE_FLIP_X, _capi.CLEARANCE_FLIP_Y) == (ref.NEGATE, ref.FLIP_X, ref.FLIP_Y)
    assert {"sgs_clearance_map", "sgs_clearance_query"} <= set(_capi.EXPORTS)
    header = open(__import__("os").path.join(__import__("emu_harness").ROOT, "include", "sage_gs.h")).read()
    for line in ("#define SGS_CLEARANCE_NONE 0xFFFFFFFFu", "#define SGS_CLEARANCE_SRC_MASK8 0", "#define SGS_CLEARANCE_SRC_TOPDOWN 1", "#define SGS_CLEARANCE_UNSEEN_BLOCKS 1u",
                 "#define SGS_CLEARANCE_NEGATE 1u", "#define SGS_CLEARANCE_FLIP_X 2u", "#define SGS_CLEARANCE_FLIP_Y 4u", "#define SGS_VERSION 114"):
        assert line in header, line


def test_python_inflation_limit_and_loader(tmp_path):
    """sage_gs.clearance's host side: inflation_limit against the restatement's, and what the loader refuses."""
    from sage_gs import clearance
    for r in (0.0, 0.05, 0.1, 0.12, 0.15, 0.2, 0.25, 0.3, 0.5, 1.0):
        for s in (0.05, 0.1, 0.025):
            assert clearance.inflation_limit(r, s) == ref.inflation_limit(r, s), (r, s)
    assert clearance.inflation_limit(0.15, 0.05) == 8 and clearance.inflation_limit(-1.0, 0.05) == -1
    for bad in ((0.1, 0.0), (0.1, float("nan")), (float("nan"), 0.05), (1e9, 0.05)):
        with pytest.raises(ValueError):
            clearance.inflation_limit(*bad)
    empty = tmp_path / "empty.json"
    empty.write_text("[]")
    with pytest.raises(ValueError):
        clearance.load_semantic_map(empty)
    with pytest.raises(OSError):
        clearance.load_semantic_map(tmp_path / "missing.json")
