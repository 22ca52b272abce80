"""The geodesic field and its paths (sgs_geodesic_field, sgs_geodesic_path; csrc/sgs_geodesic.h) under the wave64 emulator: the kernels'
own source, on the CPU, through the C ABI.  Every picture of tests/geodesic_cases.py against the integer restatement
(tests/geodesic_ref.py, itself held to a brute-force loop, to SciPy and to the reference's answers by test_geodesic_ref.py), every cell
exactly; the tile edge T is read from the binding.  The emulator cannot see a race between workgroups: that a round has none is argued
in DESIGN.md §18, not tested here."""
import ctypes as C
import os

import pytest

import emu_harness
import geodesic_cases as gc
import geodesic_ref as ref
from sage_gs import _capi


@pytest.fixture(scope="module")
def lib():
    return _capi.Lib(emu_harness.build_emu())


@pytest.fixture(scope="module")
def drv(lib):
    d = gc.AbiGeodesic(lib)
    yield d
    d.close()


def test_sizes(drv):
    assert drv.T in (32, 64)
    gc.check_sizes(drv)


def test_pictures(drv):
    gc.check_picture_properties(drv.T)
    gc.check_pictures(drv, gc.pictures(drv.T))


def test_serpentine_needs_continue(drv):
    gc.check_serpentine_needs_continue(drv)


def test_schedule_independence(drv):
    gc.check_schedule_independence(drv)


def test_batches_and_padded_strides(drv):
    gc.check_batches(drv)


def test_both_sources(drv):
    gc.check_sources(drv)


def test_paths(drv):
    gc.check_paths(drv)


def test_the_references_own_answers(drv):
    gc.check_golden(drv)


def test_refusals(drv):
    gc.check_refusals(drv)


def test_binding_mirrors_the_struct(lib):
    P = _capi.SgsGeodesicParams
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == [
        ("nx", 0, 4), ("ny", 4, 4), ("source", 8, 4), ("max_d2", 12, 4), ("flags", 16, 4), ("reserved", 20, 4)]
    assert C.sizeof(P) == 24
    assert (_capi.GEODESIC_NONE, _capi.GEODESIC_SRC_MASK8, _capi.GEODESIC_SRC_D2, _capi.GEODESIC_CONTINUE) == (ref.NONE, ref.SRC_MASK8, ref.SRC_D2, ref.CONTINUE)
    assert (_capi.GEODESIC_PATH_OK, _capi.GEODESIC_PATH_UNREACHABLE, _capi.GEODESIC_PATH_TRUNCATED, _capi.GEODESIC_PATH_INVALID, _capi.GEODESIC_PATH_NOT_FINAL) == \
        (ref.PATH_OK, ref.PATH_UNREACHABLE, ref.PATH_TRUNCATED, ref.PATH_INVALID, ref.PATH_NOT_FINAL)
    assert {"sgs_geodesic_tile", "sgs_geodesic_state_words", "sgs_geodesic_field", "sgs_geodesic_path"} <= set(_capi.EXPORTS)
    header = open(os.path.join(__import__("emu_harness").ROOT, "include", "sage_gs.h")).read()
    for line in ("#define SGS_GEODESIC_NONE 0xFFFFFFFFu", "#define SGS_GEODESIC_SRC_MASK8 0", "#define SGS_GEODESIC_SRC_D2 1", "#define SGS_GEODESIC_CONTINUE 1u",
                 f"#define SGS_GEODESIC_MAX_N {_capi.GEODESIC_MAX_N}", f"#define SGS_GEODESIC_MAX_FIELDS {_capi.GEODESIC_MAX_FIELDS}",
                 f"#define SGS_GEODESIC_PATH_MAX_FIELDS {_capi.GEODESIC_PATH_MAX_FIELDS}", "#define SGS_VERSION 114"):
        assert line in header, line
    assert lib.sgs_geodesic_state_words(65, 33, 3) == 3 * (2 + -(-65 // lib.sgs_geodesic_tile()) * -(-33 // lib.sgs_geodesic_tile()))
