"""The visible-object table (sgs_object_table, csrc/sgs_objects.h) under the wave64 emulator: the kernels' own source, on the CPU, through
the C ABI.  Every picture of tests/object_cases.py against the NumPy restatement (tests/object_table_ref.py, itself held to a Python loop
by test_object_table_ref.py), every field exactly; frames rendered by sgs_render_mesh_ids; batches with a padded stride; the refusals."""
import pytest

import emu_harness
import mesh_id_cases as ic
import object_cases as oc
from sage_gs import _capi


@pytest.fixture(scope="module")
def lib():
    return _capi.Lib(oc.emu_lib_path())


@pytest.fixture(scope="module")
def drv(lib):
    d = oc.AbiObjects(lib)
    yield d
    d.close()


@pytest.mark.parametrize("make", oc.SMALL + oc.LARGE, ids=lambda m: m.__name__)
def test_pictures(drv, make):
    oc.check_pictures(drv, [make])


def test_rendered_room_frames(drv, lib):
    e = ic.EmuIds(lib)
    try:
        oc.check_rendered(drv, e)
    finally:
        e.close()


def test_batches_and_padded_strides(drv):
    oc.check_batches(drv)


def test_refusals(drv):
    oc.check_refusals(drv)


def test_binding_mirrors_the_row():
    import ctypes as C
    import object_table_ref as ref
    assert _capi.OBJECT_ROW_DTYPE == ref.ROW_DTYPE and C.sizeof(_capi.SgsObjectRow) == 40 and C.alignment(_capi.SgsObjectRow) == 8
    assert [(n, _capi.OBJECT_ROW_DTYPE.fields[n][1]) for n in ref.FIELDS] == [(n, getattr(_capi.SgsObjectRow, n).offset) for n, _ in _capi.SgsObjectRow._fields_]
    assert "sgs_object_table" in _capi.EXPORTS
