"""The visible-object table (sgs_object_table, csrc/sgs_objects.h) under the wave64 emulator: the kernels' own source, on the CPU, through
the C ABI.  Every picture of tests/object_cases.py against the NumPy restatement (tests/object_table_ref.py, itself held to a Python loop
by test_object_table_ref.py), every field exactly; frames rendered by sgs_render_mesh_ids; batches with a padded stride; the refusals,
misaligned buffers among them; and the split of a call into launches of SGS_OBJ_MAX_FRAMES frames, on a build whose constant is 4."""
import pytest

import emu_harness
import mesh_id_cases as ic
import object_cases as oc
from sage_gs import _capi


SPLIT_CHUNK = 4


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(the emulator library, a build of a copy of csrc/ whose SGS_OBJ_MAX_FRAMES is 4), compiled side by side."""
    path, proc = emu_harness.start_emu_copy(tmp_path_factory.mktemp("object_split"), {"sgs_objects.h": [oc.chunk_edit(SPLIT_CHUNK)]})
    main = emu_harness.build_emu()
    assert proc.wait() == 0, "the copy with launches of 4 frames does not compile"
    return main, path


@pytest.fixture(scope="module")
def lib(libs):
    return _capi.Lib(libs[0])


@pytest.fixture(scope="module")
def drv(lib):
    d = oc.AbiObjects(lib)
    yield d
    d.close()


@pytest.fixture(scope="module")
def split_drv(libs):
    d = oc.AbiObjects(_capi.Lib(libs[1]))
    yield d
    d.close()


@pytest.mark.parametrize("make", oc.SMALL + oc.PATHS + oc.LARGE, ids=lambda m: m.__name__)
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


def test_misaligned_buffers_are_refused(drv):
    oc.check_misaligned(drv)


def test_split_launch_with_chunks_of_4_frames(split_drv):
    """sgs_object_table cuts n_frames into launches of SGS_OBJ_MAX_FRAMES (gridDim.y): with the constant at 4, 11 one-pixel frames
    take two full launches and a short one; then the batches of 1, 3 and 9 frames, the last of which is cut 4 + 4 + 1."""
    assert oc.check_split(split_drv, SPLIT_CHUNK) == 2 * SPLIT_CHUNK + 3
    oc.check_batches(split_drv)


def test_binding_mirrors_the_row():
    import ctypes as C
    import object_table_ref as ref
    assert _capi.OBJECT_ROW_DTYPE == ref.ROW_DTYPE and C.sizeof(_capi.SgsObjectRow) == 40 and C.alignment(_capi.SgsObjectRow) == 8
    assert [(n, _capi.OBJECT_ROW_DTYPE.fields[n][1]) for n in ref.FIELDS] == [(n, getattr(_capi.SgsObjectRow, n).offset) for n, _ in _capi.SgsObjectRow._fields_]
    assert "sgs_object_table" in _capi.EXPORTS
