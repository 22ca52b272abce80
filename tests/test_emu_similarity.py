"""The image similarity (sgs_image_similarity, csrc/sgs_similarity.h) under the wave64 emulator: the kernels' own source, on the CPU,
through the C ABI.  Every picture of every shape of tests/similarity_cases.py against the NumPy restatement (tests/similarity_ref.py,
itself held to a Python-integer loop by test_similarity_ref.py), every field exactly; batches with padded strides against per-frame
and shared targets; the refusals, misaligned buffers among them."""
import ctypes as C

import pytest

import emu_harness
import similarity_cases as sc
import similarity_ref as ref
from sage_gs import _capi


@pytest.fixture(scope="module")
def drv():
    d = sc.AbiSimilarity(_capi.Lib(emu_harness.build_emu()))
    yield d
    d.close()


@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_pictures(drv, shape):
    sc.check_shape(drv, shape)


def test_the_emulated_levels_are_the_restatements(drv):
    for shape in (sc.SHAPES[0], sc.SHAPES[3]):
        wild = sc.pictures_of(shape)["out_of_range"][0]
        assert (drv.pack(wild) == ref.levels(wild)).all()


def test_batches_and_padded_strides(drv):
    sc.check_batches(drv)


def test_refusals(drv):
    sc.check_refusals(drv)


def test_binding_mirrors_the_row():
    assert _capi.SIMILARITY_ROW_DTYPE == ref.ROW_DTYPE and C.sizeof(_capi.SgsSimilarityRow) == 64 and C.alignment(_capi.SgsSimilarityRow) == 8
    assert [(n, _capi.SIMILARITY_ROW_DTYPE.fields[n][1]) for n in ref.FIELDS] == [(n, getattr(_capi.SgsSimilarityRow, n).offset) for n, _ in _capi.SgsSimilarityRow._fields_]
    assert _capi.SIMILARITY_DTYPE.names[:4] == ref.FIELDS and _capi.SIMILARITY_DTYPE.names[4:] == ("ssim", "ssim_rgb", "mse", "psnr")
    assert "sgs_image_similarity" in _capi.EXPORTS and _capi.SIMILARITY_Q_BITS == ref.Q_BITS
