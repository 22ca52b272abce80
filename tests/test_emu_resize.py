"""The frame resize (sgs_resize, csrc/sgs_resize.h) under the wave64 emulator: the kernels' own source, on the CPU, through the C ABI.

Every shape pair of resize_cases.SHAPES with every picture through both filters and both formats against the NumPy restatement
(tests/resize_ref.py, itself held to PIL.Image.resize by test_resize_ref.py): bicubic bit-equal, linear RGB8 bit-equal, linear F32
within a derived bound; the resized frame through sgs_pack_rgba8 and sgs_encode_png; batches with padded strides; the table cache;
the refusals."""
import numpy as np
import pytest

import emu_harness
import png_cases
import resize_cases as rc
import resize_ref as ref
from sage_gs import _capi


@pytest.fixture(scope="module")
def drv():
    d = rc.AbiResize(_capi.Lib(emu_harness.build_emu()))
    yield d
    d.close()


@pytest.mark.parametrize("shape", rc.SHAPES, ids=rc.shape_id)
def test_shape_pairs(drv, shape):
    rc.check_shape(drv, shape)


@pytest.mark.parametrize("shape", [rc.SHAPES[0], rc.SHAPES[2], rc.SHAPES[6]], ids=rc.shape_id)
def test_resized_frames_pack_and_encode_to_the_resampled_levels(drv, shape):
    png = png_cases.AbiPng(drv.lib, drv.ctx)
    rc.check_downstream(drv, png, shape)


def test_batches_and_padded_strides(drv):
    rc.check_batch_and_strides(drv)


def test_a_second_call_with_other_sizes_on_the_same_context():
    """The table cache: sizes seen in turn, and again, on one context of its own; the same axis pair in the other format."""
    d = rc.AbiResize(_capi.Lib(emu_harness.build_emu()))
    try:
        for shape in (rc.SHAPES[2], rc.SHAPES[0], rc.SHAPES[2], rc.SHAPES[3], rc.SHAPES[0]):
            W, H, w, h = shape
            pic = rc.colour_pictures(W, H)["random"]
            want, _ = ref.resize_rgb8(pic, w, h)
            assert np.array_equal(d.one(pic, (w, h)), want), rc.shape_id(shape)
            dep = rc.depth_pictures(W, H)["plateaus"][0]
            assert np.array_equal(d.one(dep, (w, h), "f32"), ref.bicubic_f32(dep, w, h)), rc.shape_id(shape)
    finally:
        d.close()


def test_refusals(drv):
    rc.check_refusals(drv)
