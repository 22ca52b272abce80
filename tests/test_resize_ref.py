"""The restatement of the resize's value rule (tests/resize_ref.py) against PIL.Image.resize, on the CPU: uint8 RGB and mode F
bit-equal at every shape pair the library is tested at; the linear filter's 2:1 identity; the k / 255 round trip of all 256 levels."""
import numpy as np
import pytest

import resize_cases as rc
import resize_ref as ref

Image = pytest.importorskip("PIL.Image")


@pytest.mark.parametrize("shape", rc.SHAPES, ids=rc.shape_id)
def test_bicubic_equals_pillow(shape):
    W, H, w, h = shape
    rs = np.random.RandomState(W * 131 + h)
    img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    img[:H // 2] = (img[:H // 2] > 128) * 255              # hard edges: values that leave [0, 255] before the clamp
    want = np.asarray(Image.fromarray(img).resize((w, h)))
    got = ref.bicubic_u8(img, w, h)
    assert want.shape == got.shape and np.array_equal(want, got), f"uint8: {int(np.abs(want.astype(int) - got).max())} levels apart"
    d = (rs.rand(H, W) * 7).astype(np.float32)
    d[::5, ::3] = np.float32(6.5)
    im = Image.fromarray(d)
    assert im.mode == "F"
    want = np.asarray(im.resize((w, h)))
    got = ref.bicubic_f32(d, w, h)
    assert want.dtype == np.float32 and np.array_equal(want.view(np.uint32), got.view(np.uint32)), f"float: {float(np.abs(want - got).max())} apart"


def test_linear_two_to_one_is_the_rounded_mean():
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, (48, 64, 3)).astype(np.int64)
    want = (img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2
    assert np.array_equal(ref.linear_u8(img.astype(np.uint8), 32, 24), want)
    d = rs.rand(48, 64).astype(np.float32)
    mean = (d[0::2, 0::2].astype(np.float64) + d[0::2, 1::2] + d[1::2, 0::2] + d[1::2, 1::2]) / 4
    assert np.abs(ref.linear_f(d, 32, 24, dtype=np.float64) - mean).max() < 1e-12
    # the same size is the picture itself, and an enlargement clamps at the edges
    assert np.array_equal(ref.linear_u8(img.astype(np.uint8), 64, 48), img)
    up = ref.linear_u8(img.astype(np.uint8), 128, 96)
    assert np.array_equal(up[0, 0], img[0, 0]) and np.array_equal(up[-1, -1], img[-1, -1])


def test_levels_round_trip_through_k_over_255():
    """The fp32 nearest k / 255 goes back to k under x * 255 + 0.5: unfused in fp32, and fused (the exact product plus a half, rounded
    once: evaluated here in fp64, where k / 255 * 255 + 0.5 is exact to far below the 2^-15 the argument needs)."""
    k = np.arange(256)
    x = ref.unlevel(k)
    assert x.dtype == np.float32 and np.array_equal(ref.levels(x), k)
    exact = x.astype(np.float64) * 255 + 0.5
    assert np.abs(exact - (k + 0.5)).max() < 2.0 ** -15
    assert np.array_equal(exact.astype(np.float32).astype(np.uint32), k)


def test_float_clip_keeps_nan_and_makes_inf_finite():
    d = np.float32([[np.inf, -np.inf, np.nan, 0.05, 3.0, 7.0]])
    got = ref.clip(d, (0.1, 6.5))
    assert np.isnan(got[0, 2]) and got[0, [0, 1, 3, 4, 5]].tolist() == [6.5, np.float32(0.1), np.float32(0.1), 3.0, 6.5]
    assert np.array_equal(ref.clip(d, None).view(np.uint32), d.view(np.uint32))
