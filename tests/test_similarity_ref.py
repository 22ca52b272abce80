"""The NumPy restatement of the image similarity (tests/similarity_ref.py) held to a Python-integer loop written from the definition,
window by window; the known answers; and the one tolerance of the feature: the score against an fp64 SSIM with the float Gaussian."""
import numpy as np
import pytest

import similarity_cases as sc
import similarity_ref as ref

# The integer window (taps rounded to 1/2048, the centre lowered by 1) against Wang et al.'s float Gaussian, both on the same levels:
# the worst |score - ssim_float| over every picture of every shape of similarity_cases is 5.3e-4 (11x11 noise_pair: a single
# window per channel, nothing averages out), rounded up
# to one significant digit.  scripts/similarity_bench.py uses the same bound.
WINDOW_QUANTISATION_BOUND = 6e-4


def _small_pairs():
    rs = np.random.RandomState(2)
    out = []
    for W, H in ((11, 11), (13, 12), (12, 11), (11, 12), (13, 11)):
        a, b = rs.randint(0, 256, (H, W)), rs.randint(0, 256, (H, W))
        out += [(a, b), (a, a), (a, 255 - a), (np.zeros_like(a), np.full_like(a, 255)), (rs.randint(0, 2, (H, W)) * 255, rs.randint(0, 2, (H, W)) * 255)]
    return out


def test_restatement_equals_the_python_integer_loop():
    for x, y in _small_pairs():
        want = np.array(ref.q_loop(x.tolist(), y.tolist()), np.int64)
        got = ref.window_q(x, y)
        assert got.shape == want.shape == (x.shape[0] - 10, x.shape[1] - 10) and np.array_equal(got, want)
        frame = np.stack([x, y, x], -1).astype(np.uint8), np.stack([y, y, x], -1).astype(np.uint8)
        r = ref.row(*frame)
        assert r["ssim_q"].tolist() == [int(want.sum()), int(np.array(ref.q_loop(y.tolist(), y.tolist())).sum()), int(np.array(ref.q_loop(x.tolist(), x.tolist())).sum())]
        assert r["sse"].tolist() == [int(((x - y) ** 2).sum()), 0, 0] and r["n_windows"] == want.size and r["n_pixels"] == x.size


def test_taps_are_the_scaled_gaussian():
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    want = np.round(2048 * g / g.sum()).astype(int)
    assert want.sum() == 2049
    want[5] -= 1
    assert want.tolist() == list(ref.TAPS) and sum(ref.TAPS) == 2048


@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_known_answers(shape):
    W, H = shape
    nw = (W - 10) * (H - 10)
    pics = sc.pictures_of(shape)
    sc.check_picture_properties(shape)
    a = pics["identical"][1]
    assert np.array_equal(ref.window_q(a[..., 0], a[..., 0]), np.full((H - 10, W - 10), ref.ONE))
    # constant 0 against constant 255: A = 0, every second moment of x is 0, B = 255 T, T Cyy = B^2: n2 = d2 = c2, so s = c1 / (B^2 + c1)
    B = 255 * ref.T
    q = int(np.floor(ref.C1 / (B * B + ref.C1) * 2.0 ** 30 + 0.5))
    z = ref.window_q(np.zeros((H, W), int), np.full((H, W), 255))
    assert (z == q).all() and q == (2 * ref.C1 * ref.ONE + (B * B + ref.C1)) // (2 * (B * B + ref.C1)) == 107363
    r = ref.row(ref.levels(pics["zero_against_255"][0]), pics["zero_against_255"][1])
    assert r["ssim_q"].tolist() == [q * nw] * 3 and r["sse"].tolist() == [65025 * W * H] * 3
    inv = ref.row(ref.levels(pics["inverse"][0]), pics["inverse"][1])
    assert (inv["ssim_q"] < 0).all() and ref.score(inv) < -0.9


def test_int64_bounds_hold_at_the_extremes():
    """The largest terms: all 255 against all 255 (A^2 = B^2 = (255 T)^2), and the checkerboard against its inverse (the most negative n2)."""
    hi = np.full((11, 11), 255)
    assert ref.window_q(hi, hi).tolist() == [[ref.ONE]]
    A = 255 * ref.T
    assert 2 * A * A + ref.C1 < 2 ** 63 and 2 * (ref.T * 255 * 255 * ref.T) + ref.C2 < 2 ** 63
    yy, xx = np.mgrid[0:11, 0:11]
    ch = 255 * ((xx + yy) & 1)
    assert ref.window_q(ch, 255 - ch)[0, 0] < -(ref.ONE * 9 // 10)


def test_score_is_within_the_window_quantisation_bound_of_float_ssim():
    worst, where = 0.0, None
    for shape in sc.SHAPES:
        for name, (frame, target) in sc.pictures_of(shape).items():
            lv = ref.levels(frame)
            d = abs(ref.score(ref.row(lv, target)) - ref.ssim_float(lv, target))
            if d > worst:
                worst, where = d, f"{sc.shape_id(shape)} {name}"
    print(f"[similarity] worst |score - float-Gaussian SSIM| = {worst:.3e} at {where}")
    assert worst <= WINDOW_QUANTISATION_BOUND, (worst, where)
