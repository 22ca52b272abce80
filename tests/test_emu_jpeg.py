"""The JPEG encoder (sgs_encode_jpeg, csrc/sgs_jpeg.h) under the wave64 emulator: the kernels' own source, on the CPU.

1 coefficients against the fp64 reference, 2 structure, 3 interoperability with PIL, 4 fidelity against PIL's own files, 5 issue
independence, 6 capacity, 7 refusals, 8 seeded faults (mutants) that checks 1-2 must catch.  Figures of test 4 are printed (pytest -s)
and listed in DESIGN.md §11."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_harness
import jpeg_cases as jc
import jpeg_ref
from sage_gs import _capi

JPEG_H = os.path.join(emu_harness.PKG, "csrc", "sgs_jpeg.h")


@pytest.fixture(scope="module")
def drv():
    d = jc.AbiJpeg(_capi.Lib(emu_harness.build_emu()))
    yield d
    d.close()


IMAGES = jc.image_set()


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_files_against_reference_and_pil(drv, name):
    """Tests 1-4 for every quality and both subsamplings (no byte past the reported size: the sentinel check of encode_one)."""
    img = IMAGES[name]
    for q in jc.QUALITIES:
        for sub in jc.SUBSAMPLINGS:
            jc.check_file(drv.encode_one(img, q, sub), img, q, sub, label=name)


def test_exact_ties_round_away_from_zero(drv):
    jc.check_exact_ties(drv.encode_one)


def test_parser_reads_a_pil_file_and_refuses_damage(drv):
    """The checker's own sensitivity: parse_jpeg decodes PIL's file to PIL's tables and the reference's neighbourhood, and raises on
    a wrong RSTn index, a dropped byte, a wrong size field and a bad code."""
    img = jc.gradient_noise(32, 48, 3)          # whole MCUs: libjpeg fills the blocks beyond a partial MCU's edge in its own way
    u8 = jc.levels_of(img)
    p = jpeg_ref.parse_jpeg(jc.pil_encode(u8, 75, "4:2:0"))
    assert (p["width"], p["height"]) == (48, 32) and (p["qtables"][0] == jpeg_ref.ijg_table(jpeg_ref.Q_LUM, 75)).all()
    ref = jpeg_ref.reference_coefficients(u8, 75, "4:2:0")
    assert max(int(np.abs(c - r[1]).max()) for c, r in zip(p["coefficients"], ref)) <= 2       # (libjpeg rounds thrice: close, not equal)
    good = drv.encode_one(jc.gradient_noise(48, 64, 4), 75, "4:2:0")       # 12 MCUs: two restart intervals
    jpeg_ref.parse_jpeg(good)
    at = good.index(b"\xff\xd0")
    for bad in (good[:at + 1] + b"\xd1" + good[at + 2:], good[:at - 1] + good[at:], good[:-2], good[:4] + b"\x00\x11" + good[6:],
                good[:at - 3] + b"\x00\x00" + good[at - 1:]):
        with pytest.raises(jpeg_ref.JpegError):
            jpeg_ref.parse_jpeg(bad)


def test_issue_independence(drv):
    """Test 5: a batch of 5 different frames yields, frame by frame, the bytes each yields alone; two calls yield the same bytes."""
    frames = np.stack([jc.gradient_noise(45, 70, seed=s) * (0.5 + 0.1 * s) for s in range(5)])
    for q, sub in ((95, "4:2:0"), (75, "4:4:4")):
        batch = drv.encode(frames, q, sub)
        assert batch["rc"] == 0
        jc.check_nothing_written_beyond(batch)
        again = drv.encode(frames, q, sub)
        assert again["files"] == batch["files"]
        assert len(set(batch["files"])) == 5
        for i in range(5):
            assert drv.encode_one(frames[i], q, sub) == batch["files"][i], f"frame {i} depends on the batch it is issued in"
        pair = drv.encode(frames[[3, 1]], q, sub)
        assert pair["files"] == [batch["files"][3], batch["files"][1]]


def test_capacity(drv):
    """Test 6: one byte short — nothing beyond the capacity is written, the sizes are reported, the status says overflow; a retry with
    sgs_jpeg_bound bytes per frame succeeds."""
    frames = np.stack([jc.gradient_noise(40, 56, seed=s) for s in range(3)])
    full = drv.encode(frames, 95, "4:2:0")
    assert full["rc"] == 0
    need = full["needed"]
    short = drv.encode(frames, 95, "4:2:0", capacity=need - 1)
    assert short["rc"] == -4 and short["needed"] == need, (short["rc"], short["needed"])        # SGS_ERR_OVERFLOW
    assert b"out_capacity" in drv.lib.sgs_last_error(drv.ctx)
    assert (short["sizes"] == full["sizes"]).all() and (short["offsets"] == full["offsets"]).all()
    jc.check_nothing_written_beyond(short)
    assert (short["buffer"][need - 1:] == jc.SENTINEL).all()
    # the frames that do fit are complete files; the one that does not is not started
    cut = int(full["offsets"][2])
    assert bytes(short["buffer"][:cut]) == bytes(full["buffer"][:cut]) and (short["buffer"][cut:] == jc.SENTINEL).all()
    none = drv.encode(frames, 95, "4:2:0", capacity=0)
    assert none["rc"] == -4 and (none["buffer"] == jc.SENTINEL).all() and (none["sizes"] == full["sizes"]).all()
    retry = drv.encode(frames, 95, "4:2:0", capacity=3 * drv.bound(56, 40, 95, "4:2:0"))
    assert retry["rc"] == 0 and retry["files"] == full["files"]
    exact = drv.encode(frames, 95, "4:2:0", capacity=need)
    assert exact["rc"] == 0 and exact["files"] == full["files"]


def test_bound_covers_the_worst_file_we_can_make(drv):
    """sgs_jpeg_bound is derived, not measured; the densest pictures of the set stay far below it."""
    img = jc.checkerboard(24, 40)
    noise = np.random.RandomState(9).rand(24, 40, 3).astype(np.float32)
    for pic in (img, noise):
        for sub in jc.SUBSAMPLINGS:
            assert len(drv.encode_one(pic, 100, sub)) <= drv.bound(40, 24, 100, sub)
    assert drv.bound(1, 1, 95, "4:2:0") == 629 + 2 * 9948 + 2


def test_refusals(drv):
    """Test 7: every invalid argument returns SGS_ERR_INVALID with a message."""
    lib, ctx = drv.lib, drv.ctx
    f = np.zeros((2, 8, 8, 3), np.float32)
    out = np.zeros(1 << 16, np.uint8); offs = np.zeros(2, np.int64); sizes = np.zeros(2, np.int64)

    def call(w=8, h=8, n=2, quality=95, sub=_capi.JPEG_420, rgb=f.ctypes.data, o=out.ctypes.data, a=offs.ctypes.data, s=sizes.ctypes.data,
             params=True, cap=out.size):
        p = _capi.SgsJpegParams(quality, sub, 0, 0)
        return lib.sgs_encode_jpeg(ctx, rgb, w, h, n, 192, C.byref(p) if params else None, o, cap, a, s, None)

    assert call() == 0
    # (what the message must name, the argument): each refusal sets a message of its own, not the previous one's
    bad = [(b"quality 0 ", dict(quality=0)), (b"quality 101 ", dict(quality=101)), (b"subsampling 2 ", dict(sub=2)), (b"subsampling -1 ", dict(sub=-1)),
           (b"0 x 8", dict(w=0)), (b"8 x 0", dict(h=0)), (b"65536 x 8", dict(w=65536)), (b"8 x 65536", dict(h=65536)), (b"n_frames = -1", dict(n=-1)),
           (b"null rgb", dict(rgb=None)), (b"null out", dict(o=None)), (b"null out_offsets", dict(a=None)), (b"null out_sizes", dict(s=None)),
           (b"params is NULL", dict(params=False)), (b"capacity -1", dict(cap=-1))]
    for word, kw in bad:
        assert call(**kw) == -1, word
        assert word in lib.sgs_last_error(ctx), (word, lib.sgs_last_error(ctx))
    # a call that encodes nothing clears the status of the one before it
    assert call(cap=10) == 0 and lib.sgs_jpeg_status(ctx, None) == -4
    assert call(n=0) == 0 and lib.sgs_jpeg_status(ctx, None) == 0
    p = _capi.SgsJpegParams(0, 0, 0, 0)
    assert lib.sgs_jpeg_bound(8, 8, C.byref(p)) == -1 and lib.sgs_jpeg_bound(8, 8, None) == -1
    d = _capi.SgsJpegParams()
    lib.sgs_jpeg_params_default(C.byref(d))
    assert (d.quality, d.subsampling, d.flags) == (95, _capi.JPEG_420, 0)
    assert lib.sgs_jpeg_bound(0, 8, C.byref(d)) == -1 and lib.sgs_jpeg_bound(8, 65536, C.byref(d)) == -1


# ---- test 8: seeded faults ------------------------------------------------------------------------------------------------------------
H = "sgs_jpeg.h"
MUTANTS = {          # name: {file of csrc/: [(anchor, replacement)]}
    "halves_toward_zero": {H: [("(int)roundf(f / s_q[tq][lane])", "(int)(f / s_q[tq][lane] < 0 ? ceilf(f / s_q[tq][lane] - 0.5f) : floorf(f / s_q[tq][lane] + 0.5f) - (floorf(f / s_q[tq][lane] + 0.5f) - f / s_q[tq][lane] == 0.5f ? 1.0f : 0.0f))")]},
    "luminance_table_off_by_one": {H: [("T.q[0][k] = (float)quant_step(kQLum[n], quality);", "T.q[0][k] = (float)(quant_step(kQLum[n], quality) + (k == 5 ? 1 : 0));")]},
    "dc_predictor_not_reset": {H: [("int pred_y = 0, pred_cb = 0, pred_cr = 0;", "int pred_y = it ? 3 : 0, pred_cb = 0, pred_cr = 0;")]},
    "stuffing_skipped": {H: [("if (ff) dst[at + 1] = 0;", "if (ff) dst[at + 1] = 0x5A;")]},
    "zero_padding": {H: [("min(py, J.height - 1) * J.width + min(px, J.width - 1));", "min(py, J.height - 1) * J.width + min(px, J.width - 1));\n            const bool outside = px >= J.width || py >= J.height;"),
                         ("const float r = jpeg_level(p[0]), g = jpeg_level(p[1]), bl = jpeg_level(p[2]);", "const float r = outside ? 0.f : jpeg_level(p[0]), g = outside ? 0.f : jpeg_level(p[1]), bl = outside ? 0.f : jpeg_level(p[2]);")]},
    "cb_cr_swapped": {H: [("s = comp == 1 ? w * fmaf(-0.168736f, srg, 0.5f * sbg)", "s = comp == 2 ? w * fmaf(-0.168736f, srg, 0.5f * sbg)")]},
}
CAUGHT_BY = {
    "halves_toward_zero": r"exact tie",
    "luminance_table_off_by_one": r"coefficients differ outside the tie window|not the IJG table",
    "dc_predictor_not_reset": r"coefficients differ outside the tie window",
    "stuffing_skipped": r"marker 0x5a inside the scan",
    "zero_padding": r"coefficients differ outside the tie window",
    "cb_cr_swapped": r"coefficients differ outside the tie window",
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    return emu_harness.build_mutants(tmp_path_factory.mktemp("jpeg_mutants"), MUTANTS, "libsage_gs_jpeg_mutant.so")


def _checks_1_and_2(d):
    """Tests 1-2 (coefficients incl. the exact ties, structure) on the pictures that exercise every fault's territory."""
    jc.check_exact_ties(d.encode_one)
    for name in ("gradient_250x187", "flat_regions", "checkerboard_19x13"):
        img = IMAGES[name]
        u8 = jc.levels_of(img)
        for q, sub in ((50, "4:2:0"), (95, "4:4:4"), (100, "4:2:0")):
            data = d.encode_one(img, q, sub)
            parsed, _, _, _ = jc.check_coefficients(data, u8, q, sub)
            jc.check_structure(data, parsed, u8.shape[1], u8.shape[0], q, sub)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_jpeg_mutant_is_caught(mutant_libs, name):
    d = jc.AbiJpeg(_capi.Lib(mutant_libs[name]))
    caught = None
    try:
        _checks_1_and_2(d)
    except (AssertionError, jpeg_ref.JpegError) as e:
        caught = e
    finally:
        d.close()
    assert caught is not None, f"{name}: checks 1-2 pass on this mutant"
    assert re.search(CAUGHT_BY[name], f"{type(caught).__name__}: {caught}"), f"{name}: failed on another assertion: {str(caught)[:300]}"
    print(f"[jpeg mutant] {name}: caught: {str(caught)[:200]}")


def test_the_unmutated_library_passes_the_mutants_checks(drv):
    _checks_1_and_2(drv)


# ---- test 9: padded strides, long scans -----------------------------------------------------------------------------------------------
def test_padded_stride_and_long_scan(drv):
    """Frames a frame plus 37 floats apart (NaN and 1e30 between them) give the packed batch's files; a batch of 20 frames of 128x112
    at 4:4:4 has 280 restart intervals, so that k_jpeg_scan's 256 threads take two each: offsets and sizes end to end, nothing written
    beyond, every frame the bytes it gets alone."""
    frames = np.stack([jc.gradient_noise(112, 128, seed=s) * (0.6 + 0.02 * s) for s in range(20)])
    batch = jc.check_stride_and_long_scan(drv.encode, frames, 256, 14, quality=75, subsampling="4:4:4")
    assert len(set(batch["files"])) == 20
    for i in (0, 9, 10, 19):
        assert drv.encode_one(frames[i], 75, "4:4:4") == batch["files"][i], f"frame {i} depends on the batch it is issued in"
    jc.check_file(batch["files"][19], frames[19], 75, "4:4:4", label="long_scan_frame_19")
    jc.check_stride_and_long_scan(drv.encode, frames[:3], 0, 4, quality=95, subsampling="4:2:0")
