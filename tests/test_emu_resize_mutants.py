"""Seeded faults in the frame resize (csrc/sgs_resize.h, and the pass selection in csrc/sgs_api.hip), under the wave64 emulator: each
is made in a copy of csrc/, compiled, and must be caught by resize_cases.check_shape — by the assertion named for it."""
import re

import pytest

import emu_harness
import resize_cases as rc
from sage_gs import _capi

HALF = "int r = 1 << (SGS_RESIZE_BITS - 1), g = r, b = r;"
MID = "else J.mid[f * J.H * J.w + i] = R | (G << 8) | (B << 16);"
FLOOR = "else J.mid[f * J.H * J.w + i] = resize_clamp8(r - (1 << (SGS_RESIZE_BITS - 1))) | (resize_clamp8(g - (1 << (SGS_RESIZE_BITS - 1))) << 8) | " \
        "(resize_clamp8(b - (1 << (SGS_RESIZE_BITS - 1))) << 16);"
HALF_AFTER = ("\n        for (int j = 0; j < n; ++j) {", "\n        if (J.v_from_src) {")      # the line stands twice in the file: what follows each
H, API = "sgs_resize.h", "sgs_api.hip"
MUTANTS = {          # name: {file of csrc/: [(anchor, replacement)]}
    "rounding_term_dropped": {H: [(HALF + after, "int r = 0, g = r, b = r;" + after) for after in HALF_AFTER]},
    "window_starts_one_late": {H: [("int lo = (int)(c - support + 0.5);", "int lo = (int)(c - support + 0.5) + 1;")]},
    "weights_not_normalised": {H: [("if (ww != 0.0) kk[j] = kk[j] / ww;", "if (ww != 0.0) kk[j] = kk[j];")]},
    "vertical_pass_fed_unrounded_sums": {H: [(MID, FLOOR)]},
    "levels_by_truncation": {H: [("return (int)(unsigned)(c * 255.0f + 0.5f);", "return (int)(unsigned)(c * 255.0f);")]},
    "skipped_pass_run_with_identity_weights": {API: [("const bool do_h = bicubic && J.W != J.w, do_v = bicubic && J.H != J.h;",
                                                      "const bool do_h = bicubic, do_v = bicubic;")]},
}
# The first failing assertion of resize_cases.check_shape on each mutant, with its figures (the bytes are deterministic).  Dropped
# rounding and floored intermediates read one level low; un-normalised weights of a cut window overflow on the brightest constant; with
# identity weights a skipped pass is the same picture in RGB8 and for finite depth (the weights are exactly 0, 1, 0, 0), and differs only
# where a zero weight meets the NaN: 12 more pixels of the picture with a single NaN.
CAUGHT_BY = {
    "rounding_term_dropped": r"37x23_to_13x7 thresholds: bicubic rgb8 differs from the restatement at 243 of 273 values \(first: 160\.000 for level 161\)",
    "window_starts_one_late": r"37x23_to_13x7 thresholds: bicubic rgb8 differs from the restatement at 85 of 273 values",
    "weights_not_normalised": r"37x23_to_13x7 constant_255: bicubic rgb8 differs from the restatement at 273 of 273 values",
    "vertical_pass_fed_unrounded_sums": r"37x23_to_13x7 thresholds: bicubic rgb8 differs from the restatement at 141 of 273 values \(first: 83\.000 for level 84\)",
    "levels_by_truncation": r"37x23_to_13x7 thresholds: bicubic rgb8 differs from the restatement at 111 of 273 values \(first: 147\.000 for level 148\)",
    "skipped_pass_run_with_identity_weights": r"64x48_to_64x20 single_nan: bicubic f32 differs from the restatement at 12 of 1276 values",
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    return emu_harness.build_mutants(tmp_path_factory.mktemp("resize_mutants"), MUTANTS, "libsage_gs_resize_mutant.so")


def _checks(d):
    for shape in rc.SHAPES:
        rc.check_shape(d, shape)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_resize_mutant_is_caught(mutant_libs, name):
    d = rc.AbiResize(_capi.Lib(mutant_libs[name]))
    caught = None
    try:
        _checks(d)
    except AssertionError as e:
        caught = e
    finally:
        d.close()
    assert caught is not None, f"{name}: the resize's checks pass on this mutant"
    print(f"[resize mutant] {name}: caught: {str(caught)[:200]}")
    assert re.search(CAUGHT_BY[name], str(caught)), f"{name}: failed on another assertion: {str(caught)[:300]}"


def test_the_unmutated_library_passes_the_mutants_checks():
    d = rc.AbiResize(_capi.Lib(emu_harness.build_emu()))
    try:
        _checks(d)
    finally:
        d.close()
