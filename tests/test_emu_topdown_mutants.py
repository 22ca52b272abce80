"""Seeded faults in the top-down seen map (csrc/sgs_topdown.h, and its entry in csrc/sgs_api.hip), under the wave64 emulator: each is
made in a copy of csrc/, compiled, and must be caught by the check named for it, on the assertion written down here.

One fault of the list this file was written to has no counterpart in these kernels: "a run continued across a row end".  A run
carries its key and its length and nothing else — no x, no y, no box — so two neighbouring lanes with one key add the same count
to the same cell whether an image row ends between them or not: k_topdown_map lets such a run continue on purpose, and a kernel
that cut it there would compute the same grid.  What a row end does change is the pixel's position, which the kernel steps along
with the lanes; the fault seeded in its place is that step not wrapping at the end of a row (row_end_not_wrapped: the first frame of
more than one pixel per thread, 67 x 5, shows it; a head contributing 1 leaves the wall's cell with one hit per wave and step, 74 of 4690).  The figures in the patterns follow from the pictures: at max_z the one sample
equal to it moves from binned to out of range; at occ_lo the row of eight cells at h = 0.5 becomes occupied; with u == nx inside, or
(int) taken first, the ten pixels of the outer column are binned or fall in no band; the counters of frames 4 and 8 land on frame 0."""
import re

import pytest

import emu_harness
import topdown_cases as tc
from sage_gs import _capi

H, API = "sgs_topdown.h", "sgs_api.hip"
CHUNK = 4
_pictures = lambda *makers: (lambda d: tc.check_pictures(d, makers))                             # noqa: E731
_NO_REFUSAL = [("if (reinterpret_cast<uintptr_t>(b.at) % 4) SGS_FAIL", "if (false) SGS_FAIL"),
               ('if (reinterpret_cast<uintptr_t>(grid) % 4) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: grid %p', 'if (false) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: grid %p'),
               ("if (reinterpret_cast<uintptr_t>(out) % 8) SGS_FAIL", "if (false) SGS_FAIL")]

# name: ({file of csrc/: [(anchor, replacement)]}, the check that must catch it, what its first failing assertion says)
MUTANTS = {
    "row_end_not_wrapped": ({H: [("if (x >= W) { x -= W; y += 1u; }", "")]}, _pictures(tc.sizes),
                            r"sizes\[4\] 67x5: cell \(41, 22\) occupied is 3, the restatement has 0"),
    "run_head_contributes_1": ({H: [("const unsigned len = (unsigned)(next - lane);", "const unsigned len = 1u;")]}, _pictures(tc.wall),
                               r"wall\[0\] 67x70: cell \(2, 1\) free is 74, the restatement has 4690"),
    "no_slot_path_dropped": ({H: [("else atomicAdd(&J.grid[v], len);", "else {}")]}, _pictures(tc.own_cell),
                             r"own_cell\[0\] 97x89: cell \(\d+, \d+\) \w+ is 0, the restatement has 1"),
    "slot_flush_dropped": ({H: [("if (s_n[s]) atomicAdd(&J.grid[s_key[s] - 1u], s_n[s]);", "if (false) atomicAdd(&J.grid[s_key[s] - 1u], s_n[s]);")]},
                           _pictures(tc.mixed_paths), r"mixed_paths\[0\] 64x192: cell \(\d+, 0\) free is \d+, the restatement has \d+"),
    "less_than_at_max_z": ({H: [("z <= J.max_z", "z < J.max_z")]}, _pictures(tc.depth_specials),
                           r"depth_specials\[0\] 14x1: counts are \[\[11, 0, 0, 3\]\], the restatement has \[\[10, 0, 0, 4\]\]"),
    "less_or_equal_at_occ_lo": ({H: [("J.occ_lo < h", "J.occ_lo <= h")]}, _pictures(tc.borders),
                                r"borders\[0\] 9x10: counts are \[\[0, 10, 16, 64\]\], the restatement has \[\[0, 10, 24, 56\]\]"),
    "u_equal_nx_is_inside": ({H: [("u < (float)J.nx", "u <= (float)J.nx")]}, _pictures(tc.borders),
                             r"borders\[0\] 9x10: counts are \[\[0, 0, 27, 63\]\], the restatement has \[\[0, 10, 24, 56\]\]"),
    "int_taken_before_the_range_test": ({H: [("const bool inside = u >= 0.0f && u < (float)J.nx && v >= 0.0f && v < (float)J.ny;",
                                              "const int i = (int)u, j = (int)v;\n    const bool inside = i >= 0 && i < J.nx && j >= 0 && j < J.ny;"),
                                             ("    const int i = (int)u, j = (int)v;\n    const bool is_free", "    const bool is_free")]},
                                        _pictures(tc.borders), r"borders\[1\] 9x10: counts are \[\[0, 0, 27, 63\]\], the restatement has \[\[0, 10, 24, 56\]\]"),
    "counts_not_rebased_on_the_second_launch": ({API: [("K.counts = out_counts + 4ll * f0;", "")], H: [tc.chunk_edit(CHUNK)]},
                                                lambda d: tc.check_split(d, CHUNK), r"split: frame 0 of 11 \(launches of 4\): counts are \[1, 0, 0, 2\], the restatement has \[0, 0, 0, 1\]"),
    "clear_ignored": ({API: [("J.clear = p->flags & SGS_TOPDOWN_CLEAR;", "J.clear = 0;")]}, _pictures(tc.wall),
                      r"wall\[0\] 67x70: cell \(0, 0\) free is 2779096485 \(0xA5 bytes are left in it\), the restatement has 0"),
    "alignment_refusal_removed": ({API: _NO_REFUSAL}, tc.check_misaligned, r"depth off by \{'depth': 1\} bytes was accepted"),
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    return emu_harness.build_mutants(tmp_path_factory.mktemp("topdown_mutants"), {name: edits for name, (edits, _, _) in MUTANTS.items()},
                                     "libsage_gs_topdown_mutant.so")


@pytest.mark.parametrize("name", list(MUTANTS))
def test_topdown_mutant_is_caught(mutant_libs, name):
    _, check, pattern = MUTANTS[name]
    d = tc.AbiTopdown(_capi.Lib(mutant_libs[name]))
    try:
        with pytest.raises(AssertionError) as e:
            check(d)
    finally:
        d.close()
    print(f"[topdown mutant] {name}: caught: {str(e.value)[:200]}")
    assert re.search(pattern, str(e.value)), f"{name}: failed on another assertion: {str(e.value)[:300]}"


def test_the_unmutated_library_passes_the_mutants_checks():
    d = tc.AbiTopdown(_capi.Lib(emu_harness.build_emu()))
    try:
        tc.check_pictures(d, (tc.sizes, tc.wall, tc.own_cell, tc.mixed_paths, tc.depth_specials, tc.borders))
        tc.check_misaligned(d)
    finally:
        d.close()
