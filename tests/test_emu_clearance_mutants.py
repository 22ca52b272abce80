"""Seeded faults in the clearance map (csrc/sgs_clearance.h, and its entries in csrc/sgs_api.hip), under the wave64 emulator: each is
made in a copy of csrc/, compiled, and must be caught by the check named for it, on the assertion written down here.

One fault of the list this file was written to has no counterpart in these kernels: "the walk stopped at dy >= g of the own row
instead of dy^2 >= best".  A cell starts from best = g^2, so dy < g IS dy^2 < best at the start, and best only shrinks afterwards:
a walk bounded by the own row's g goes on at least as long as the exact one and finds the same minimum — a slower kernel, not a wrong
one (and from a row without obstacles both walk to the map's edge).  What can end a walk too early here is the wave's loop: it must
go on while ANY lane still walks.  The fault seeded in its place ends it with the wave's first lane (walk_ends_with_the_first_lane).
"The margin clamp removed" is seeded as the margin ignored — a sample within the margin collides like one beyond it —, since reading
d2 at the unclamped pixel would read outside the map."""
import re

import pytest

import emu_harness
import clearance_cases as cc
from sage_gs import _capi

H, API = "sgs_clearance.h", "sgs_api.hip"
_pictures = lambda maker, **kw: (lambda d: cc.check_pictures(d, maker(**kw)))                     # noqa: E731
_CELL = r"d2 of cell \(\d+, \d+\) is \d+, the restatement has \d+"
_NO_REFUSAL = [("if (b.words && reinterpret_cast<uintptr_t>(b.at) % 4) SGS_FAIL", "if (false) SGS_FAIL"),
               ('if (reinterpret_cast<uintptr_t>(d2) % 4) SGS_FAIL', "if (false) SGS_FAIL"),
               ("if (reinterpret_cast<uintptr_t>(out) % 4) SGS_FAIL", "if (false) SGS_FAIL"),
               ("if (reinterpret_cast<uintptr_t>(segs) % 8) SGS_FAIL", "if (false) SGS_FAIL")]
_G = "if (row && i < J.nx) g[i] = left < right ? left : right;"

# name: ({file of csrc/: [(anchor, replacement)]}, the check that must catch it, what its first failing assertion says)
MUTANTS = {
    "left_carry_dropped": ({H: [("else if (last >= 0) left = (unsigned)(i - last);", "else if (false) left = (unsigned)(i - last);")]}, _pictures(cc.lane_pictures),
                           r"lane_0_of_65x3 65x3: d2 of cell \(64, 0\) is 4294967295, the restatement has 4097"),
    "right_carry_dropped": ({H: [("else if (next >= 0) right = (unsigned)(next - i);", "else if (false) right = (unsigned)(next - i);")]}, _pictures(cc.lane_pictures),
                            r"lane_64_of_65x3 65x3: d2 of cell \(0, 0\) is 4294967295, the restatement has 4097"),
    "lanes_beyond_nx_are_obstacles": ({H: [("const bool ob = row && i < J.nx && clearance_obstacle(J, m, j, i);",
                                            "const bool ob = row && (i >= J.nx || clearance_obstacle(J, m, j, i));")]},
                                      lambda d: cc.check_sizes(d, [(63, 3)]), r"63x3 none 63x3: d2 of cell \(0, 0\) is 3969, the restatement has 4294967295"),
    "walk_upward_only": ({H: [("if (dy <= down_rows) {", "if (false) {")]}, _pictures(cc.shape_pictures), r"empty_rows_between 130x5: d2 of cell \(\d+, 0\) is \d+, the restatement has \d+"),
    "no_walk_from_a_row_without_obstacles": ({H: [("const bool walks = dy2 < best &&", "const bool walks = best != SGS_CLEAR_NONE && dy2 < best &&")]},
                                             _pictures(cc.shape_pictures), r"empty_rows_between 130x5: d2 of cell \(0, 1\) is 4294967295, the restatement has 10"),
    "row_without_obstacles_gets_g_0": ({H: [(_G, "if (row && i < J.nx) g[i] = (left < right ? left : right) == SGS_CLEAR_NONE ? 0u : (left < right ? left : right);")]},
                                       _pictures(cc.shape_pictures), r"empty_rows_between 130x5: d2 of cell \(0, 0\) is 1, the restatement has 9"),
    "walk_ends_with_the_first_lane": ({H: [("if (!__ballot(walks)) break;", "if (!(__ballot(walks) & 1ull)) break;")]}, _pictures(cc.shape_pictures),
                                      r"empty_rows_between 130x5: " + _CELL),
    "second_map_not_rebased": ({H: [("[m * J.stride + cell] != 0", "[cell] != 0")]}, cc.check_batches, r"B = 3, map 1: " + _CELL),
    "seen_map_reads_the_free_channel": ({H: [("const unsigned free_hits = c[0], occ = c[1];", "const unsigned free_hits = c[0], occ = c[0];")]}, cc.check_seen_maps,
                                        r"seen map 0, min_hits = 1, unseen_blocks = False: " + _CELL),
    "greater_than_at_min_hits": ({H: [("return occ >= J.min_hits ||", "return occ > J.min_hits ||")]}, cc.check_seen_maps,
                                 r"seen map 0, min_hits = 1, unseen_blocks = False: " + _CELL),
    "unseen_blocks_ignored": ({API: [("J.unseen_blocks = p->flags & SGS_CLEARANCE_UNSEEN_BLOCKS;", "J.unseen_blocks = 0;")]}, cc.check_seen_maps,
                              r"seen map 0, min_hits = 1, unseen_blocks = True: " + _CELL),
    "less_than_at_max_d2": ({H: [("best > 0u && best <= J.max_d2", "best > 0u && best < J.max_d2")]}, cc.check_counters,
                            r"max_d2 = [1-9]\d*: counts are \[\d+, \d+, \d+, 0\], the restatement has \[\d+, \d+, \d+, 0\]"),
    "floor_of_v_plus_half": ({H: [("const double q = rint((v - lo) / scale);", "const double q = floor((v - lo) / scale + 0.5);")]}, cc.check_rounding,
                             r"half-way points: segment \d+ .* gives \[\d+, \d+\], the restatement has \[\d+, \d+\]"),
    "margin_ignored": ({H: [("if (!(q >= -(double)margin && q < (double)n + (double)margin)) return false;", "if (!(q >= 0.0 && q < (double)n)) return false;")]},
                       cc.check_flags_margins_samples, r"flags = 0, margin = 2, n_samples = 0: segment \d+ "),
    "samples_start_at_0": ({H: [("for (int s = 1; s <= Q.n_samples; ++s) {", "for (int s = 0; s <= Q.n_samples; ++s) {")]}, cc.check_flags_margins_samples,
                           r"flags = 0, margin = 0, n_samples = 2: segment \d+ .* gives \[0, \d+\], the restatement has \[[12], \d+\]"),
    "alignment_refusal_removed": ({API: _NO_REFUSAL}, cc.check_misaligned, r"src off by \{'src': 1\} bytes was accepted"),
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    return emu_harness.build_mutants(tmp_path_factory.mktemp("clearance_mutants"), {name: edits for name, (edits, _, _) in MUTANTS.items()},
                                     "libsage_gs_clearance_mutant.so")


@pytest.mark.parametrize("name", list(MUTANTS))
def test_clearance_mutant_is_caught(mutant_libs, name):
    _, check, pattern = MUTANTS[name]
    d = cc.AbiClearance(_capi.Lib(mutant_libs[name]))
    try:
        with pytest.raises(AssertionError) as e:
            check(d)
    finally:
        d.close()
    print(f"[clearance mutant] {name}: caught: {str(e.value)[:200]}")
    assert re.search(pattern, str(e.value)), f"{name}: failed on another assertion: {str(e.value)[:300]}"


def test_the_unmutated_library_passes_the_mutants_checks():
    d = cc.AbiClearance(_capi.Lib(emu_harness.build_emu()))
    try:
        cc.check_pictures(d, {**cc.lane_pictures(), **cc.shape_pictures()})
        cc.check_sizes(d, [(63, 3)])
        cc.check_batches(d)
        cc.check_seen_maps(d)
        cc.check_counters(d)
        cc.check_rounding(d)
        cc.check_flags_margins_samples(d)
        cc.check_misaligned(d)
    finally:
        d.close()
