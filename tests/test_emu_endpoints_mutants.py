"""Seeded faults in the item endpoints (csrc/sgs_endpoints.h), under the wave64 emulator: each is made in a copy of csrc/, compiled,
and must be caught by the check named for it, on the assertion written down here.

Every fault keeps every index inside its buffer, so that a faulty library computes wrong numbers, not wild addresses: the neighbour
outside the grid is never loaded (the fault is in what stands for it); the duplicate test looks one entry back from the second entry
on; the window that is not clipped grows the bytes the call says it needs past the work it was given, so no field is written at all."""
import re

import pytest

import emu_harness
import endpoints_cases as ec
from sage_gs import _capi

H = "sgs_endpoints.h"
_Q = r"query \d+ \(.*\) has "

# name: ({file of csrc/: [(anchor, replacement)]}, the check that must catch it, what its first failing assertion says)
MUTANTS = {
    "neighbour_outside_the_grid_is_a_member": ({H: [("const bool left = lx > 0 && f[row * W.w + lx - 1] != 0,", "const bool left = (lx == 0 && W.x0 == 0) || (lx > 0 && f[row * W.w + lx - 1] != 0),")]},
                                               ec.check_shapes, r"shapes: item 0 has boundary = \d+, the restatement has \d+"),
    "left_ballot_word_ignored": ({H: [("left = s > 0 ? l : 0ull,", "left = 0ull,")]}, ec.check_word_seams,
                                 r"seam: item at 63, free cell at 64: " + _Q + r"x = -1, the restatement has 64"),
    "right_ballot_word_ignored": ({H: [("right = s + 1 < segs ? r : 0ull;", "right = 0ull;")]}, ec.check_word_seams,
                                  r"seam: item at 0 and 64, free cell at 63: " + _Q + r"d = 63, the restatement has 1"),
    "upward_sweep_dropped": ({H: [("min(below + 1u, SGS_EP_FAR));", "SGS_EP_FAR);")]}, ec.check_max_dist,
                             r"max_dist 1: free cell at distance 1, sign -1: " + _Q + r"x = -1"),
    "max_dist_compared_with_less_than": ({H: [("(d <= (unsigned)J.max_dist ? d", "(d < (unsigned)J.max_dist ? d")]}, ec.check_max_dist,
                                         r"max_dist 0: free cell at distance 0, sign 1: query 0 " + r"\(.*\) has x = -1"),
    "blocked_cell_accepted": ({H: [("if (!ep_free(J, cell)) continue;", "if (false) continue;")]}, ec.check_sizes, r"\d+x\d+: " + _Q),
    "half_plane_strict": ({H: [("(n * y - sy) * ay < 0) continue;", "(n * y - sy) * ay <= 0) continue;")]}, ec.check_max_dist,
                          r"max_dist 0: free cell at distance 0, sign 1: query 1 " + r"\(.*\) has x = -1"),
    "duplicates_dropped_from_the_sums": ({H: [("sx += x; sy += y;\n", "if (e == 0 || J.cells[begin + e - 1] != (int)c) { sx += x; sy += y; }\n")]}, ec.check_shapes,
                                         r"shapes: item 10 has cx = 38, the restatement has 50"),
    "dot_in_32_bits": ({H: [("if (towards && (n * x - sx) * ax + (n * y - sy) * ay < 0) continue;",
                             "if (towards && (int)((n * x - sx) * ax) + (int)((n * y - sy) * ay) < 0) continue;")]}, ec.check_entry_limit, r"2\^19 entries: " + _Q),
    "tie_goes_to_the_greatest_index": ({H: [("key = min(key, o_key); count += o_count;", "key = max(key, o_key); count += o_count;")]}, ec.check_sizes,
                                       r"\d+x\d+: " + _Q + r"[xy] = "),
    "n_at_d_counted_over_all_d": ({H: [("if (o_d < d) { key = o_key; count = o_count; }", "if (o_d < d) { key = o_key; count += o_count; }")]}, ec.check_sizes,
                                  r"\d+x\d+: " + _Q + r"n_at_d = "),
    "half_rounded_up": ({H: [("if (2 * r == n) return (int)(q + (q & 1ull));", "if (2 * r == n) return (int)(q + 1);")]}, ec.check_shapes,
                        r"shapes: item 1 has cx = 69, the restatement has 68"),
    "window_not_clipped": ({H: [("W.w = min(r.x_end + J.max_dist, J.nx) - W.x0;", "W.w = r.x_end + J.max_dist - W.x0;")]}, ec.check_shapes,
                           r"shapes: item 0 has boundary = 0, the restatement has \d+"),
    "query_item_index_ignored": ({H: [("const EpItem r = J.items[q.item];", "const EpItem r = J.items[0];"), ("f += J.win_off[q.item];", "f += J.win_off[0];")]},
                                 ec.check_batches, r"batch: query 5 "),
    "d2_source_uses_greater_or_equal": ({H: [("static_cast<const unsigned*>(J.src)[cell] > J.max_d2;", "static_cast<const unsigned*>(J.src)[cell] >= J.max_d2;")]},
                                        ec.check_sources, r"d2 source, max_d2 = 0: " + _Q),
    "boundary_by_the_left_and_upper_neighbour_alone": ({H: [("is_boundary = !(left && right && up && down);", "is_boundary = !(left && right && up && down) && (lx == 0 || lx + 1 == W.w || !left || !up);")]},
                              ec.check_shapes, r"shapes: item \d+ has boundary = "),
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    return emu_harness.build_mutants(tmp_path_factory.mktemp("endpoints_mutants"), {name: edits for name, (edits, _, _) in MUTANTS.items()},
                                     "libsage_gs_endpoints_mutant.so")


@pytest.mark.parametrize("name", list(MUTANTS))
def test_endpoints_mutant_is_caught(mutant_libs, name):
    _, check, pattern = MUTANTS[name]
    d = ec.AbiEndpoints(_capi.Lib(mutant_libs[name]))
    try:
        with pytest.raises(AssertionError) as e:
            check(d)
    finally:
        d.close()
    print(f"[endpoints mutant] {name}: caught: {str(e.value)[:200]}")
    assert re.search(pattern, str(e.value)), f"{name}: failed on another assertion: {str(e.value)[:300]}"


def test_the_unmutated_library_passes_the_mutants_checks():
    d = ec.AbiEndpoints(_capi.Lib(emu_harness.build_emu()))
    try:
        for check in (ec.check_shapes, ec.check_word_seams, ec.check_max_dist, ec.check_sizes, ec.check_entry_limit, ec.check_batches, ec.check_sources):
            check(d)
    finally:
        d.close()
