"""Seeded faults in the connected regions (csrc/sgs_regions.h), under the wave64 emulator: each is made in a copy of csrc/, compiled,
and must be caught by the check named for it, on the assertion written down here.

Every fault leaves the forest's indices inside the map (a parent, a root and a label stay below the number of cells), so that a
faulty library computes wrong numbers, not wild addresses: the row written past capacity goes ONE row past, into the driver's
sentinel bytes; the outside cells of a partial tile are put into the set on a picture (edge_hooks) whose pieces at the edges each
hold a cell that precedes every outside cell of their tile."""
import re

import pytest

import emu_harness
import regions_cases as rc
from sage_gs import _capi

H = "sgs_regions.h"
_CELL = r"cell \(\d+, \d+\) has label \d+, the restatement has \d+"
_pictures = lambda *names: (lambda d: rc.check_pictures(d, {n: rc.pictures(d.T)[n] for n in names}))            # noqa: E731

# name: ({file of csrc/: [(anchor, replacement)]}, the check that must catch it, what its first failing assertion says)
MUTANTS = {
    "corner_diagonal_not_merged": ({H: [("if (xx < 0 || xx >= J.nx) continue;", "if (xx < 0 || xx >= J.nx || xx / SGS_REG_TILE != x / SGS_REG_TILE) continue;")]},
                                   _pictures("corner_diagonal"), r"corner_diagonal \d+x\d+ under 8: " + _CELL),
    "anti_diagonal_neighbour_omitted": ({H: [("if (dx != 0 && J.conn == 4) continue;\n            const int xx", "if (dx != 0 && J.conn == 4) continue;\n            if (dx < 0) continue;\n            const int xx")]},
                                        _pictures("corner_anti_diagonal"), r"corner_anti_diagonal \d+x\d+ under 8: " + _CELL),
    "connectivity_ignored_under_4": ({H: [("if (dx != 0 && dy != 0 && J.conn == 4) continue;", "if (false) continue;")]}, _pictures("corner_diagonal under 4"),
                                     r"corner_diagonal under 4 \d+x\d+ under 4: " + _CELL),
    "vertical_borders_not_merged": ({H: [("if (t < n_v) {", "if (false && t < n_v) {")]}, _pictures("serpentine"), r"serpentine \d+x\d+ under 4: " + _CELL),
    "larger_root_kept_in_the_union": ({H: [("if (a < b) { const unsigned t = a; a = b; b = t; }", "if (a > b) { const unsigned t = a; a = b; b = t; }")]},
                                      _pictures("comb"), r"comb \d+x\d+ under 4: " + _CELL),
    "rank_not_in_raster_order": ({H: [("for (int u = 0; u < k * SGS_REG_WAVES + wave; ++u) before += s_n[u];",
                                       "for (int u = 0; u < SGS_REG_PER_THREAD * SGS_REG_WAVES; ++u) before += (u % SGS_REG_WAVES < wave || (u % SGS_REG_WAVES == wave && u / SGS_REG_WAVES < k)) ? s_n[u] : 0u;")]},
                                 _pictures("checkerboard under 4"), r"checkerboard under 4 \d+x\d+ under 4: " + _CELL),
    "flatten_stops_after_one_hop": ({H: [("for (unsigned step = 0; step < J.cells; ++step) {\n                    const unsigned p = parent[r];",
                                          "for (unsigned step = 0; step < 1u; ++step) {\n                    const unsigned p = parent[r];")]},
                                    _pictures("serpentine"), r"serpentine \d+x\d+ under 4: " + _CELL),
    "local_solve_cut_to_one_sweep": ({H: [("if (!s_changed[sweep & 1] || sweep == SGS_REG_MAX_SWEEPS) break;", "break;")]}, rc.check_sizes, _CELL),
    "partial_tile_outside_cells_in_the_set": ({H: [("in_set[k] = inside && reg_in_set(", "in_set[k] = !inside || reg_in_set(")]}, _pictures("edge_hooks"),
                                              r"edge_hooks \d+x\d+ under 8: " + _CELL),
    "hi_compared_with_less_than": ({H: [("return J.lo <= v && v <= J.hi;", "return J.lo <= v && v < J.hi;")]}, rc.check_sources, r"mask, lo = 1, hi = 255: " + _CELL),
    "x_end_without_the_plus_one": ({H: [("atomicMax(&s_x1[s], x + len);", "atomicMax(&s_x1[s], x + len - 1u);")]}, rc.check_rows,
                                   r"rows picture, max_regions = 7: row 0 has x_end = \d+, the restatement has \d+"),
    "row_written_past_max_regions": ({H: [("if (label > (unsigned)J.max_regions) return;", "if (label > (unsigned)J.max_regions + 1u) return;")]}, rc.check_capacity,
                                     r"bytes were written behind out_rows"),
    "map_index_ignored_in_a_batch": ({H: [("[m * J.stride + cell]\n", "[0 * J.stride + cell]\n")]}, rc.check_batches, r"batch map 1 under 8: " + _CELL),
    "scan_base_not_reset_between_maps": ({H: [("unsigned base = 0;\n    for (int u = 0; u < tid; ++u)", "unsigned base = m != 0;\n    for (int u = 0; u < tid; ++u)")]}, rc.check_batches,
                                         r"batch map 1 under 8: " + _CELL),
    "largest_area_tie_takes_the_greatest_label": ({H: [("if (area[r] > best) {", "if (area[r] >= best) {"), ("(s_area[u] == best && s_label[u] < label)", "(s_area[u] == best && s_label[u] > label)")]},
                                                  rc.check_rows, r"rows picture, max_regions = 7: counters \[5, 42, 12, 4\], the restatement has \[5, 42, 12, 1\]"),
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    return emu_harness.build_mutants(tmp_path_factory.mktemp("regions_mutants"), {name: edits for name, (edits, _, _) in MUTANTS.items()},
                                     "libsage_gs_regions_mutant.so")


@pytest.mark.parametrize("name", list(MUTANTS))
def test_regions_mutant_is_caught(mutant_libs, name):
    _, check, pattern = MUTANTS[name]
    d = rc.AbiRegions(_capi.Lib(mutant_libs[name]))
    try:
        with pytest.raises(AssertionError) as e:
            check(d)
    finally:
        d.close()
    print(f"[regions mutant] {name}: caught: {str(e.value)[:200]}")
    assert re.search(pattern, str(e.value)), f"{name}: failed on another assertion: {str(e.value)[:300]}"


def test_the_unmutated_library_passes_the_mutants_checks():
    d = rc.AbiRegions(_capi.Lib(emu_harness.build_emu()))
    try:
        rc.check_sizes(d)
        rc.check_pictures(d, rc.pictures(d.T))
        rc.check_capacity(d)
        rc.check_sources(d)
        rc.check_batches(d)
        rc.check_rows(d)
    finally:
        d.close()
