"""Seeded faults in the geodesic field and its paths (csrc/sgs_geodesic.h, and their entries in csrc/sgs_api.hip), under the wave64
emulator: each is made in a copy of csrc/, compiled, and must be caught by the check named for it, on the assertion written down here.

One fault of the list this file was written to computes the same result: the comparison's `p^2 < 2 q^2` made `<=`.  In that branch
p > 0 and q > 0, and p^2 = 2 q^2 has no solution in positive integers (sqrt(2) is irrational) — the very fact the feature rests on —, so
`<=` and `<` decide every pair alike.  The fault seeded in its place flips the OTHER branch's comparison (p < 0 and q < 0:
`p^2 > 2 q^2` made `<`); the flip of `p^2 < 2 q^2` itself is seeded as listed.  Under either flip the
relaxation has no fixed point: the local solve is cut at SGS_GEO_MAX_SWEEPS, the tiles stay dirty, and the driver's own bound on the
rounds (nx * ny) is the assertion that fails."""
import re

import pytest

import emu_harness
import geodesic_cases as gc
from sage_gs import _capi

H, API = "sgs_geodesic.h", "sgs_api.hip"
_CELL = r"cell \(\d+, \d+\) is \(\d+, \d+\), the restatement has \(\d+, \d+\)"
_pictures = lambda name: (lambda d: gc.check_pictures(d, {name: gc.pictures(d.T)[name]}))            # noqa: E731
_HALO = "const bool inside = gx >= 0 && gx < J.nx && gy >= 0 && gy < J.ny;"

# name: ({file of csrc/: [(anchor, replacement)]}, the check that must catch it, what its first failing assertion says)
MUTANTS = {
    "diagonal_counted_as_straight": ({H: [("(dx != 0 && dy != 0) ? (1ull << 32) : 1ull", "(dx != 0 && dy != 0) ? 1ull : 1ull")]}, gc.check_sizes,
                                     r"empty_room_corner_seed \d+x\d+: " + _CELL),
    "comparison_flipped": ({H: [("if (p > 0) return p * p < 2 * q * q;", "if (p > 0) return p * p > 2 * q * q;")]}, gc.check_sizes, r"the field of \d+x\d+ does not converge"),
    "comparison_of_the_negative_branch_flipped": ({H: [("return p * p > 2 * q * q;    ", "return p * p < 2 * q * q;    ")]}, gc.check_sizes, r"the field of \d+x\d+ does not converge"),
    "corner_cutting_forbidden": ({H: [("if (v == SGS_GEO_NONE2) continue;\n                        const unsigned long long cand",
                                       "if (v == SGS_GEO_NONE2 || (dx != 0 && dy != 0 && (s_d[at + dx] == SGS_GEO_NONE2 || s_d[at + dy * SGS_GEO_HALO] == SGS_GEO_NONE2))) continue;\n"
                                       "                        const unsigned long long cand")]}, _pictures("diagonal_corridor"),
                                 r"diagonal_corridor \d+x\d+: cell \(\d+, \d+\) is \(4294967295, 4294967295\), the restatement has \(0, \d+\)"),
    "halo_unloaded_on_one_side": ({H: [(_HALO, _HALO[:-1] + " && hx != 0;")]}, gc.check_sizes, _CELL),
    "halo_corners_omitted": ({H: [(_HALO, _HALO[:-1] + " && !((hx == 0 || hx == SGS_GEO_HALO - 1) && (hy == 0 || hy == SGS_GEO_HALO - 1));")]}, _pictures("diagonal_corridor"),
                             r"diagonal_corridor \d+x\d+: cell \(\d+, \d+\) is \(4294967295, 4294967295\), the restatement has \(0, \d+\)"),
    "no_dirty_flag_for_the_diagonal_neighbour": ({H: [("if (ex && ey) s_mark[4 + 3 * ey + ex] = 1;", "if (false) s_mark[4 + 3 * ey + ex] = 1;")]}, _pictures("diagonal_corridor"),
                                                 r"diagonal_corridor \d+x\d+: cell \(\d+, \d+\) is \(4294967295, 4294967295\), the restatement has \(0, \d+\)"),
    "no_dirty_flag_when_only_border_cells_changed": ({H: [("if (ex) s_mark[4 + ex] = 1;", "if (!ex && !ey) s_mark[4] = 1;\n        if (ex) s_mark[4 + ex] = 1;"),
                                                          ("if (tid < 9 && tid != 4 && s_mark[tid]) {", "if (tid < 9 && tid != 4 && s_mark[tid] && s_mark[4]) {")]},
                                                     _pictures("edge_column"), r"edge_column \d+x\d+: cell \(\d+, \d+\) is \(4294967295, 4294967295\), the restatement has \(\d+, 0\)"),
    "local_solve_stops_after_one_sweep": ({H: [("if (!s_changed[sweep & 1]) break;", "break;")]}, gc.check_sizes, _CELL),
    "less_than_at_max_d2": ({H: [("[m * stride + cell] <= max_d2;", "[m * stride + cell] < max_d2;")]}, gc.check_sources, r"d2 source, max_d2 = \d: " + _CELL),
    "blocked_seed_accepted": ({H: [("if (geodesic_blocked(J.src, J.kind, J.stride, J.max_d2, J.nx, m, j, i)) {", "if (false) {")]}, _pictures("sealed_region"),
                              r"sealed_region \d+x\d+: cell \(\d+, \d+\) is \(\d+, \d+\), the restatement has \(\d+, \d+\)"),
    "field_map_ignored": ({API: [("W.w[k] = k < n ? (unsigned)field_map[f0 + k] : 0u;", "W.w[k] = 0u;")]}, gc.check_batches, r"batch field 0 on map 2: " + _CELL),
    "partial_tile_edge_is_free": ({H: [("is_free[k] = inside && !geodesic_blocked(", "is_free[k] = !inside || !geodesic_blocked("),
                                       ("if (!is_free[k] || next[k] == first[k]) continue;", "if (!is_free[k] || next[k] == first[k] || x0 + lx >= J.nx || y0 + ly >= J.ny) continue;")]},
                                  _pictures("edge_wall"), r"edge_wall \d+x\d+: " + _CELL),
    "path_neighbour_order_changed": ({H: [("const int di[8] = {-1, 1, 0, 0, -1, -1, 1, 1}, dj[8] = {0, 0, -1, 1, -1, 1, -1, 1};",
                                           "const int di[8] = {-1, -1, 1, 1, -1, 1, 0, 0}, dj[8] = {-1, 1, -1, 1, 0, 0, -1, 1};"),
                                          ("if (v + (d < 4 ? 1ull : (1ull << 32)) == cur)", "if (v + (d >= 4 ? 1ull : (1ull << 32)) == cur)")]}, gc.check_paths,
                                     r"query \(\d+, \d+\) walks .* the restatement "),
    "path_stops_one_cell_early": ({H: [("if (s == steps) break;", "if (s + 1 == steps) break;")]}, gc.check_paths, r"query \(\d+, \d+\) (has status|walks)"),
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    return emu_harness.build_mutants(tmp_path_factory.mktemp("geodesic_mutants"), {name: edits for name, (edits, _, _) in MUTANTS.items()},
                                     "libsage_gs_geodesic_mutant.so")


@pytest.mark.parametrize("name", list(MUTANTS))
def test_geodesic_mutant_is_caught(mutant_libs, name):
    _, check, pattern = MUTANTS[name]
    d = gc.AbiGeodesic(_capi.Lib(mutant_libs[name]))
    try:
        with pytest.raises(AssertionError) as e:
            check(d)
    finally:
        d.close()
    print(f"[geodesic mutant] {name}: caught: {str(e.value)[:200]}")
    assert re.search(pattern, str(e.value)), f"{name}: failed on another assertion: {str(e.value)[:300]}"


def test_the_unmutated_library_passes_the_mutants_checks():
    d = gc.AbiGeodesic(_capi.Lib(emu_harness.build_emu()))
    try:
        gc.check_sizes(d)
        gc.check_pictures(d, gc.pictures(d.T))
        gc.check_sources(d)
        gc.check_batches(d)
        gc.check_paths(d)
    finally:
        d.close()
