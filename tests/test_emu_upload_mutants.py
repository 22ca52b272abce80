"""Seeded faults in the scene upload (csrc/sgs_kernels.h k_mean_bounds ... k_chunk_bounds, and the pass loop in csrc/sgs_api.hip), under
the wave64 emulator: each is made in a copy of csrc/, compiled for the host (never for gfx950), and must be caught by upload_cases' checks —
by the assertion named for it, not by a crash (every fault keeps the sort's stores inside its buffers).

The same mutants then go through the tests that named the upload before — test_z_order_sort_of_a_scene_that_spans_several_scan_workgroups,
test_compressed_upload_decodes_on_the_device_and_sorts_in_z_order and parity_cases.case_chunk_bounds: which of them those let through is
printed, asserted and written down in DESIGN.md §9: a frame does not depend on the layout, so they see almost none."""
import os
import re

import pytest

import emu_harness
import parity_cases as pc
import upload_cases as uc

K, API = "sgs_kernels.h", "sgs_api.hip"
MUTANTS = {          # name: {file of csrc/: [(anchor, replacement)]}
    "spread_mask_off": {K: [("v = (v | v << 4) & 0x10c30c30c30c30c3ull;", "v = (v | v << 4) & 0x10c30c30c30c30c1ull;")]},
    "y_shift_dropped": {K: [("| sgs_spread21(q[1]) << 1 |", "| sgs_spread21(q[1]) |")]},
    "seven_passes": {API: [("for (int shift = 0; shift < 64; shift += 8, cur ^= 1) {", "for (int shift = 0; shift < 56; shift += 8, cur ^= 1) {")]},
    "rank_reversed_within_a_run": {K: [("if (valid) { keys_out[dst + rank] = k; idx_out[dst + rank] = v; }",
                                        "if (valid) { const unsigned rr = (unsigned)__popcll(peers) - 1u - rank; keys_out[dst + rr] = k; idx_out[dst + rr] = v; }")]},
    # (keys then collide and leave holes in the sort's output; the second patch is no fault: it zeroes the sort's buffers, so that a hole
    #  reads as Gaussian 0 and not as whatever the heap held — the fault must fail an assertion, not read the scene out of bounds)
    "bsum_not_added": {K: [("for (unsigned g = 0; g < at / SGS_RSCAN_SPAN; ++g) run += bsum[g];", "(void)bsum;")],
                       API: [("keys[k] = own_keys[k].p; idx[k] = own_idx[k].p;",
                              "keys[k] = own_keys[k].p; idx[k] = own_idx[k].p; hipMemset(keys[k], 0, (size_t)n * 8); hipMemset(idx[k], 0, (size_t)n * 4);")]},
    "wave_base_from_the_wrong_quarter": {K: [("for (int w = 0; w < 4; ++w) { const unsigned c = s_cur[w][tid]; s_cur[w][tid] = run; run += c; }",
                                              "for (int w = 3; w >= 0; --w) { const unsigned c = s_cur[w][tid]; s_cur[w][tid] = run; run += c; }")]},
    "finite_test_removed_from_the_bounds": {K: [("if (fabsf(m[c]) < 3.0e38f) { const unsigned k = sgs_ordered(m[c]);", "if (true) { const unsigned k = sgs_ordered(m[c]);")]},
    "padding_lanes_in_the_chunk_bounds": {K: [("const bool real = pos < n;  ", "const bool real = pos < n || true;  ")]},
    "radius_padding_0_999": {K: [("r = r * 1.0001f + 1.0e-6f", "r = r * 0.999f + 1.0e-6f")]},
    "s_max_by_fminf": {K: [("sm = fmaxf(sm, __shfl_xor(sm, d));", "sm = fminf(sm, __shfl_xor(sm, d));")]},
    "radius_always_inf": {K: [("if (__ballot(bad) != 0ull || !(r < 3.0e37f)", "if (true || __ballot(bad) != 0ull || !(r < 3.0e37f)")]},
}
# The cases the mutants go through, in this order (the unmutated library passes them all), and the first assertion that fails on each.
CHECKS = ("size_65", "size_513", "size_2049", "every_mean_equal", "two_points_interleaved") + tuple(f"one_digit_{j}" for j in range(8)) + \
         ("key_bit_62", "rows_of_lanes_digit_0", "random_cloud", "non_finite_means", "size_32768", "size_32769")
CAUGHT_BY = {
    "spread_mask_off": r"keys that differ in digit 0 only: permutation: differs from the stable sort",      # (random keys rarely tie in all other bits)
    "y_shift_dropped": r"size 65: permutation: differs from the stable sort",
    "seven_passes": r"size 65: permutation: differs from the stable sort .*\(keys ascending: False\)",
    "rank_reversed_within_a_run": r"size 65: permutation: differs from the stable sort",
    "bsum_not_added": r"size 32769: permutation: not a permutation",
    "wave_base_from_the_wrong_quarter": r"size 513: permutation: differs from the stable sort",          # (65: one wave; 513: the second quarter's first key)
    "finite_test_removed_from_the_bounds": r"non-finite means: permutation: differs from the stable sort",
    "padding_lanes_in_the_chunk_bounds": r"size 65: chunk bounds: the centre of chunk 1",        # (the chunk of one real Gaussian)
    "radius_padding_0_999": r"size 65: chunk bounds: R of chunk 0 is .* a member lies outside the sphere",
    "s_max_by_fminf": r"size 65: chunk bounds: s_max of chunk 0",
    "radius_always_inf": r"size 65: chunk bounds: R of chunk 0 is inf, more than .* the sphere is not tight",
}
# What the tests that named the upload before this file let through (deterministic; DESIGN.md §9 quotes it).
OLD_TESTS_CATCH = {
    "spread_mask_off": (),
    "y_shift_dropped": ("case_chunk_bounds",),                # (its "more than 40 % of the chunks are skipped": the order has lost an axis)
    "seven_passes": ("case_chunk_bounds",),                   # (the same assertion)
    "rank_reversed_within_a_run": (),
    "bsum_not_added": ("z_order_sort",),                      # (the laid-out scene is not the input: Gaussians are missing)
    "wave_base_from_the_wrong_quarter": (),
    "finite_test_removed_from_the_bounds": (),
    "padding_lanes_in_the_chunk_bounds": (),
    "radius_padding_0_999": (),                               # (a sphere that does not hold its members: no frame of theirs shows it)
    "s_max_by_fminf": (),
    "radius_always_inf": ("case_chunk_bounds",),              # (nothing is skipped)
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    return emu_harness.build_mutants(tmp_path_factory.mktemp("upload_mutants"), MUTANTS, "libsage_gs_upload_mutant.so")


def _checks(d):
    for name in CHECKS:
        uc.CASES[name](d)


def test_every_seeded_fault_has_a_named_check():
    assert set(CAUGHT_BY) == set(MUTANTS) == set(OLD_TESTS_CATCH)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_upload_mutant_is_caught(mutant_libs, name):
    d = emu_harness.EmuRenderer(record_capacity=1 << 22, lib_path=mutant_libs[name])
    caught = None
    try:
        _checks(d)
    except AssertionError as e:
        caught = e
    finally:
        d.close()
    assert caught is not None, f"{name}: the upload's checks pass on this mutant"
    print(f"[upload mutant] {name}: caught: {str(caught)[:240]}")
    assert re.search(CAUGHT_BY[name], str(caught)), f"{name}: failed on another assertion: {str(caught)[:400]}"


def test_the_unmutated_library_passes_the_mutants_checks():
    d = emu_harness.EmuRenderer(record_capacity=1 << 22)
    try:
        _checks(d)
    finally:
        d.close()


def _old_tests(lib_path, tmp_path):
    """The three tests that named the upload before, on the emulator library at lib_path: the names of those that fail."""
    import test_emu_parity as tep
    from sage_gs import _capi
    failed = []
    keep = emu_harness._lib
    emu_harness._lib = _capi.Lib(lib_path)              # (the two tests make their own EmuRenderer of emu_harness.lib())
    try:
        os.makedirs(tmp_path, exist_ok=True)
        for what, run in (("z_order_sort", tep.test_z_order_sort_of_a_scene_that_spans_several_scan_workgroups),
                          ("compressed_upload", lambda: tep.test_compressed_upload_decodes_on_the_device_and_sorts_in_z_order(tmp_path)),
                          ("case_chunk_bounds", None)):
            try:
                if run is not None:
                    run()
                else:
                    d = emu_harness.EmuRenderer(record_capacity=1 << 21)
                    try:
                        pc.case_chunk_bounds(d, n=6000, res=(208, 150))
                    finally:
                        d.close()
            except AssertionError:
                failed.append(what)
    finally:
        emu_harness._lib = keep
    return failed


def test_what_the_earlier_upload_tests_let_through(mutant_libs, tmp_path):
    """The measure of the gap: every mutant through the two tests that named the upload and case_chunk_bounds."""
    seen = {}
    for k, name in enumerate(MUTANTS):
        seen[name] = tuple(_old_tests(mutant_libs[name], tmp_path / f"m{k}"))
        print(f"[upload mutant] {name}: the earlier tests: {'caught by ' + ', '.join(seen[name]) if seen[name] else 'LET THROUGH'}")
    through = [n for n, f in seen.items() if not f]
    print(f"[upload mutant] let through by the earlier tests: {len(through)} of {len(seen)}: {', '.join(through)}")
    assert seen == OLD_TESTS_CATCH, seen
