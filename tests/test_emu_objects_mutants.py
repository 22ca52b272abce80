"""Seeded faults in the visible-object table (csrc/sgs_objects.h), under the wave64 emulator: each is made in a copy of csrc/, compiled,
and must be caught by object_cases.check_pictures — by the assertion named for it — or, for the faults of the host entry and of one
path of the reduction (CHECK_MUTANTS), by the check named for it.

z_min's filter is the unsigned comparison itself (patterns with the sign bit, and NaNs, lie above +inf's): the fault that admits
negatives is therefore a run's minimum taken over the patterns read as SIGNED integers, where every negative number and -0 comes first."""
import re

import pytest

import emu_harness
import object_cases as oc
from sage_gs import _capi

H = "sgs_objects.h"
MUTANTS = {          # name: ({file of csrc/: [(anchor, replacement)]}, the pictures that are run)
    "run_continues_across_a_row_end": ({H: [("(lane == 0 || x == 0 || v != prev)", "(lane == 0 || v != prev)")]}, oc.SMALL),
    "run_head_contributes_length_1": ({H: [("const unsigned long long L = len;", "const unsigned long long L = 1;"),
                                           ("atomicAdd(&s_n[s], len);", "atomicAdd(&s_n[s], 1u);")]}, oc.SMALL),
    "x_end_without_plus_1": ({H: [("atomicMax(&s_x1[s], x + len);", "atomicMax(&s_x1[s], x + len - 1u);")]}, oc.SMALL),
    "no_slot_path_dropped": ({H: [("else obj_send(&rows[v], len, x, y, x + len, y + 1u, sx, sy);", "")]}, (oc.own_label,)),
    "sum_x_accumulated_in_32_bits": ({H: [("atomicAdd(&r->sum_x, sx);", "atomicAdd(reinterpret_cast<unsigned*>(&r->sum_x), (unsigned)sx);")]},
                                     oc.SMALL + (oc.sum_over_2_32,)),
    "z_min_admits_negatives": ({H: [("if (lane - d >= seg) z = min(z, o);", "if (lane - d >= seg) z = (unsigned)min((int)z, (int)o);")]}, oc.SMALL),
    "clear_kernel_skips_empty_rows": ({H: [("for (long long i = first; i < n_rows; i += step) {", "for (long long i = first; i < 0; i += step) {")]}, oc.SMALL),
}
# The first failing assertion of object_cases.check_pictures on each mutant, with its figures (the tables are deterministic).
CAUGHT_BY = {
    "run_continues_across_a_row_end": r"one_label_ragged\[0\] 67x5: label 2: x_end is 128, the restatement has 67",
    "run_head_contributes_length_1": r"one_label_ragged\[0\] 67x5: label 2: n_pixels is 10, the restatement has 335",
    "x_end_without_plus_1": r"one_pixel\[0\] 1x1: label 1: x_end is 0, the restatement has 1",
    "no_slot_path_dropped": r"own_label\[0\] 97x53: label \d+: n_pixels is 0, the restatement has 1",
    "sum_x_accumulated_in_32_bits": r"sum_over_2_32\[0\] 40000x6: label 0: sum_x is 504912704, the restatement has 4799880000",
    "z_min_admits_negatives": r"depth_specials\[0\] 16x4: label 0: z_min is 0x7f800000, the restatement has 0x0",
    "clear_kernel_skips_empty_rows": r"one_pixel\[0\] 1x1: the empty row of label 0 was not written \(0xA5 bytes are left in it\)",
}


# Seeded faults that pictures of one frame cannot see, or that one picture is built for: name: ({file of csrc/: edits}, the checks run —
# EACH of them must catch the fault by itself —, what the first failure of each says).  The launch split is exercised with
# SGS_OBJ_MAX_FRAMES at 4, as test_emu_objects.py does.
CHUNK = 4
_SPLIT = lambda d: oc.check_split(d, CHUNK)                                                    # noqa: E731
_MIXED, _COLLIDING = (lambda d: oc.check_pictures(d, (oc.mixed_paths,))), (lambda d: oc.check_pictures(d, (oc.colliding,)))   # noqa: E731
_NO_REFUSAL = [(f"if (reinterpret_cast<uintptr_t>({arg}) % {n}) SGS_FAIL", f"if (false) SGS_FAIL")
               for arg, n in (("out_rows", 8), ("ids", 4), ("depth", 4), ("out_counts", 4))]
CHECK_MUTANTS = {
    "chunk_rows_not_rebased": ({"sgs_api.hip": [("K.rows = J.rows + (int64_t)f0 * n_labels; ", "")], "sgs_objects.h": [oc.chunk_edit(CHUNK)]},
                               [_SPLIT], [r"split: frame 0 of 11 \(launches of 4\): label 0: n_pixels is 3, the restatement has 1"]),
    "chunk_counts_not_rebased": ({"sgs_api.hip": [("K.counts = out_counts + 2ll * f0;", "")], "sgs_objects.h": [oc.chunk_edit(CHUNK)]},
                                 [_SPLIT], [r"split: frame 2 of 11 \(launches of 4\): counts are \[3, 0\], the restatement has \[1, 0\]"]),
    "no_slot_path_drops_y_end": ({"sgs_objects.h": [("else obj_send(&rows[v], len, x, y, x + len, y + 1u, sx, sy);",
                                                     "else obj_send(&rows[v], len, x, y, x + len, 0u, sx, sy);")]},
                                 [_MIXED, _COLLIDING], [r"mixed_paths\[0\] 64x96: label 1: y_end is 29, the restatement has 96",
                                                        r"colliding\[0\] 40x9: label 1: y_end is 0, the restatement has 9"]),
    "no_slot_path_drops_its_depth": ({"sgs_objects.h": [("else obj_send_z(&rows[v], z);", "else {}")]},
                                     [_MIXED, _COLLIDING], [r"mixed_paths\[0\] 64x96: label 1: z_min is 0x3f800000, the restatement has 0x3f000000",
                                                            r"colliding\[0\] 40x9: label 1: z_min is 0x7f800000, the restatement has"]),
    "slot_flush_drops_x_min": ({"sgs_objects.h": [("obj_send(r, s_n[s], s_x0[s], s_y0[s], s_x1[s], s_y1[s], s_sx[s], s_sy[s]);",
                                                   "obj_send(r, s_n[s], 0x7FFFFFFFu, s_y0[s], s_x1[s], s_y1[s], s_sx[s], s_sy[s]);")]},
                               [_MIXED, _COLLIDING], [r"mixed_paths\[0\] 64x96: label 2: x_min is 2147483647, the restatement has 0",
                                                      r"colliding\[0\] 40x9: label \d+: x_min is 2147483647, the restatement has"]),
    "alignment_refusal_removed": ({"sgs_api.hip": _NO_REFUSAL}, [oc.check_misaligned], [r"out_rows off by \{'rows': 4\} bytes was accepted"]),
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    edits = {name: e for name, (e, _) in MUTANTS.items()}
    edits.update({name: e for name, (e, _, _) in CHECK_MUTANTS.items()})
    return emu_harness.build_mutants(tmp_path_factory.mktemp("object_mutants"), edits, "libsage_gs_objects_mutant.so")


@pytest.mark.parametrize("name", list(MUTANTS))
def test_object_mutant_is_caught(mutant_libs, name):
    d = oc.AbiObjects(_capi.Lib(mutant_libs[name]))
    caught = None
    try:
        oc.check_pictures(d, MUTANTS[name][1])
    except AssertionError as e:
        caught = e
    finally:
        d.close()
    assert caught is not None, f"{name}: the table's checks pass on this mutant"
    print(f"[object mutant] {name}: caught: {str(caught)[:200]}")
    assert re.search(CAUGHT_BY[name], str(caught)), f"{name}: failed on another assertion: {str(caught)[:300]}"


@pytest.mark.parametrize("name", list(CHECK_MUTANTS))
def test_object_check_mutant_is_caught(mutant_libs, name):
    """The launch split: a chunk's rows or counts pointer left at the call's first frame is caught by check_split (the second launch
    adds its frames to the first four's rows / counters).  The alignment refusal removed is caught by check_misaligned alone, and
    only here: on a GPU the misaligned atomics must not run.
    The path faults — the no-slot path dropping y_end or its depth, the slot's flush dropping x_min — are caught by mixed_paths, on
    label a (no-slot: its y_end falls back to region 0's, its z_min to the slot path's least) or on c (flush).  The older `colliding`
    picture catches each of them as well — four of its five labels have no slot anywhere and its fifth has nothing but the slot — so
    both are run, each by itself; what only mixed_paths has is a row fed by both paths from different workgroups."""
    _, checks, caught_by = CHECK_MUTANTS[name]
    d = oc.AbiObjects(_capi.Lib(mutant_libs[name]))
    try:
        for check, pattern in zip(checks, caught_by):
            with pytest.raises(AssertionError) as e:
                check(d)
            print(f"[object mutant] {name}: caught: {str(e.value)[:200]}")
            assert re.search(pattern, str(e.value)), f"{name}: failed on another assertion: {str(e.value)[:300]}"
    finally:
        d.close()


def test_the_unmutated_library_passes_the_mutants_checks():
    d = oc.AbiObjects(_capi.Lib(emu_harness.build_emu()))
    try:
        oc.check_pictures(d, oc.SMALL + oc.PATHS)
        oc.check_misaligned(d)
    finally:
        d.close()
