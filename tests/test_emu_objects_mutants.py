"""Seeded faults in the visible-object table (csrc/sgs_objects.h), under the wave64 emulator: each is made in a copy of csrc/, compiled,
and must be caught by object_cases.check_pictures — by the assertion named for it.

z_min's filter is the unsigned comparison itself (patterns with the sign bit, and NaNs, lie above +inf's): the fault that admits
negatives is therefore a run's minimum taken over the patterns read as SIGNED integers, where every negative number and -0 comes first."""
import os
import re
import shutil

import pytest

import emu_harness
import object_cases as oc
from sage_gs import _capi

MUTANTS = {          # name: ([(anchor, replacement)], the pictures that are run)
    "run_continues_across_a_row_end": ([("(lane == 0 || x == 0 || v != prev)", "(lane == 0 || v != prev)")], oc.SMALL),
    "run_head_contributes_length_1": ([("const unsigned long long L = len;", "const unsigned long long L = 1;"),
                                       ("atomicAdd(&s_n[s], len);", "atomicAdd(&s_n[s], 1u);")], oc.SMALL),
    "x_end_without_plus_1": ([("atomicMax(&s_x1[s], x + len);", "atomicMax(&s_x1[s], x + len - 1u);")], oc.SMALL),
    "no_slot_path_dropped": ([("else obj_send(&rows[v], len, x, y, x + len, y + 1u, sx, sy);", "")], (oc.own_label,)),
    "sum_x_accumulated_in_32_bits": ([("atomicAdd(&r->sum_x, sx);", "atomicAdd(reinterpret_cast<unsigned*>(&r->sum_x), (unsigned)sx);")],
                                     oc.SMALL + (oc.sum_over_2_32,)),
    "z_min_admits_negatives": ([("if (lane - d >= seg) z = min(z, o);", "if (lane - d >= seg) z = (unsigned)min((int)z, (int)o);")], oc.SMALL),
    "clear_kernel_skips_empty_rows": ([("for (long long i = first; i < n_rows; i += step) {", "for (long long i = first; i < 0; i += step) {")], oc.SMALL),
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


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    root = tmp_path_factory.mktemp("object_mutants")
    procs, libs = {}, {}
    for k, (name, (edits, _)) in enumerate(MUTANTS.items()):
        base = root / f"m{k}"
        shutil.copytree(os.path.join(emu_harness.PKG, "csrc"), base / "pkg" / "csrc")
        os.makedirs(base / "include")
        shutil.copy(os.path.join(emu_harness.ROOT, "include", "sage_gs.h"), base / "include" / "sage_gs.h")     # (../../include/sage_gs.h)
        path = base / "pkg" / "csrc" / "sgs_objects.h"
        s = path.read_text()
        for old, new in edits:
            assert s.count(old) == 1, f"mutant anchor found {s.count(old)} times: {old!r}"
            s = s.replace(old, new)
        path.write_text(s)
        libs[name] = str(base / "libsage_gs_objects_mutant.so")
        procs[name] = emu_harness.build_emu(src_dir=base / "pkg" / "csrc", out=libs[name], wait=False)
    for name, p in procs.items():
        assert p.wait() == 0, f"{name}: the mutant does not compile"
    return libs


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


def test_the_unmutated_library_passes_the_mutants_checks():
    d = oc.AbiObjects(_capi.Lib(oc.emu_lib_path()))
    try:
        oc.check_pictures(d, oc.SMALL)
    finally:
        d.close()
