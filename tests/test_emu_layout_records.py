"""layout_record_cases.py under the wave64 emulator, and the seeded fault they exist for: a composite that gathers splats[slot] without the
lookup through the scene's inverse permutation (csrc/sgs_kernels.h splat_at) — everywhere, and at each of the four gather sites alone.
Mutants are emulator builds: never compiled for gfx950, never run in a `gpu` test."""
import re

import pytest

import emu_harness
import layout_record_cases as lc

K = "sgs_kernels.h"
MUTANTS = {          # name: [(anchor, replacement)] in csrc/sgs_kernels.h
    "gather_without_the_lookup": [("{ return inv ? inv[slot] : slot; }", "{ return slot; }")],
    "single_batch_gather_without_the_lookup": [("splats + splat_at(inv, have ? (unsigned)mine : 0u)", "splats + (have ? (unsigned)mine : 0u)")],
    "multi_batch_gather_without_the_lookup": [("splats + splat_at(inv, gv[gb + (unsigned)tid])", "splats + gv[gb + (unsigned)tid]")],
    "deep_cull_gather_without_the_lookup": [("splats + splat_at(inv, hv[u] ? (unsigned)kq[u] : 0u)", "splats + (hv[u] ? (unsigned)kq[u] : 0u)")],
    "resort_keys_without_the_lookup": [("splats[splat_at(inv, a_v[i])].key", "splats[a_v[i]].key")],
}
DIFFERS = r"differs from the frame of the caller's order in \d+ pixels|the fully sorted queues differ between the two layouts"
CAUGHT_BY = [        # (mutant, case, the assertion that must catch it)
    ("gather_without_the_lookup", lc.case_ties_against_the_layout, r"ties against the layout: .*" + DIFFERS),
    ("gather_without_the_lookup", lc.case_every_gather_site, r"every gather site: .*" + DIFFERS),
    ("single_batch_gather_without_the_lookup", lc.case_every_gather_site, r"every gather site: the Z-ordered scene's frame 'plain' differs"),
    ("multi_batch_gather_without_the_lookup", lc.case_every_gather_site, r"every gather site: .*" + DIFFERS),
    ("deep_cull_gather_without_the_lookup", lc.case_deep_tile_gather, r"deep-tile gather: the Z-ordered scene's frame 'plain' differs"),
    ("resort_keys_without_the_lookup", lc.case_every_gather_site, r"every gather site: .*" + DIFFERS),
]
assert {m for m, _, _ in CAUGHT_BY} == set(MUTANTS)


@pytest.fixture(scope="module")
def drv():
    d = emu_harness.EmuRenderer(record_capacity=1 << 21)
    yield d
    d.close()


def test_ties_against_the_layout(drv):
    lc.case_ties_against_the_layout(drv)


def test_export_by_index(drv):
    lc.case_export_by_index(drv)


def test_every_gather_site(drv):
    lc.case_every_gather_site(drv)


def test_deep_tile_gather(drv):
    lc.case_deep_tile_gather(drv)


def test_group_path(drv):
    lc.case_group_path(drv)


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    return emu_harness.build_mutants(tmp_path_factory.mktemp("layout_record_mutants"), {name: {K: e} for name, e in MUTANTS.items()},
                                     "libsage_gs_layout_mutant.so")


@pytest.mark.parametrize("name,case,pattern", CAUGHT_BY, ids=[f"{m}-{c.__name__}" for m, c, _ in CAUGHT_BY])
def test_gather_without_the_lookup_is_caught(mutant_libs, name, case, pattern):
    d = emu_harness.EmuRenderer(record_capacity=1 << 21, lib_path=mutant_libs[name])
    caught = None
    try:
        case(d)
    except AssertionError as e:
        caught = e
    finally:
        d.close()
    assert caught is not None, f"{name}: {case.__name__} passes on this mutant"
    print(f"[layout mutant] {name}: caught: {str(caught)[:300]}")
    assert re.search(pattern, str(caught)), f"{name}: failed on another assertion: {str(caught)[:400]}"
