"""The connected regions (sgs_regions_label, csrc/sgs_regions.h) under the wave64 emulator: regions_cases' sizes, pictures, sources,
batches, rows, the reference's recorded answers and the refusals, over host buffers.  Every comparison is exact."""
import pytest

import emu_harness
import regions_cases as rc


@pytest.fixture(scope="module")
def drv():
    d = rc.AbiRegions(emu_harness.lib())
    yield d
    d.close()


def test_the_tile_and_the_pictures(drv):
    assert drv.T >= 16 and drv.T % 8 == 0
    rc.check_picture_properties(drv.T)


def test_sizes(drv):
    rc.check_sizes(drv)


def test_pictures(drv):
    rc.check_pictures(drv, rc.pictures(drv.T))


def test_capacity_exceeded(drv):
    rc.check_capacity(drv)


def test_sources(drv):
    rc.check_sources(drv)


def test_batches(drv):
    rc.check_batches(drv)


def test_rows_and_counters(drv):
    rc.check_rows(drv)


def test_reachability_on_the_golden_grids(drv):
    rc.check_reachability_drv(drv)


def test_the_references_semantic_map_items(drv):
    rc.check_golden_drv(drv)


def test_refusals(drv):
    rc.check_refusals(drv)
