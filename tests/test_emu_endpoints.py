"""The item endpoints (sgs_endpoints, csrc/sgs_endpoints.h) under the wave64 emulator: endpoints_cases' sizes, word seams, search
distances, shapes, the entry limit, flagged items, sources, batches, the short work and its retry, the reference's recorded answers and
the refusals, over host buffers.  Every comparison is exact."""
import pytest

import emu_harness
import endpoints_cases as ec


@pytest.fixture(scope="module")
def drv():
    d = ec.AbiEndpoints(emu_harness.lib())
    yield d
    d.close()


def test_the_tile(drv):
    assert drv.T == 64


def test_sizes(drv):
    ec.check_sizes(drv)


def test_word_seams(drv):
    ec.check_word_seams(drv)


def test_max_dist_and_one_past_it(drv):
    ec.check_max_dist(drv)


def test_shapes_edges_ring_and_half_centroids(drv):
    ec.check_shapes(drv)


def test_an_item_equal_to_the_grid(drv):
    ec.check_whole_grid(drv)


def test_the_entry_limit_and_one_past_it(drv):
    ec.check_entry_limit(drv)


def test_flagged_items_and_invalid_queries(drv):
    ec.check_flagged_items(drv)


def test_sources(drv):
    ec.check_sources(drv)


def test_batches(drv):
    ec.check_batches(drv)


def test_short_work_then_the_retry(drv):
    ec.check_short_work(drv)


def test_the_references_answers(drv):
    ec.check_golden_drv(drv)


def test_refusals(drv):
    ec.check_refusals(drv)
