"""The connected regions on the MI355X (sgs_regions_label): regions_cases' sizes, pictures, sources, batches, rows, the reference's
recorded answers and the refusals through device pointers, at the emulator's small shapes; one call of four 512 x 512 maps against the
restatement; and the layers above the C ABI — Renderer.label_regions, sage_gs.regions.label / Regions / semantic_map_items,
ClearanceMap.free_regions and same_region from a semantic-map JSON.  Every comparison is exact.  Neither SciPy nor the reference's
tree is used here: its answers come from tests/golden/regions_golden.json and geodesic_golden.json."""
import numpy as np
import pytest

import geodesic_ref
import regions_cases as rc
import regions_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    from sage_gs import Renderer
    rr = Renderer("cuda:0")
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def drv(r):
    return rc.GpuRegions(r)


@pytest.fixture(scope="session")
def maps_512():
    """(four maps bool [4, 512, 512], the restatement's (labels, rows, counts) per map at 64 rows), computed once."""
    ob = geodesic_ref.rooms_with_doors(512)
    maps = np.stack([~ob, ob, ~geodesic_ref.serpentine_maze(512), np.random.RandomState(12).rand(512, 512) < 0.5])
    return maps, [ref.regions(m, 8, max_regions=64) for m in maps]


def test_sizes_on_the_gpu(drv):
    rc.check_sizes(drv)


def test_pictures_on_the_gpu(drv):
    rc.check_pictures(drv, rc.pictures(drv.T))
    rc.check_capacity(drv)


def test_sources_and_batches_on_the_gpu(drv):
    rc.check_sources(drv)
    rc.check_batches(drv)


def test_rows_and_counters_on_the_gpu(drv):
    rc.check_rows(drv)


def test_the_references_own_answers_on_the_gpu(drv):
    rc.check_reachability_drv(drv)
    rc.check_golden_drv(drv)


def test_refusals_on_the_gpu(drv):
    rc.check_refusals(drv)


def test_four_maps_of_512_in_one_call(r, maps_512):
    import torch
    from sage_gs import _capi
    maps, want = maps_512
    labels, rows, counts = r.label_regions(torch.from_numpy(maps).to(r.device), max_regions=64)
    assert labels.shape == (4, 512, 512) and labels.dtype == torch.int32 and rows.shape == (4, 64, 10) and counts.shape == (4, 4)
    labels, counts = labels.cpu().numpy(), counts.cpu().numpy().view(np.uint32)
    rows = rows.cpu().numpy().reshape(4, -1).view(_capi.REGION_ROW_DTYPE)
    for k, (wl, wr, wc) in enumerate(want):
        diff = np.nonzero(labels[k] != wl)
        assert len(diff[0]) == 0, f"map {k}: {len(diff[0])} cells differ from the restatement, first (i, j) = {(int(diff[1][0]), int(diff[0][0]))}"
        assert counts[k].tolist() == wc.tolist() and rows[k].tobytes() == wr.tobytes(), f"map {k}: rows or counters differ"
    assert counts[0, 0] == 1 and counts[2, 0] == 1 and counts[3, 0] > 64             # the doors join every room; the maze is one corridor
    alone, _, c1 = r.label_regions(torch.from_numpy(maps[3]).to(r.device), max_regions=0)
    assert np.array_equal(alone.cpu().numpy(), labels[3]) and c1.cpu().numpy().view(np.uint32).tolist() == counts[3].tolist()


def test_label_regions_arguments(r):
    import torch
    a = torch.from_numpy(rc.rows_picture(32)).to(r.device)
    labels, rows, counts = r.label_regions(a)
    assert labels.shape == a.shape and rows.shape == (1024, 10) and counts.cpu().tolist() == [5, 42, 12, 1]
    as_d2, _, _ = r.label_regions(torch.where(a, 9, 4).to(torch.int32), lo=5)
    four, _, c4 = r.label_regions(a, connectivity=4, max_regions=0)
    assert torch.equal(as_d2, labels) and torch.equal(four, labels) and c4.cpu().tolist() == [5, 42, 12, 1]
    for bad in (dict(src=a.float()), dict(src=a.cpu()), dict(src=a, connectivity=6), dict(src=a, lo=3, hi=2), dict(src=a, hi=256), dict(src=a, source="topdown"),
                dict(src=a, max_regions=-1), dict(src=a, lo=-1)):
        with pytest.raises(ValueError):
            r.label_regions(bad.pop("src"), **bad)


def test_regions_label_and_the_regions_object(r, maps_512):
    from sage_gs import regions
    maps, want = maps_512
    got, n = regions.label(maps[3][:100, :130], renderer=r)
    wl, wn = ref.label(maps[3][:100, :130], 8)
    assert n == wn and got.dtype == np.int32 and np.array_equal(got, wl)
    got4, n4 = regions.label(maps[3][:100, :130].astype(np.uint8) * 7, connectivity=4, renderer=r)
    assert (n4, got4.tolist()) == (ref.label(maps[3][:100, :130], 4)[1], ref.label(maps[3][:100, :130], 4)[0].tolist())
    reg = regions.Regions.of(maps[3][:100, :130], renderer=r, first_guess=8)          # more regions than the first guess: the call is made again
    assert reg.n == wn > 8 and len(reg.table) == wn and reg.table.tobytes() == ref.rows_of(wl, wn, wn).tobytes()
    assert reg.counts == tuple(ref.counts_of(wl, wn).tolist()) and reg.largest() == reg.counts[3]
    for k in (1, reg.largest(), wn):
        ys, xs = reg.cells(k)
        wy, wx = np.nonzero(wl == k)
        assert np.array_equal(ys, wy) and np.array_equal(xs, wx)
    cells = [(0, 0), (129, 99), (130, 0), (-1, 5), (17, 44)]
    assert reg.label_at(cells).tolist() == [int(wl[0, 0]), int(wl[99, 129]), 0, 0, int(wl[44, 17])]
    rc.check_golden(lambda occ, scale, x_min, y_min: regions.semantic_map_items(occ, scale, x_min, y_min, renderer=r))


def test_clearance_map_free_regions_from_a_semantic_map(r, tmp_path):
    """ClearanceMap.free_regions and same_region end to end: the regions of d2 > the inflation limit on the reference's grown grid, and
    pairs of positions, against the restatement and against the geodesic field (a finite field iff one region)."""
    import clearance_cases as cc
    from sage_gs.clearance import ClearanceMap
    e = cc.golden()["maps"][0]
    m = ClearanceMap.from_semantic_map(cc.write_golden_map(e, tmp_path), robot_radius_m=0.1, scale=e["scale"], renderer=r)
    free = m.obstacle_map == 0
    wl, wn = ref.label(free, 8)
    reg = m.free_regions()
    assert reg is m.free_regions() and reg.n == wn and np.array_equal(reg.labels_host(), wl)
    cells = geodesic_ref.seeded_free_cells(free, 6, seed=1) + geodesic_ref.seeded_free_cells(~free, 30, seed=2)      # six grown-obstacle cells, thirty free ones
    sx, sy = m.min_x + m.max_x, m.min_y + m.max_y                                   # map (x, y) -> the caller's frame, as the checks map back
    xy = np.array([[m.min_x + i * m.scale - sx, m.min_y + j * m.scale - sy, 0.5] for i, j in cells])
    assert m.cells_of(xy).tolist() == [list(c) for c in cells]
    a, b = xy[:-1], xy[1:]
    want = [wl[j0, i0] != 0 and wl[j0, i0] == wl[j1, i1] for (i0, j0), (i1, j1) in zip(cells[:-1], cells[1:])]
    assert m.same_region(a, b).tolist() == want and any(want) and not all(want)
    goal = cells[-1]
    steps = m.geodesic_field(xy[-1:]).steps
    reached = steps[..., 0] != geodesic_ref.NONE
    assert np.array_equal(reached, wl == wl[goal[1], goal[0]])
    outside = np.array([[1.0e6, 0.0]])
    assert m.same_region(outside, xy[-1:, :2]).tolist() == [False]
