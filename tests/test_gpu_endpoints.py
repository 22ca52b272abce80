"""The item endpoints on the MI355X (sgs_endpoints): endpoints_cases' sizes, word seams, search distances, shapes, the entry limit,
flagged items, sources, batches, the short work with its retry, the reference's recorded answers and the refusals through device
pointers, at the emulator's small shapes; one 512 x 512 map with 64 items and 2 000 queries against the restatement; and the layers
above the C ABI — Renderer.endpoints, sage_gs.trajectory (ItemSet, nearest_free, nearest_free_pixel_on_side, connectivity_map,
plan_pairs, validate_and_generate_path) and ClearanceMap.nearest_free from a semantic-map JSON.  Every comparison is exact.  The
reference's tree is not used here: its answers come from tests/golden/endpoints_golden.json."""
import json

import numpy as np
import pytest

import endpoints_cases as ec
import endpoints_ref as ref
import geodesic_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    from sage_gs import Renderer
    rr = Renderer("cuda:0")
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def drv(r):
    return ec.GpuEndpoints(r)


def test_sizes_on_the_gpu(drv):
    ec.check_sizes(drv)


def test_seams_and_search_distances_on_the_gpu(drv):
    ec.check_word_seams(drv)
    ec.check_max_dist(drv)


def test_shapes_and_the_whole_grid_on_the_gpu(drv):
    ec.check_shapes(drv)
    ec.check_whole_grid(drv)


def test_the_entry_limit_and_flagged_items_on_the_gpu(drv):
    ec.check_entry_limit(drv)
    ec.check_flagged_items(drv)


def test_sources_batches_and_the_short_work_on_the_gpu(drv):
    ec.check_sources(drv)
    ec.check_batches(drv)
    ec.check_short_work(drv)


def test_the_references_answers_on_the_gpu(drv):
    ec.check_golden_drv(drv)


def test_refusals_on_the_gpu(drv):
    ec.check_refusals(drv)


def test_64_items_and_2000_queries_on_a_512_map(r):
    """Rooms with doors under seeded clutter that leaves 3 % of the cells free, 64 items — rectangles of seeded sizes, every fourth with
    duplicates, every fourth one cell —, 2 000 seeded queries, a quarter of them without a target: Renderer.endpoints — which owns the
    scratch and its retry — against the restatement, every field.  By the restatement about half the answers lie off the item (d > 0),
    more than 1 000 are forced and more than 800 are ties."""
    import torch
    from sage_gs import _capi
    nx = ny = 512
    rs = np.random.RandomState(64)
    blocked = geodesic_ref.rooms_with_doors(512) | (rs.rand(ny, nx) < 0.97)
    items = []
    for k in range(64):
        w, h = (1, 1) if k % 4 == 1 else (int(rs.randint(1, 40)), int(rs.randint(1, 40)))
        x0, y0 = int(rs.randint(0, nx - w + 1)), int(rs.randint(0, ny - h + 1))
        cells = ec.rect(nx, x0, y0, x0 + w, y0 + h)
        items.append(np.concatenate([cells, cells[:len(cells) // 3]]) if k % 4 == 0 else cells)
    q = np.stack([rs.randint(0, 64, 2000), rs.randint(0, nx, 2000), rs.randint(0, ny, 2000), (rs.rand(2000) < 0.75).astype(np.int64)], 1)
    offsets, cells = ec.csr(items)
    rows, answers, counts = r.endpoints(torch.from_numpy(blocked).to(r.device), (offsets.astype(np.int64), cells), q)
    assert rows.shape == (64, 14) and answers.shape == (2000, 4) and counts.shape == (4,)
    got = (rows.cpu().numpy().reshape(-1).view(_capi.ENDPOINTS_ITEM_DTYPE), answers.cpu().numpy().reshape(-1).view(_capi.ENDPOINTS_ANSWER_DTYPE),
           [int(v) for v in counts.cpu().tolist()])
    queries = [tuple(int(v) for v in row) for row in q]
    ec.check_call("512 x 512", got, blocked.astype(np.uint8), items, queries)
    assert got[2][0] > 1500 and (got[1]["n_at_d"] == 1).sum() > 1000 and (got[1]["n_at_d"] > 1).sum() > 800 and (got[1]["d"] > 0).sum() > 900


def test_renderer_endpoints_arguments(r):
    import torch
    mask, items, queries = ec.shapes_scene(64)
    offsets, cells = ec.csr(items)
    m = torch.from_numpy(mask).to(r.device)
    it = (torch.from_numpy(offsets.astype(np.int32)).to(r.device), torch.from_numpy(cells).to(r.device))
    rows, answers, counts = r.endpoints(m, it, queries)
    want = ref.endpoints(mask, items, queries)
    assert rows.cpu().numpy().tobytes() == want[0].tobytes() and answers.cpu().numpy().tobytes() == want[1].tobytes() and counts.cpu().tolist() == want[2]
    as_d2 = r.endpoints(torch.where(m != 0, 3, 9).to(torch.int32), it, queries, max_d2=3)[1]
    assert torch.equal(as_d2, answers)
    none, a0, c0 = r.endpoints(m, it, [])
    assert torch.equal(none, rows) and a0.shape == (0, 4) and c0.cpu().tolist()[:3] == [0, 0, 0]
    for bad in (dict(src=m.float()), dict(src=m.cpu()), dict(src=m, max_dist=64), dict(src=m, max_dist=-1), dict(src=m, max_d2=1), dict(src=m, source="topdown"),
                dict(src=m[None])):
        with pytest.raises(ValueError):
            r.endpoints(bad.pop("src"), it, queries, **bad)


def test_the_trajectory_module_against_the_reference(r, tmp_path):
    """From a semantic-map JSON written to tmp_path: ClearanceMap.obstacle_map is build_2d_map's grid; ItemSet's centroids, the
    drop-in, the batch form on the grid and on the clearance map, the connectivity groups, and the whole dict of
    validate_and_generate_path for the pairs whose endpoints are forced."""
    from sage_gs import trajectory
    from sage_gs.clearance import ClearanceMap
    n_path = n_none = 0
    for s in ec.golden()["scenes"]:
        path = tmp_path / (s["name"] + ".json")
        path.write_text(json.dumps(s["instances"]))
        grid = ec.golden_grid(s)
        m = ClearanceMap.from_semantic_map(str(path), robot_radius_m=s["robot_radius_m"], scale=s["scale"], renderer=r)
        assert np.array_equal(m.obstacle_map, grid), f"{s['name']}: the obstacle map differs from the reference's grid"
        assert [m.min_x, m.min_y] == s["min"]
        inst = ec.golden_inst(s)
        items = trajectory.ItemSet.from_instances(inst, grid.shape, renderer=r)
        for name, it in s["items"].items():
            assert list(items.centroid(name)) == it["centroid"] and int(items.rows["boundary"][items.index[name]]) == it["n_boundary"], name
        # the batch form on the grid and on the clearance map, against the recorded queries
        names = [q["item"] for q in s["queries"]]
        towards = [q["towards"] for q in s["queries"]]
        on_grid = trajectory.nearest_free(items, grid, towards, names)
        on_map = m.nearest_free(items, towards, names)
        assert on_grid.tobytes() == on_map.tobytes()
        for q, a in zip(s["queries"], on_grid):
            assert (q["answer"] is None) == (int(a["d"]) < 0) and (q["answer"] is None or int(a["d"]) == q["d"])
            if int(a["n_at_d"]) == 1:
                assert [int(a["x"]), int(a["y"])] == q["answer"]
        # the drop-in, one query at a time, on a few
        for q in s["queries"][::37]:
            got = trajectory.nearest_free_pixel_on_side(inst[q["item"]]["mask_coords"], grid, None if q["towards"] is None else tuple(q["towards"]), renderer=r)
            k = s["queries"].index(q)
            assert got == (None if int(on_grid["d"][k]) < 0 else (int(on_grid["x"][k]), int(on_grid["y"][k])))
        groups = trajectory.connectivity_map(grid, inst, renderer=r)
        assert {frozenset(g) for g in groups.values()} == {frozenset(g) for g in s["connectivity"]}
        flat = sorted(s["connectivity"])
        if len(flat) > 1:
            assert trajectory.are_items_connected(flat[0][0], flat[0][-1], groups) and not trajectory.are_items_connected(flat[0][0], flat[1][0], groups)
        got = trajectory.plan_pairs([(p["start"], p["end"]) for p in s["pairs"]], inst, grid, s["scale"], s["min"][0], s["min"][1], renderer=r)
        for p, g in zip(s["pairs"], got):
            assert g == p["result"], f"{s['name']}: {p['start']} -> {p['end']}: the trajectory differs from the reference's"
            n_path += g is not None
            n_none += g is None
        for p in s["pairs"][:2]:
            assert trajectory.validate_and_generate_path(p["start"], p["end"], inst, grid, s["scale"], s["min"][0], s["min"][1], renderer=r) == p["result"]
        assert trajectory.validate_and_generate_path("no_such_item", names[0], inst, grid, s["scale"], s["min"][0], s["min"][1], renderer=r) is None
    assert n_path >= 20 and n_none >= 5
