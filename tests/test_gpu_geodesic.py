"""The geodesic field and its paths on the MI355X (sgs_geodesic_field, sgs_geodesic_path): geodesic_cases' pictures, batches, sources,
schedules, paths, the reference's own recorded answers and the refusals through device pointers, at the emulator's small shapes; one
512 x 512 map of rooms joined by doors with 8 goals against the restatement; and the layers above the C ABI — Renderer.geodesic_field
driving the CONTINUE loop, sage_gs.geodesic.GeodesicField, ClearanceMap.geodesic_field from a semantic-map JSON, geodesic.astar_pixel.
Every comparison is exact.  Neither SciPy nor the reference's tree is used here: its answers come from tests/golden/geodesic_golden.json."""
import numpy as np
import pytest

import geodesic_cases as gc
import geodesic_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    from sage_gs import Renderer
    rr = Renderer("cuda:0")
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def drv(r):
    return gc.GpuGeodesic(r)


@pytest.fixture(scope="session")
def rooms_512():
    """(blocked, goals, the restatement's field per goal), computed once."""
    ob = ref.rooms_with_doors(512)
    goals = ref.seeded_free_cells(ob, 8, seed=4)
    return ob, goals, [ref.field(ob, [g]) for g in goals]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_sizes_on_the_gpu(drv):
    gc.check_sizes(drv)


def test_pictures_and_the_serpentine_on_the_gpu(drv):
    gc.check_pictures(drv, gc.pictures(drv.T))
    gc.check_serpentine_needs_continue(drv)


def test_schedule_independence_on_the_gpu(drv):
    gc.check_schedule_independence(drv)


def test_batches_and_sources_on_the_gpu(drv):
    gc.check_batches(drv)
    gc.check_sources(drv)


def test_paths_on_the_gpu(drv):
    gc.check_paths(drv)


def test_the_references_own_answers_on_the_gpu(drv):
    gc.check_golden(drv)


def test_refusals_on_the_gpu(drv):
    gc.check_refusals(drv)


def test_eight_goals_on_rooms_with_doors_512(r, rooms_512):
    import torch
    ob, goals, want = rooms_512
    src = torch.from_numpy(ob).to(r.device)
    steps, blocked = r.geodesic_field(src, [(f,) + g for f, g in enumerate(goals)], field_map=[0] * 8)
    assert steps.shape == (8, 512, 512, 2) and steps.dtype == torch.int32 and blocked.tolist() == [0] * 8
    got = _u32(steps)
    for f in range(8):
        diff = np.nonzero((got[f] != want[f]).any(-1))
        assert len(diff[0]) == 0, f"goal {f}: {len(diff[0])} cells differ from the restatement, first (i, j) = {(int(diff[1][0]), int(diff[0][0]))}"
    assert int((want[0][..., 0] != ref.NONE).sum()) == int((~ob).sum())              # every free cell reaches the goal through the doors
    starts = ref.seeded_free_cells(ob, 64, seed=9)
    q = [(f, i, j) for f in range(8) for i, j in starts[8 * f:8 * f + 8]]
    longest = max(int(want[f][j, i].astype(np.int64).sum()) + 1 for f, i, j in q)
    cells, info = r.geodesic_path(src, steps, q, field_map=[0] * 8, max_len=longest)
    cells, info = cells.cpu().numpy(), info.cpu().numpy()
    for (f, i, j), c, n in zip(q, cells, info):
        path, status = ref.path(ob, want[f], (i, j))
        assert n.tolist() == [len(path), status] and [tuple(v) for v in c[:n[0]].tolist()] == path


def test_renderer_drives_the_continue_loop_on_the_serpentine(r, drv):
    import torch
    ob, seeds = gc.serpentine(drv.T)
    src = torch.from_numpy(ob).to(r.device)
    sd = [(0,) + s for s in seeds]
    steps, blocked = r.geodesic_field(src, sd)
    dflt = gc.default_rounds(drv.T, ob.shape[1], ob.shape[0])
    assert r.last_geodesic_rounds > dflt and r.last_geodesic_rounds % dflt == 0 and blocked.tolist() == [0]
    gc.check_field("serpentine through the Renderer", _u32(steps)[0], ob, seeds)
    one, _ = r.geodesic_field(src, sd, rounds=1)
    assert torch.equal(one, steps) and dflt < r.last_geodesic_rounds < ob.size
    as_d2, _ = r.geodesic_field(torch.from_numpy(np.where(ob, 3, 4).astype(np.int32)).to(r.device), sd, max_d2=3)
    assert torch.equal(as_d2, steps)
    for bad in (dict(src=src.float()), dict(src=src, max_d2=1), dict(src=src.cpu()), dict(src=src.to(torch.int32)), dict(src=src, rounds=0), dict(src=src, seeds=[])):
        with pytest.raises(ValueError):
            r.geodesic_field(bad.pop("src"), bad.pop("seeds", sd), **bad)
    from sage_gs import SgsError
    with pytest.raises(SgsError, match="outside the grid"):
        r.geodesic_field(src, [(0, ob.shape[1], 0)])


def test_clearance_map_geodesic_field_from_a_semantic_map(r, tmp_path):
    """ClearanceMap.geodesic_field end to end: the field on the reference's grown grid_map (d2 <= the inflation limit), from goals given
    as positions; distances in cells and metres; paths."""
    import clearance_cases as cc
    from sage_gs.clearance import ClearanceMap
    e = cc.golden()["maps"][0]
    m = ClearanceMap.from_semantic_map(cc.write_golden_map(e, tmp_path), robot_radius_m=0.1, scale=e["scale"], renderer=r)
    ob = m.obstacle_map != 0
    goals = [(5, 5), (40, 30)]
    assert not ob[5, 5] and not ob[30, 40]
    sx, sy = m.min_x + m.max_x, m.min_y + m.max_y                                   # map (x, y) -> the caller's frame: x3d = x2d - (min + max)
    xy = [[m.min_x + i * m.scale - sx, m.min_y + j * m.scale - sy, 0.5] for i, j in goals]
    assert m.cells_of(xy).tolist() == [list(g) for g in goals]
    f = m.geodesic_field(xy)
    want = ref.field(ob, goals)
    assert f.goal_cells == goals and f.blocked_goals == 0 and np.array_equal(f.steps, want)
    assert np.array_equal(f.distance_cells(), ref.distance_cells(want)) and np.array_equal(f.distance_m(), ref.distance_cells(want) * e["scale"])
    starts = ref.seeded_free_cells(ob, 20, seed=2) + [(0, 0), (-1, 3), (ob.shape[1], 3)]
    for s, p in zip(starts, f.paths(starts)):
        inside = 0 <= s[0] < ob.shape[1] and 0 <= s[1] < ob.shape[0]
        cells, status = ref.path(ob, want, s) if inside else ([], ref.PATH_INVALID)
        assert p == (cells if status == ref.PATH_OK else None), s
    assert f.path(goals[0]) == [goals[0]] and f.path((0, 0)) is None


def test_geodesic_field_and_astar_pixel_on_the_golden_pairs(r):
    """Every recorded pair through GeodesicField.from_mask and .paths; the first three starts of every goal through the drop-in
    astar_pixel itself (one field and one path a call)."""
    from sage_gs import geodesic
    fields = {}

    def field_of(ob, goal):
        fields[goal] = geodesic.GeodesicField.from_mask(ob, [goal], renderer=r)
        return fields[goal].steps

    gc.check_golden(field_of=field_of, path_of=lambda ob, fld, goal, starts: fields[goal].paths(starts))
    for e in gc.golden()["grids"]:
        ob = gc.golden_grid(e)
        grid = ob.astype(np.uint8)
        for g in e["goals"]:
            goal = tuple(g["goal"])
            for p in g["pairs"][:3]:
                mine = geodesic.astar_pixel(grid, tuple(p["start"]), goal, renderer=r)
                if p["path"] is None:
                    assert mine is None
                else:
                    theirs = gc.decode_path(p["start"], p["path"])
                    assert mine[0] == theirs[0] and mine[-1] == goal and ref.count_steps(mine) == ref.count_steps(theirs)
                    assert all(isinstance(c, tuple) and not ob[c[1], c[0]] for c in mine)
    blocked = np.argwhere(gc.golden_grid(gc.golden()["grids"][0]))[0]
    assert geodesic.astar_pixel(gc.golden_grid(gc.golden()["grids"][0]), (int(blocked[1]), int(blocked[0])), (5, 5), renderer=r) is None      # the stated departure
