"""GPU: the 2-D and the 3-D route are two instances of one engine (csrc/densemap_route_core.hpp), and a handle owns one of each.  What
sharing the code could break is state that belongs to one instance and is used by the other: a static, or a buffer sized for pairs
and used for triples.  So one handle runs, interleaved: route_cells on a 33 x 34 grid (two tiles per axis, a remainder of 1 and 2),
route3_cells on a 9 x 10 x 17 plane (a remainder of 1 and 2 cells beyond a brick in x and y, three bricks in z), route_trace from every
cell of the grid, route3_trace from every cell of the plane, frontiers_cells with a start (which routes again through the 2-D
instance) and route3_trace once more, which must give what it gave before.  Every field, stats[0:4] and every route is the bytes of
the models' (tests/densemap_route_model.py, tests/densemap_route3_model.py, tests/densemap_frontier_model.py), no tolerance anywhere.
The layouts are checked on the CPU: a reachable cell in every tile and brick, and traversable cells that no route reaches."""
import numpy as np
import pytest

import densemap_frontier_model as fm
import densemap_grid_model as gm
import densemap_route3_model as r3
import densemap_route_model as rm
from loam_velodyne_amd import loamx

LEAF = 0.5
NX2, NZ2 = 33, 34
NX3, NY3, NZ3 = 9, 10, 17
GOALS2, GOALS3 = [(0, 0)], [(0, 0, 0)]
START2 = (31, 2)         # of the frontier call: beyond the wall from the goal
CAP2, CAP3 = 48, 12      # shorter than the longest route of either field: some routes come back truncated
PAIRS = [(4, 6), (8, 18), (4, 26), (8, 26)]    # (2-D, 3-D) connectivity: both of the one, all three of the other


def grid():
    """33 x 34: a wall with a gap at its far end, a diagonal wall (the corner rule), a closed box with a free inside that nothing
    reaches, and a patch of UNKNOWN cells (blocked for the route, frontiers for the frontier call)"""
    cls = np.full((NZ2, NX2), gm.FREE)
    cls[0:30, 10] = gm.OBSTACLE
    for i in range(6):
        cls[20 + i, 3 + i] = gm.OBSTACLE
    cls[5:10, 20:25] = gm.OBSTACLE
    cls[6:9, 21:24] = gm.FREE
    cls[15:19, 27:31] = gm.UNKNOWN
    return rm.cells_of(cls)


def plane():
    """9 x 10 x 17: a floor at z = 5 that leaves only the column x = 8 open, a closed shell with one open cell inside that nothing
    reaches, and blocked cells scattered by a fixed seed; d2 varies, so that the soft weights act"""
    rng = np.random.default_rng(3)
    d2 = rng.integers(1, 30, size=(NZ3, NY3, NX3)).astype(np.uint16)
    d2[rng.random((NZ3, NY3, NX3)) < 0.08] = 0
    d2[5, :, 0:8] = 0
    d2[5, :, 8] = 9
    d2[10:13, 2:5, 2:5] = 0
    d2[11, 3, 3] = 9
    d2[0, 0, 0] = 9
    return d2


CFG3 = dict(soft_d2=25, soft_weight=9)
_cache = {}


def model2(conn):
    if ("2", conn) not in _cache:
        cells, cfg = grid(), dict(connectivity=conn)
        f = rm.field(cells, cfg, GOALS2)
        starts = [(x, z) for z in range(NZ2) for x in range(NX2)]
        _cache[("2", conn)] = (f, rm.stats(cells, cfg, GOALS2, f), starts, [rm.trace(f, s, CAP2) for s in starts])
    return _cache[("2", conn)]


def model3(conn):
    if ("3", conn) not in _cache:
        d2, cfg = plane(), dict(CFG3, connectivity=conn)
        f = r3.field(d2, cfg, GOALS3)
        starts = [(x, y, z) for z in range(NZ3) for y in range(NY3) for x in range(NX3)]
        _cache[("3", conn)] = (f, r3.stats(d2, cfg, GOALS3, f), starts, [r3.trace(f, s, CAP3) for s in starts])
    return _cache[("3", conn)]


def frontier_model(conn):
    if ("f", conn) not in _cache:
        _cache[("f", conn)] = fm.frontiers(grid(), dict(connectivity=conn), dict(connectivity=conn), START2)
    return _cache[("f", conn)]


@pytest.mark.parametrize("conn2,conn3", PAIRS)
def test_the_layouts_reach_every_tile_and_brick_and_leave_cells_unreached(conn2, conn3):
    f2, st2, starts2, want2 = model2(conn2)
    reach2 = f2["cost"] != rm.UNREACHABLE
    assert all(reach2[z:z + 32, x:x + 32].any() for z in range(0, NZ2, 32) for x in range(0, NX2, 32))
    assert st2[1] < st2[0] < NX2 * NZ2 and st2[2] == 1 and not reach2[7, 22] and rm.weight(grid())[7][22] > 0
    assert len(starts2) == 1122 <= 4096 and max(n for _, n in want2) > CAP2 and sum(1 for _, n in want2 if n) == st2[1]
    f3, st3, starts3, want3 = model3(conn3)
    reach3 = f3["cost"] != r3.UNREACHABLE
    assert all(reach3[z:z + 8, y:y + 8, x:x + 8].any() for z in range(0, NZ3, 8) for y in range(0, NY3, 8) for x in range(0, NX3, 8))
    assert st3[1] < st3[0] < NX3 * NY3 * NZ3 and st3[2] == 1 and not reach3[11, 3, 3] and plane()[11, 3, 3] > 0
    assert len(starts3) == 1530 and max(n for _, n in want3) > CAP3 and sum(1 for _, n in want3 if n) == st3[1]
    out, _, fstats, ffield = frontier_model(conn2)
    assert len(out) >= 1 and fstats[4] >= 1 and ffield.tobytes() != f2.tobytes()    # frontiers, some reached; another field than the goals'


@pytest.fixture(scope="module")
def handle():
    return loamx.DenseMap(leaf=LEAF, initial_slots=1024)    # an empty map: the *_cells calls need a handle, not its voxels


def stats4(st):
    return (st["traversable"], st["reachable"], st["goals_used"], st["max_cost"])


def same_routes(got, want):
    routes, lengths = got
    assert len(routes) == len(lengths) == len(want)
    for i, (w, n) in enumerate(want):
        assert lengths[i] == n and routes[i].tobytes() == w.tobytes(), i


@pytest.mark.gpu
@pytest.mark.parametrize("conn2,conn3", PAIRS)
def test_the_two_instances_interleaved_on_one_handle(handle, conn2, conn3):
    d = handle
    f2, st2, starts2, want2 = model2(conn2)
    f3, st3, starts3, want3 = model3(conn3)
    got2 = d.route_cells(grid(), GOALS2, connectivity=conn2)                       # 1
    assert got2.dtype == rm.ROUTE_CELL and got2.shape == f2.shape and got2.tobytes() == f2.tobytes()
    assert stats4(d.route_stats) == st2
    got3 = d.route3_cells(plane(), GOALS3, connectivity=conn3, **CFG3)             # 2
    assert got3.dtype == r3.ROUTE_CELL and got3.shape == f3.shape and got3.tobytes() == f3.tobytes()
    assert stats4(d.route3_stats) == st3 and stats4(d.route_stats) == st2
    same_routes(d.route_trace(starts2, CAP2), want2)                                # 3
    first3 = d.route3_trace(starts3, CAP3)                                          # 4
    same_routes(first3, want3)
    w_out, w_lab, w_stats, _ = frontier_model(conn2)                                # 5
    lab, out = d.frontiers_cells(grid(), start=START2, route=loamx.RouteConfig(connectivity=conn2), connectivity=conn2)
    assert out.dtype == fm.FRONTIER and out.tobytes() == w_out.tobytes()
    assert lab.dtype == np.uint32 and lab.shape == w_lab.shape and lab.tobytes() == w_lab.tobytes()
    assert tuple(d.frontier_stats[k] for k in loamx.FRONTIER_STATS[:5]) == w_stats
    again3 = d.route3_trace(starts3, CAP3)                                          # 6
    same_routes(again3, want3)
    assert again3[1].tobytes() == first3[1].tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(again3[0], first3[0]))
