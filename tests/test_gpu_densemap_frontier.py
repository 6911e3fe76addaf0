"""GPU: frontiers of the navigation grid (include/loamx.h, loamx_densemap_frontiers and what goes with it) against their model
(tests/densemap_frontier_model.py).  Every comparison is the bytes of the record array and of the label array against the model's, no
tolerance anywhere, and stats[0:5] equal the model's; stats[5], hook attempts lost, describes the schedule and is printed.  The shapes
are the smallest at which a 32 x 32 tiling with a halo of one (k_dm_fr_mark, k_dm_fr_link) can go wrong.  Through the map: the 541-voxel
box scene of tests/test_gpu_densemap_grid.py."""
import ctypes as C

import numpy as np
import pytest

import densemap_carve_model as cm
import densemap_frontier_model as fm
import densemap_grid_model as gm
import densemap_raycast_model as rcm
import densemap_route_model as rm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

LEAF = 0.5
BASE = dict(min_points=1, band_lo=1, band_hi=4, max_step=1, clear_max=3)    # of tests/test_gpu_densemap_grid.py
K1 = dict(cell_leaves=1, x0=-8, z0=-5, nx=17, nz=11)                         # of tests/test_gpu_densemap_route.py
W37 = dict(cell_leaves=1, x0=-18, z0=-26, nx=37, nz=53)
SOFT = dict(soft_clear2=25, soft_weight=9)
SENTINEL = 0xABABABAB

# name -> (cells, configuration beside the connectivity)
CASES = {
    "1x1_free": (lambda: fm.filled(1, 1, gm.FREE), {}),
    "1x1_unknown": (lambda: fm.filled(1, 1, gm.UNKNOWN), {}),
    "1x70": (lambda: fm.runs(1, 70), {}),
    "70x1": (lambda: fm.runs(70, 1), {}),
    "32x32": (lambda: fm.square(32, 32, 0, 0, 31), {}),                       # one tile exactly; the square touches two window edges
    "33x31": (lambda: fm.square(33, 31, 1, 1, 29), {}),                       # a one-cell second tile column and a short tile
    "square_on_the_corner": (lambda: fm.square(70, 70, 22, 22, 20), {}),      # one closed loop through four tiles
    "staircase": (lambda: fm.staircase(70, 20, 45), {}),                      # through the tile corner by corners only
    "spiral": (lambda: fm.spiral(70, 45), {}),                                # one frontier that re-enters the same tiles many times
    "combs": (lambda: fm.combs(), {}),                                        # the smallest index travels round each bend
    "all_free": (lambda: fm.filled(70, 70, gm.FREE), {}),                     # outside is not unknown
    "no_unknown": (lambda: fm.no_unknown(), {}),
    "narrow": (lambda: fm.narrow(3), dict(min_clear2=3)),
    "all_unknown": (lambda: fm.filled(70, 45, gm.UNKNOWN), {}),
    "random70": (lambda: fm.random70(), {}),
    "random70_unknown3": (lambda: fm.random70(), dict(min_unknown=3)),
    "random70_cells4": (lambda: fm.random70(), dict(min_cells=4)),
    "random70_clear6": (lambda: fm.random70(), dict(min_clear2=6)),
}
_cells, _model = {}, {}


def cells_of_case(name):
    if name not in _cells:
        _cells[name] = CASES[name][0]()
    return _cells[name]


def model_of(name, conn):
    """(records, labels, stats[0:5]) of a case, computed once"""
    if (name, conn) not in _model:
        _model[(name, conn)] = fm.frontiers(cells_of_case(name), dict(CASES[name][1], connectivity=conn))[:3]
    return _model[(name, conn)]


def explain(got, want):
    if len(got) != len(want):
        return f"{len(got)} records, want {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g.tobytes() != w.tobytes():
            return f"record {i}: got {g}, want {w}"
    return "equal"


def check(d, got, want):
    """(labels, records) of a call against the model's (records, labels, stats)"""
    lab, out = got
    w_out, w_lab, w_stats = want
    st = d.frontier_stats
    print("stats", st)
    assert out.dtype == fm.FRONTIER and out.tobytes() == w_out.tobytes(), explain(out, w_out)
    assert lab.dtype == np.uint32 and lab.shape == w_lab.shape and lab.tobytes() == w_lab.tobytes(), np.argwhere(lab != w_lab)[:4]
    assert tuple(st[k] for k in loamx.FRONTIER_STATS[:5]) == w_stats


@pytest.fixture(scope="module")
def handle():
    return loamx.DenseMap(leaf=LEAF, initial_slots=1024)    # an empty map: frontiers_cells needs a handle, not its voxels


# ---- 1: the shapes x connectivity 4 and 8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(CASES))
def test_frontiers_equal_the_model(handle, name, conn):
    want = model_of(name, conn)
    check(handle, handle.frontiers_cells(cells_of_case(name), connectivity=conn, **CASES[name][1]), want)
    stats = want[2]
    if name in ("1x1_free", "1x1_unknown", "all_free", "no_unknown", "all_unknown"):
        assert stats == (0, 0, 0, 0, 0)
    if name == "square_on_the_corner":
        assert stats == (76, 1, 1, 76, 0) and want[0][0]["unknown_links"] == 12 * 18 + 20
    if name == "staircase":
        assert stats[:3] == ((26, 1, 1) if conn == 8 else (26, 26, 26))
    if name == "spiral":
        assert stats[1:3] == (1, 1) and want[0][0]["cells"] == stats[0] == int((cells_of_case(name)["cls"] == gm.FREE).sum())
    if name == "combs":
        assert stats == (812, 2, 2, 812, 0)
    if name == "narrow":
        assert stats == (2, 2, 2, 2, 0)
    if name in ("1x70", "70x1"):
        assert stats == (23, 23, 23, 23, 0)


def test_the_parameters_act():
    for conn in (4, 8):
        variants = [model_of(n, conn) for n in ("random70", "random70_unknown3", "random70_cells4", "random70_clear6")]
        assert len({v[0].tobytes() + v[1].tobytes() for v in variants}) == 4
    assert model_of("random70", 4)[0].tobytes() != model_of("random70", 8)[0].tobytes()


# ---- 2: with a start: the cost words and the trace ------------------------------------------------------------------------------------------
def with_start(d, cells, start, cfg=None, route=None):
    want = fm.frontiers(cells, cfg, route, start)
    got = d.frontiers_cells(cells, start=start, route=loamx.RouteConfig(**(route or {})), **(cfg or {}))
    check(d, got, want[:3])
    return got[1], want


@pytest.mark.parametrize("conn", [4, 8])
def test_costs_on_random70(handle, conn):
    cells = fm.random70()
    start = tuple(int(v) for v in np.argwhere((cells["cls"] == gm.FREE) & (cells["clear2"] >= 1))[1200][::-1])    # a FREE cell, (rx, rz)
    out, want = with_start(handle, cells, start, dict(connectivity=conn), dict(SOFT, connectivity=conn))
    assert want[2][4] >= 1 and int((out["reachable"] > 0).sum()) == want[2][4] and int((out["best_cost"] != rm.UNREACHABLE).sum()) == want[2][4]
    # without the penalties the cost words differ: the route configuration is used
    assert fm.frontiers(cells, dict(connectivity=conn), dict(connectivity=conn), start)[0].tobytes() != want[0].tobytes()


def test_a_tie_goes_to_the_smaller_index(handle):
    out, _ = with_start(handle, fm.square(21, 21, 5, 5, 11), (10, 10))
    assert (out[0]["best_cost"], out[0]["best_cell"], out[0]["reachable"]) == (50, 5 * 21 + 10, 40)


def test_behind_a_wall_outside_and_on_an_obstacle(handle):
    cells = fm.walled()
    out, want = with_start(handle, cells, (5, 5))
    assert out["reachable"].tolist() == [out[0]["cells"], 0] and (out[1]["best_cost"], out[1]["best_cell"]) == (rm.UNREACHABLE, fm.NONE)
    assert handle.frontier_stats["kept_reachable"] == 1 and loamx.frontiers_best(out) == 0
    for start in ((40, 5), (2 ** 32 - 1, 0), (19, 5)):    # outside the window; on the wall: LOAMX_OK, nothing reachable
        out, _ = with_start(handle, cells, start)
        assert len(out) == 2 and np.all(out["reachable"] == 0) and np.all(out["best_cost"] == rm.UNREACHABLE) and np.all(out["best_cell"] == fm.NONE)
        assert handle.frontier_stats["kept_reachable"] == 0 and loamx.frontiers_best(out) == fm.NONE


def test_trace_from_the_best_cell_ends_on_the_start(handle):
    cells = fm.random70()
    start = (35, 34)
    assert cells["cls"][34, 35] == gm.FREE
    out, want = with_start(handle, cells, start, dict(connectivity=4), SOFT)    # 187 frontiers, 43 of them reachable
    assert loamx.frontiers_best(out) != fm.NONE and out[loamx.frontiers_best(out)]["best_cost"] == 0    # the one the start stands on
    pick = loamx.frontiers_best(out, 1)
    assert pick != fm.NONE and pick == fm.best(want[0], 1)
    cell = int(out[pick]["best_cell"])
    routes, lengths = handle.route_trace([(cell % 70, cell // 70)], 4900)
    w_route, w_len = rm.trace(want[3], (cell % 70, cell // 70))
    assert lengths[0] == w_len > 1 and routes[0].tobytes() == w_route.tobytes() and routes[0][-1].tolist() == list(start)
    field = want[3]
    assert field[cell // 70, cell % 70]["cost"] == out[pick]["best_cost"] and field[34, 35]["next"] == rm.GOAL


# ---- 3: through the map ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    S = rcm.box_cast_scene()
    S["model"] = cm.CarveModel(leaf=LEAF)
    S["map"] = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
    S["map"].enable_carving()
    for p, o in S["sweeps"]:
        S["model"].add(p, o)
        assert S["map"].add(p, o) in (loamx.OK, True)
    assert len(S["model"]) == len(S["map"]) == 541
    return S


def exports(d):
    st = d.stats()
    st.pop("slots")
    return dict(stats=st, points=d.points().tobytes(), misses=d.misses().tobytes(), carve_stats=d.carve_stats())


@pytest.mark.parametrize("window", [K1, W37], ids=["K1", "W37"])
def test_through_the_map(scene, window):
    d = scene["map"]
    cfg = dict(BASE, **window)
    before = exports(d)
    grid_before = d.grid(loamx.GridConfig(**cfg))
    cells = gm.grid(scene["model"], None, **cfg)
    assert grid_before.tobytes() == cells.tobytes()
    # the box's floor is walled in: under BASE no FREE cell touches an UNKNOWN one and there is no frontier.  With walls that do not
    # count as obstacles (min_obstacle_voxels above their height) the box's rim is one frontier of 36 cells
    for extra, cells_want in ((dict(), 0), (dict(min_obstacle_voxels=50), 36)):
        g = dict(cfg, **extra)
        cells = gm.grid(scene["model"], None, **g)
        start = tuple(int(v) for v in np.argwhere(cells["cls"] == gm.FREE)[20][::-1])
        for conn in (4, 8):
            want = fm.frontiers(cells, dict(connectivity=conn), None, start)
            check(d, d.frontiers(grid=loamx.GridConfig(**g), start=start, connectivity=conn), want[:3])
            assert want[2] == ((36, 1, 1, 36, 1) if cells_want else (0, 0, 0, 0, 0))
            check(d, d.frontiers(grid=loamx.GridConfig(**g), connectivity=conn), fm.frontiers(cells, dict(connectivity=conn))[:3])
        rule = loamx.StaticRule(*cm.DEFAULT_RULE)
        check(d, d.frontiers(grid=loamx.GridConfig(**g), static=rule), fm.frontiers(gm.grid(scene["model"], cm.DEFAULT_RULE, **g))[:3])
    # every export of the map is byte for byte what it was, and grid returns the bytes it returned
    assert exports(d) == before and d.grid(loamx.GridConfig(**cfg)).tobytes() == grid_before.tobytes()


def test_without_a_start_the_field_is_left_alone(scene):
    d = scene["map"]
    cfg = dict(BASE, **K1)
    cells = gm.grid(scene["model"], None, **cfg)
    want = rm.field(cells, None, [(3, 2)])
    d.route([(3, 2)], grid=loamx.GridConfig(**cfg), want_field=False)
    d.frontiers(grid=loamx.GridConfig(**dict(BASE, **W37)))    # another window, no start
    d.frontiers_cells(fm.spiral(70, 45))
    starts = [(x, z) for z in range(K1["nz"]) for x in range(K1["nx"])]
    routes, lengths = d.route_trace(starts, 40)
    for s, r, n in zip(starts, routes, lengths):
        w, m = rm.trace(want, s)
        assert n == m and r.tobytes() == w.tobytes(), s
    assert int((lengths > 0).sum()) > 10


# ---- 4: housekeeping ------------------------------------------------------------------------------------------------------------------------
def test_large_then_small_window_and_the_same_call_twice():
    d = loamx.DenseMap(leaf=LEAF, initial_slots=1024)    # a handle of its own: its arrays have never been allocated
    big = fm.square(300, 200, 40, 30, 150)               # too large for the model in a quick test: the square's closed form
    lab, out = d.frontiers_cells(big)
    assert len(out) == 1 and out[0]["cells"] == 596 and out[0]["min_cell"] == 30 * 300 + 40 and out[0]["unknown_links"] == 12 * 148 + 20
    assert out[0]["lo"].tolist() == [40, 30] and out[0]["hi"].tolist() == [189, 179] and int((lab == 0).sum()) == 596
    assert out[0]["sum_rx"] == 596 * (40 + 189) // 2 and out[0]["sum_rz"] == 596 * (30 + 179) // 2
    for name in ("narrow", "spiral", "1x1_free", "combs"):
        for _ in range(2):
            check(d, d.frontiers_cells(cells_of_case(name), connectivity=8, **CASES[name][1]), model_of(name, 8))
    d.close()


def test_empty_map():
    d = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
    g = loamx.GridConfig(cell_leaves=1, nx=37, nz=53, clear_max=2)
    for start in (None, (1, 1)):
        lab, out = d.frontiers(grid=g, start=start)
        assert len(out) == 0 and np.all(lab == fm.NONE) and lab.shape == (53, 37)
        assert list(d.frontier_stats.values()) == [0] * 6 and len(d) == 0
    d.close()


def test_capacity(handle):
    L = loamx.lib()
    cells = cells_of_case("1x70")
    w_out, w_lab, w_stats = model_of("1x70", 8)
    cp = cells.ctypes.data_as(C.c_void_p)
    for cap in (0, 22):
        out = np.full(23 * 16, SENTINEL, np.uint32)
        lab = np.full(70, SENTINEL, np.uint32)
        stats = (C.c_uint64 * 6)(*[77] * 6)
        n = C.c_uint64(99)
        rc = L.loamx_densemap_frontiers_cells(handle.h, cp, 1, 70, None, None, None, lab.ctypes.data_as(C.c_void_p),
                                              out.ctypes.data_as(C.c_void_p), C.c_uint64(cap), C.byref(n), stats)
        assert rc == loamx.E_CAPACITY and n.value == 23
        assert np.all(out == SENTINEL) and np.all(lab == SENTINEL) and list(stats) == [77] * 6
    rc = L.loamx_densemap_frontiers_cells(handle.h, cp, 1, 70, None, None, None, lab.ctypes.data_as(C.c_void_p),
                                          out.ctypes.data_as(C.c_void_p), C.c_uint64(23), C.byref(n), stats)
    assert rc == loamx.OK and n.value == 23 and out.tobytes() == w_out.tobytes() and lab.tobytes() == w_lab.tobytes()
    assert tuple(stats[:5]) == w_stats
    # out NULL: no capacity is needed, the count and the labels still come
    lab[:] = SENTINEL
    rc = L.loamx_densemap_frontiers_cells(handle.h, cp, 1, 70, None, None, None, lab.ctypes.data_as(C.c_void_p), None, C.c_uint64(0),
                                          C.byref(n), stats)
    assert rc == loamx.OK and n.value == 23 and lab.tobytes() == w_lab.tobytes()


def test_refusals(scene):
    d, L = scene["map"], loamx.lib()
    plain = loamx.DenseMap(leaf=LEAF, initial_slots=1024)    # no carving
    before = exports(d)
    good = loamx.GridConfig(**dict(BASE, **K1))
    n_cells = good.nx * good.nz
    lab, out = np.full(n_cells, SENTINEL, np.uint32), np.full(64 * 16, SENTINEL, np.uint32)
    stats = (C.c_uint64 * 6)(*[77] * 6)
    n = C.c_uint64(99)
    lp, op, np_ = lab.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(n)
    start = np.array([3, 2], np.uint32)
    sp = start.ctypes.data_as(C.c_void_p)
    rc, fc, rule, bad_rule = loamx.RouteConfig(), loamx.FrontierConfig(), loamx.StaticRule(), loamx.StaticRule(den=0)
    own = rm.open(17, 11)
    own_bad = own.copy()
    own_bad["cls"][10, 16] = 4
    cp, cbp = own.ctypes.data_as(C.c_void_p), own_bad.ctypes.data_as(C.c_void_p)
    cap = C.c_uint64(64)

    def through(h=d.h, g=good, r=None, rcfg=rc, fcfg=fc, s=sp, nn=np_, st=stats):
        return L.loamx_densemap_frontiers(h, C.byref(g), C.byref(r) if r is not None else None, C.byref(rcfg), C.byref(fcfg), s, lp, op, cap, nn, st)

    def on_cells(h=d.h, c=cp, nx=17, nz=11, rcfg=rc, fcfg=fc, s=sp, nn=np_, st=stats):
        return L.loamx_densemap_frontiers_cells(h, c, nx, nz, C.byref(rcfg), C.byref(fcfg), s, lp, op, cap, nn, st)

    cases = [(lambda: through(h=None), b"h is NULL"), (lambda: through(nn=None), b"n_frontiers"), (lambda: through(st=None), b"stats"),
             (lambda: through(fcfg=fc.copy(connectivity=6)), b"connectivity"), (lambda: through(fcfg=fc.copy(min_unknown=0)), b"min_unknown"),
             (lambda: through(fcfg=fc.copy(min_unknown=9)), b"min_unknown"), (lambda: through(fcfg=fc.copy(min_clear2=0)), b"min_clear2"),
             (lambda: through(fcfg=fc.copy(min_cells=0)), b"min_cells"), (lambda: through(rcfg=rc.copy(soft_weight=16)), b"soft_weight"),
             (lambda: through(g=good.copy(nx=0)), b"nx"), (lambda: through(g=good.copy(clear_max=65)), b"clear_max"),
             (lambda: through(r=bad_rule), b"den"), (lambda: through(h=plain.h, r=rule), b"carving"),
             (lambda: through(g=good.copy(nx=2049, nz=2048)), b"nx * nz"),
             (lambda: on_cells(h=None), b"h is NULL"), (lambda: on_cells(nn=None), b"n_frontiers"), (lambda: on_cells(st=None), b"stats"),
             (lambda: on_cells(c=None), b"cells is NULL"), (lambda: on_cells(c=cbp), b"cls"),
             (lambda: on_cells(fcfg=fc.copy(connectivity=5)), b"connectivity"), (lambda: on_cells(rcfg=rc.copy(unknown_weight=17)), b"unknown_weight"),
             (lambda: on_cells(nx=2049, nz=2048), b"nx * nz"), (lambda: on_cells(nx=0), b"nx * nz"),
             (lambda: on_cells(nx=8193, nz=8192, s=None), b"nx * nz")]
    for call, word in cases:
        assert call() == loamx.E_INVALID and word in L.loamx_last_error(), (word, L.loamx_last_error())
        assert np.all(lab == SENTINEL) and np.all(out == SENTINEL) and list(stats) == [77] * 6 and n.value == 99
    # the handle is what it was, and the calls after a refusal are right: NULL configurations are the defaults
    assert exports(d) == before
    cells = gm.grid(scene["model"], None, **dict(BASE, **K1))
    w_out, w_lab, w_stats = fm.frontiers(cells, None, None, (3, 2))[:3]
    assert L.loamx_densemap_frontiers(d.h, C.byref(good), None, None, None, sp, lp, op, cap, np_, stats) == loamx.OK
    assert n.value == len(w_out) and out.tobytes()[:64 * len(w_out)] == w_out.tobytes() and lab.tobytes() == w_lab.tobytes()
    assert tuple(stats[:5]) == w_stats and np.all(out[16 * len(w_out):] == SENTINEL)
    assert L.loamx_densemap_frontiers(d.h, C.byref(good), None, None, None, None, None, None, C.c_uint64(0), np_, stats) == loamx.OK
    assert n.value == len(w_out)
    plain.close()
