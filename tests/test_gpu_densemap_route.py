"""GPU: routing on the navigation grid (include/loamx.h, loamx_densemap_route and what goes with it) against its model
(tests/densemap_route_model.py).  Every comparison is the bytes of the whole field against the model's, no tolerance anywhere, and
stats[0:4] equal the model's.  The shapes are the smallest at which the tiling of k_dm_route_relax (32 x 32 cells, a halo of one) can go
wrong.  On every shape the schedule is held to its bound as well: at least one round is launched, and the rounds in which a tile ran are
at most min_crossings + 2 (the invariant in the head comment of csrc/densemap_route.hip) — a condition, not a measurement: a
dirty-marking bug that keeps tiles spinning fails it.  Through the map: the 541-voxel box scene of tests/test_gpu_densemap_grid.py."""
import ctypes as C

import numpy as np
import pytest

import densemap_carve_model as cm
import densemap_grid_model as gm
import densemap_raycast_model as rcm
import densemap_route_model as rm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

LEAF = 0.5
BASE = dict(min_points=1, band_lo=1, band_hi=4, max_step=1, clear_max=3)    # of tests/test_gpu_densemap_grid.py
K1 = dict(cell_leaves=1, x0=-8, z0=-5, nx=17, nz=11)
W37 = dict(cell_leaves=1, x0=-18, z0=-26, nx=37, nz=53)
SENTINEL = 0xABABABAB


def explain(got, want):
    """the first cell that differs (for the assertion message)"""
    if got.shape != want.shape:
        return f"shapes {got.shape}, {want.shape}"
    for z, x in np.argwhere((got["cost"] != want["cost"]) | (got["next"] != want["next"])):
        return f"cell [z {z}, x {x}]: got {got[z, x]}, want {want[z, x]}"
    return "equal"


def check(got, want):
    assert got.dtype == rm.ROUTE_CELL == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), explain(got, want)


def random_grid(nx=70, nz=70, seed=11):
    rng = np.random.default_rng(seed)
    cls = rng.choice(4, size=(nz, nx), p=[0.12, 0.7, 0.12, 0.06])
    clear2 = rng.integers(1, 30, size=(nz, nx))
    clear2[cls >= gm.OBSTACLE] = 0
    return rm.cells_of(cls, clear2)


def many_goals(n=4096, seed=5):
    return [tuple(v) for v in np.random.default_rng(seed).integers(0, 70, (n, 2)).tolist()]    # 4096 pairs on 4900 cells: duplicates too


SOFT = dict(soft_clear2=25, soft_weight=9)
# name -> (cells, goals, configuration beside the connectivity)
CASES = {
    "1x1": (lambda: rm.open(1, 1), [(0, 0)], {}),
    "32x32": (lambda: rm.open(32, 32), [(5, 7)], {}),                          # one tile exactly
    "33x31": (lambda: rm.open(33, 31), [(32, 30)], {}),                        # a one-cell second tile column and a short tile
    "1x70": (lambda: rm.open(1, 70), [(0, 3)], {}),
    "70x1": (lambda: rm.open(70, 1), [(66, 0)], {}),
    "open70": (lambda: rm.open(70, 70), [(0, 0)], {}),
    "serpentine": (lambda: rm.serpentine(70, 45), [(0, 0)], {}),               # 23 crossings, the same tiles entered again and again
    "serpentine_both_ends": (lambda: rm.serpentine(70, 45), [(0, 0), (69, 44)], {}),    # the fronts meet
    "random_soft": (lambda: random_grid(), [(4, 3), (61, 41)], SOFT),          # weights differ: the cheapest path is not the shortest
    "random_unknown0": (lambda: random_grid(), [(35, 35)], dict(SOFT, unknown_weight=0)),
    "random_unknown3": (lambda: random_grid(), [(35, 35)], dict(SOFT, unknown_weight=3)),
    "random_min_clear2": (lambda: random_grid(), [(35, 35), (2, 66)], dict(min_clear2=6, soft_clear2=20, soft_weight=15, unknown_weight=16)),
    "goals_mixed": (lambda: rm.serpentine(70, 45), [(5, 4), (70, 0), (0, 45), (2 ** 32 - 1, 1), (30, 10), (30, 10), (1, 8)], {}),
    "goals_all_invalid": (lambda: rm.serpentine(70, 45), [(5, 4), (70, 0), (0, 45), (9, 8)], {}),
    "goals_4096": (lambda: rm.open(70, 70), many_goals(), {}),
    "goals_4096_random": (lambda: random_grid(), many_goals(seed=6), SOFT),
}
_cells, _model = {}, {}


def cells_of_case(name):
    if name not in _cells:
        _cells[name] = CASES[name][0]()
    return _cells[name]


def model_of(name, conn):
    """(field, stats[0:4], min_crossings) of a case, computed once"""
    if (name, conn) not in _model:
        _, goals, cfg = CASES[name]
        cfg = dict(cfg, connectivity=conn)
        cells = cells_of_case(name)
        f = rm.field(cells, cfg, goals)
        _model[(name, conn)] = (f, rm.stats(cells, cfg, goals, f), rm.min_crossings(cells, cfg, goals))
    return _model[(name, conn)]


@pytest.fixture(scope="module")
def router():
    return loamx.DenseMap(leaf=LEAF, initial_slots=1024)    # an empty map: route_cells needs a handle, not its voxels


def held_to_the_bound(d, crossings):
    st = d.route_stats
    print("rounds launched", st["rounds"], "rounds that ran a tile", d.route_active_rounds, "tile runs", st["tile_runs"], "min_crossings", crossings)
    assert st["rounds"] >= 1 and d.route_active_rounds <= crossings + 2 and d.route_active_rounds <= st["rounds"]
    assert st["tile_runs"] >= d.route_active_rounds


# ---- 1: the shapes x connectivity 4 and 8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(CASES))
def test_field_equals_the_model(router, name, conn):
    _, goals, cfg = CASES[name]
    want, stats, crossings = model_of(name, conn)
    got = router.route_cells(cells_of_case(name), goals, connectivity=conn, **cfg)
    check(got, want)
    st = router.route_stats
    assert (st["traversable"], st["reachable"], st["goals_used"], st["max_cost"]) == stats
    held_to_the_bound(router, crossings)
    if name == "serpentine":
        assert stats == (2470, 2470, 1, 7686 if conn == 8 else 7830) and crossings == 23 and router.route_active_rounds >= 2
    if name == "open70":
        assert stats == (4900, 4900, 1, 966 if conn == 8 else 1380) and crossings == (2 if conn == 8 else 4)
    if name == "goals_mixed":
        assert stats[2] == 3    # the wall cell and the three outside are ignored; (30, 10) counts twice, (1, 8) lies in its wall's gap
    if name == "goals_all_invalid":
        assert stats[1:] == (0, 0, 0) and np.all(got["cost"] == rm.UNREACHABLE) and np.all(got["next"] == rm.NONE) and st["tile_runs"] == 0
    if name == "random_unknown3":
        assert stats[0] > model_of("random_unknown0", conn)[1][0] and want.tobytes() != model_of("random_unknown0", conn)[0].tobytes()
    if name == "random_soft":    # the penalties matter: without them the field differs
        assert want.tobytes() != rm.field(cells_of_case(name), dict(connectivity=conn), goals).tobytes()
    if name == "goals_4096":
        assert 2000 < stats[2] == 4096 and stats[1] == 4900


def test_a_batch_of_one_round_gives_the_same_field(router):
    """the result does not depend on the schedule: one round per look, and 64"""
    want, stats, crossings = model_of("serpentine", 8)
    try:
        for batch in (1, 64, 3):
            router.route_set_batch(batch)
            check(router.route_cells(cells_of_case("serpentine"), [(0, 0)]), want)
            held_to_the_bound(router, crossings)
            assert router.route_stats["rounds"] % batch == 0 or batch == 64
    finally:
        router.route_set_batch(16)


# ---- 2: through the map ----------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("rule,traversable,reachable", [(None, 38, 33), (cm.DEFAULT_RULE, 48, 48)], ids=["plain", "rule"])
def test_window_k1_through_the_map(scene, rule, traversable, reachable):
    d = scene["map"]
    cfg = dict(BASE, **K1)
    cells = gm.grid(scene["model"], rule, **cfg)
    want = rm.field(cells, None, [(3, 2)])
    static = None if rule is None else loamx.StaticRule(*rule)
    got, got_cells = d.route([(3, 2)], grid=loamx.GridConfig(**cfg), static=static, want_cells=True)
    check(got, want)
    st = d.route_stats
    assert (st["traversable"], st["reachable"], st["goals_used"]) == (traversable, reachable, 1) == rm.stats(cells, None, [(3, 2)], want)[:3]
    assert st["max_cost"] == rm.stats(cells, None, [(3, 2)], want)[3]
    held_to_the_bound(d, 0)
    # out_cells is the grid of the same configuration, byte for byte, and route_cells on it gives the same field
    assert got_cells.tobytes() == cells.tobytes() == d.grid(loamx.GridConfig(**cfg), static=static).tobytes()
    check(d.route_cells(got_cells, [(3, 2)]), want)
    # nothing back, then the trace over the field that stayed on the device
    assert d.route([(3, 2)], grid=loamx.GridConfig(**cfg), static=static, want_field=False) is None
    starts = [(x, z) for z in range(K1["nz"]) for x in range(K1["nx"])]
    routes, lengths = d.route_trace(starts, 40)
    for s, r, n in zip(starts, routes, lengths):
        w, m = rm.trace(want, s)
        assert n == m and r.tobytes() == w.tobytes(), s
    assert int((lengths > 0).sum()) == reachable


def test_window_37x53_through_the_map(scene):
    d = scene["map"]
    cfg = dict(BASE, **W37)
    cells = gm.grid(scene["model"], None, **cfg)
    for conn, goals, extra in ((8, [(13, 23)], {}), (4, [(13, 23), (0, 0)], dict(unknown_weight=2, soft_clear2=16, soft_weight=5))):
        rc = dict(extra, connectivity=conn)
        want = rm.field(cells, rc, goals)
        got = d.route(goals, grid=loamx.GridConfig(**cfg), **rc)
        check(got, want)
        st = d.route_stats
        assert (st["traversable"], st["reachable"], st["goals_used"], st["max_cost"]) == rm.stats(cells, rc, goals, want)
        held_to_the_bound(d, rm.min_crossings(cells, rc, goals))
    assert st["reachable"] > 1000    # through the UNKNOWN sea around the box: both tile columns and rows


def test_the_map_is_untouched_and_the_grid_keeps_its_bytes(scene):
    d = scene["map"]
    before = exports(d)
    cfg = loamx.GridConfig(**dict(BASE, **K1))
    grid_before = d.grid(cfg)
    d.route_cells(rm.serpentine(70, 45), [(0, 0)])    # a larger window on the route's own buffer
    d.route([(3, 2)], grid=loamx.GridConfig(**dict(BASE, **W37)))
    d.route_trace([(3, 2)], 10)
    assert exports(d) == before and d.grid(cfg).tobytes() == grid_before.tobytes()


def test_large_then_small_window():
    d = loamx.DenseMap(leaf=LEAF, initial_slots=1024)    # a handle of its own: its planes have never been allocated
    big = rm.open(300, 200)
    for cells, goals in ((big, [(299, 199)]), (rm.open(3, 2), [(0, 0)]), (rm.serpentine(70, 45), [(0, 0)]), (rm.open(3, 2), [(2, 1)])):
        got = d.route_cells(cells, goals)
        if cells is big:    # too large for the model in a quick test: the open grid's cost has a closed form
            dx, dz = 299 - np.arange(300)[None, :], 199 - np.arange(200)[:, None]
            assert np.array_equal(got["cost"], 14 * np.minimum(dx, dz) + 10 * np.abs(dx - dz)) and d.route_stats["reachable"] == 60000
        else:
            check(got, rm.field(cells, None, goals))
    d.close()


def test_empty_map():
    d = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
    g = loamx.GridConfig(cell_leaves=1, nx=37, nz=53, clear_max=2)
    f = d.route([(1, 1)], grid=g)
    assert np.all(f["cost"] == rm.UNREACHABLE) and d.route_stats["traversable"] == 0 == d.route_stats["goals_used"]
    f, cells = d.route([(1, 1)], grid=g, want_cells=True, unknown_weight=2)
    assert np.all(cells["cls"] == gm.UNKNOWN) and np.all(cells["clear2"] == 9)
    check(f, rm.field(cells, dict(unknown_weight=2), [(1, 1)]))
    assert d.route_stats["reachable"] == 37 * 53 and len(d) == 0
    d.close()


# ---- 3: the trace ------------------------------------------------------------------------------------------------------------------------------
def test_trace_from_every_cell_of_the_serpentine(router):
    cells = cells_of_case("serpentine")
    f, _, _ = model_of("serpentine", 8)
    got = router.route_cells(cells, [(0, 0)])
    check(got, f)
    L = loamx.lib()
    starts = [(x, z) for z in range(45) for x in range(70)] + [(70, 0), (0, 45), (2 ** 32 - 1, 2 ** 32 - 1), (5, 4)]    # outside; a wall
    want = [rm.trace(f, s) for s in starts]
    longest = max(n for _, n in want)
    assert longest > 400 and sum(1 for _, n in want if n) == 2470
    exact = want[starts.index((40, 22))][1]    # a capacity that is exactly one route's length
    for cap in (longest, 300, exact, 1, 0):
        for lo in range(0, len(starts), 4096):    # batches of up to 4096 starts
            part = np.array(starts[lo:lo + 4096], np.uint32)
            out = np.full((len(part), cap, 2), SENTINEL, np.uint32)
            lengths = np.full(len(part), SENTINEL, np.uint32)
            rc = L.loamx_densemap_route_trace(router.h, part.ctypes.data_as(C.c_void_p), C.c_uint32(len(part)),
                                              out.ctypes.data_as(C.c_void_p) if cap else None, C.c_uint32(cap), lengths.ctypes.data_as(C.c_void_p))
            assert rc == loamx.OK
            for i, (w, n) in enumerate(want[lo:lo + 4096]):
                k = min(n, cap)
                assert lengths[i] == n and out[i, :k].tobytes() == w[:k].tobytes() and np.all(out[i, k:] == SENTINEL), (cap, starts[lo + i])
    for s, (w, n) in list(zip(starts, want))[::97]:    # the host trace over the device's field: the same bytes
        h, m = loamx.route_trace(got, s)
        assert m == n and h.tobytes() == w.tobytes()
    routes, lengths = router.route_trace([(69, 44), (5, 4), (0, 0)], 5)
    assert lengths.tolist() == [longest, 0, 1] and [len(r) for r in routes] == [5, 0, 1] and routes[2].tolist() == [[0, 0]]


# ---- 4: refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(scene):
    d, L = scene["map"], loamx.lib()
    plain = loamx.DenseMap(leaf=LEAF, initial_slots=1024)    # no carving, and no field yet
    before = exports(d)
    good = loamx.GridConfig(**dict(BASE, **K1))
    n = good.nx * good.nz
    want = d.route([(3, 2)], grid=good)
    cells_buf, field_buf = np.full(n * 24, 0xAB, np.uint8), np.full(n * 8, 0xAB, np.uint8)
    stats = (C.c_uint64 * 6)(*[77] * 6)
    cp, fp = cells_buf.ctypes.data_as(C.c_void_p), field_buf.ctypes.data_as(C.c_void_p)
    goals = np.array([[3, 2]], np.uint32)
    gp = goals.ctypes.data_as(C.c_void_p)
    rc, rule, bad_rule = loamx.RouteConfig(), loamx.StaticRule(), loamx.StaticRule(den=0)
    own = rm.open(17, 11)
    own_bad = own.copy()
    own_bad["cls"][10, 16] = 4
    op, obp = own.ctypes.data_as(C.c_void_p), own_bad.ctypes.data_as(C.c_void_p)
    cases = [(lambda: L.loamx_densemap_route(None, C.byref(good), None, C.byref(rc), gp, 1, cp, fp, stats), b"h is NULL"),
             (lambda: L.loamx_densemap_route(d.h, C.byref(good), None, C.byref(rc), None, 1, cp, fp, stats), b"goals_xz"),
             (lambda: L.loamx_densemap_route(d.h, C.byref(good), None, C.byref(rc), gp, 0, cp, fp, stats), b"n_goals"),
             (lambda: L.loamx_densemap_route(d.h, C.byref(good), None, C.byref(rc), gp, 4097, cp, fp, stats), b"n_goals"),
             (lambda: L.loamx_densemap_route(d.h, C.byref(good), None, C.byref(rc.copy(connectivity=6)), gp, 1, cp, fp, stats), b"connectivity"),
             (lambda: L.loamx_densemap_route(d.h, C.byref(good), None, C.byref(rc.copy(min_clear2=0)), gp, 1, cp, fp, stats), b"min_clear2"),
             (lambda: L.loamx_densemap_route(d.h, C.byref(good.copy(nx=0)), None, C.byref(rc), gp, 1, cp, fp, stats), b"nx"),
             (lambda: L.loamx_densemap_route(d.h, C.byref(good.copy(clear_max=65)), None, C.byref(rc), gp, 1, cp, fp, stats), b"clear_max"),
             (lambda: L.loamx_densemap_route(d.h, C.byref(good), C.byref(bad_rule), C.byref(rc), gp, 1, cp, fp, stats), b"den"),
             (lambda: L.loamx_densemap_route(plain.h, C.byref(good), C.byref(rule), C.byref(rc), gp, 1, cp, fp, stats), b"carving"),
             (lambda: L.loamx_densemap_route(d.h, C.byref(good.copy(nx=2049, nz=2048)), None, C.byref(rc), gp, 1, cp, fp, stats), b"nx * nz"),
             (lambda: L.loamx_densemap_route_cells(d.h, None, 17, 11, C.byref(rc), gp, 1, fp, stats), b"cells is NULL"),
             (lambda: L.loamx_densemap_route_cells(d.h, obp, 17, 11, C.byref(rc), gp, 1, fp, stats), b"cls"),
             (lambda: L.loamx_densemap_route_cells(d.h, op, 2049, 2048, C.byref(rc), gp, 1, fp, stats), b"nx * nz"),
             (lambda: L.loamx_densemap_route_cells(d.h, op, 0, 11, C.byref(rc), gp, 1, fp, stats), b"nx * nz"),
             (lambda: L.loamx_densemap_route_cells(d.h, op, 17, 11, C.byref(rc.copy(unknown_weight=17)), gp, 1, fp, stats), b"unknown_weight"),
             (lambda: L.loamx_densemap_route_cells(d.h, op, 17, 11, C.byref(rc), None, 1, fp, stats), b"goals_xz"),
             (lambda: L.loamx_densemap_route_cells(d.h, op, 17, 11, C.byref(rc), gp, 4097, fp, stats), b"n_goals")]
    for call, word in cases:
        assert call() == loamx.E_INVALID and word in L.loamx_last_error(), (word, L.loamx_last_error())
        assert cells_buf.tobytes() == bytes([0xAB]) * (n * 24) and field_buf.tobytes() == bytes([0xAB]) * (n * 8) and list(stats) == [77] * 6
    # the trace's own refusals; the field of the last successful call is still there after all of the above
    out, lengths = np.full((2, 4, 2), SENTINEL, np.uint32), np.full(2, SENTINEL, np.uint32)
    xp, lp = out.ctypes.data_as(C.c_void_p), lengths.ctypes.data_as(C.c_void_p)
    starts = np.array([[16, 10], [3, 2]], np.uint32)
    sp = starts.ctypes.data_as(C.c_void_p)
    for call, word in [(lambda: L.loamx_densemap_route_trace(None, sp, 2, xp, 4, lp), b"h is NULL"),
                       (lambda: L.loamx_densemap_route_trace(d.h, None, 2, xp, 4, lp), b"starts_xz"),
                       (lambda: L.loamx_densemap_route_trace(d.h, sp, 0, xp, 4, lp), b"n_starts"),
                       (lambda: L.loamx_densemap_route_trace(d.h, sp, 4097, xp, 4, lp), b"n_starts"),
                       (lambda: L.loamx_densemap_route_trace(d.h, sp, 2, None, 4, lp), b"out_xz"),
                       (lambda: L.loamx_densemap_route_trace(d.h, sp, 2, xp, 4, None), b"lengths"),
                       (lambda: L.loamx_densemap_route_trace(plain.h, sp, 2, xp, 4, lp), b"no field")]:
        assert call() == loamx.E_INVALID and word in L.loamx_last_error(), (word, L.loamx_last_error())
        assert np.all(out == SENTINEL) and np.all(lengths == SENTINEL)
    with pytest.raises(loamx.LoamxError) as e:
        d.route([(3, 2)], grid=good, soft_weight=16)
    assert e.value.code == loamx.E_INVALID and "soft_weight" in str(e.value)
    # the handle is what it was, and the calls after a refusal are right
    assert exports(d) == before
    assert L.loamx_densemap_route_trace(d.h, sp, 2, xp, 4, lp) == loamx.OK
    w0, n0 = rm.trace(want, (16, 10), 4)
    assert lengths.tolist() == [n0, 1] and out[0, :min(n0, 4)].tobytes() == w0.tobytes() and out[1, 0].tolist() == [3, 2] and np.all(out[1, 1:] == SENTINEL)
    assert L.loamx_densemap_route(d.h, C.byref(good), None, None, gp, 1, cp, fp, stats) == loamx.OK    # NULL cfg: the defaults
    assert field_buf.tobytes() == want.tobytes() and cells_buf.tobytes() == d.grid(good).tobytes() and stats[2] == 1
    assert L.loamx_densemap_route(d.h, C.byref(good), None, None, gp, 1, None, None, None) == loamx.OK     # nothing wanted back
    plain.close()
