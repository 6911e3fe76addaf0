"""CPU: frontiers of the navigation grid (include/loamx.h, loamx_densemap_frontiers ...) — every new symbol declared and exported, the
record laid out as a C compiler lays it out (64 bytes), the defaults, every bound of loamx_grid_frontier_check, loamx_frontiers_best
against the model; and the model the GPU tests check the device against (tests/densemap_frontier_model.py), checked here against values
counted by hand on the designed grids."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_frontier_model as fm
import densemap_grid_model as gm
import densemap_route_model as rm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_grid_frontier_default_config", "loamx_grid_frontier_check", "loamx_densemap_frontiers",
               "loamx_densemap_frontiers_cells", "loamx_frontiers_best")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert "} loamx_grid_frontier_config;" in hdr and "} loamx_frontier;" in hdr
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for name in ("frontiers", "frontiers_cells"):
        assert callable(getattr(loamx.DenseMap, name)), name
    assert callable(loamx.FrontierConfig) and callable(loamx.frontiers_best)
    assert "#define LOAMX_FRONTIER_NONE 0xFFFFFFFFu\n" in hdr and loamx.FRONTIER_NONE == fm.NONE == 2 ** 32 - 1
    assert len(loamx.FRONTIER_STATS) == 6


def test_record_layout_matches_c(tmp_path):
    """sizeof(loamx_frontier) == 64 and every field where the binding's dtype and the model's have it"""
    fields = list(loamx.FRONTIER.names)
    cfg_fields = [f for f, _ in loamx.FrontierConfig._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     '  printf("%zu\\n", sizeof(loamx_frontier));\n' +
                     "".join(f'  printf("%zu\\n", offsetof(loamx_frontier, {f}));\n' for f in fields) +
                     '  printf("%zu\\n", sizeof(loamx_grid_frontier_config));\n' +
                     "".join(f'  printf("%zu\\n", offsetof(loamx_grid_frontier_config, {f}));\n' for f in cfg_fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    n = len(fields)
    assert got[0] == 64 == loamx.FRONTIER.itemsize == fm.FRONTIER.itemsize and loamx.FRONTIER == fm.FRONTIER
    assert got[1:1 + n] == [loamx.FRONTIER.fields[f][1] for f in fields]
    assert got[1 + n] == C.sizeof(loamx.FrontierConfig) == 16
    assert got[2 + n:] == [getattr(loamx.FrontierConfig, f).offset for f in cfg_fields] and cfg_fields == list(fm.DEFAULTS)


def test_defaults():
    c = loamx.FrontierConfig()
    assert {f: getattr(c, f) for f, _ in c._fields_} == fm.DEFAULTS == dict(connectivity=8, min_unknown=1, min_clear2=1, min_cells=1)
    loamx.lib().loamx_grid_frontier_default_config(None)   # NULL: nothing to fill
    assert c.check() is c and fm.check(fm.DEFAULTS) is None
    assert loamx.lib().loamx_grid_frontier_check(None) == loamx.E_INVALID and b"cfg" in loamx.lib().loamx_last_error()


@pytest.mark.parametrize("field,bad,good", [("connectivity", (0, 6, 9), (4, 8)), ("min_unknown", (0, 9), (1, 8)), ("min_clear2", (0,), (1, 4226)),
                                            ("min_cells", (0,), (1, 2 ** 32 - 1))])
def test_check_names_each_bad_field(field, bad, good):
    for v in bad:
        with pytest.raises(loamx.LoamxError) as e:
            loamx.FrontierConfig(**{field: v}).check()
        assert e.value.code == loamx.E_INVALID and field in str(e.value)
        assert fm.check(dict(fm.DEFAULTS, **{field: v})) == field
    for v in good:
        loamx.FrontierConfig(**{field: v}).check()
        assert fm.check(dict(fm.DEFAULTS, **{field: v})) is None


def test_check_names_the_first_bad_field():
    order = list(fm.DEFAULTS)
    for i, field in enumerate(order):    # every later field bad as well: the first one is named
        c = dict(fm.DEFAULTS, **{f: 0 for f in order[i:]})
        with pytest.raises(loamx.LoamxError) as e:
            loamx.FrontierConfig(**c).check()
        assert field in str(e.value) and fm.check(c) == field


def records(costs):
    a = np.zeros(len(costs), loamx.FRONTIER)
    a["best_cost"] = costs
    return a


def test_frontiers_best():
    U = rm.UNREACHABLE
    for costs, min_cost, want in [([30, 10, 10, 50], 0, 1),       # a tie: the smaller index
                                  ([30, 10, 10, 50], 11, 0),      # min_cost skips the frontier underfoot
                                  ([30, 10, 10, 50], 10, 1), ([30, 10, 10, 50], 31, 3), ([30, 10, 10, 50], 51, fm.NONE),
                                  ([0, 7], 0, 0), ([0, 7], 1, 1),
                                  ([U, U], 0, fm.NONE),           # none is reachable
                                  ([U, 5, U], 0, 1), ([], 0, fm.NONE)]:
        assert loamx.frontiers_best(records(costs), min_cost) == want == fm.best(records(costs), min_cost), (costs, min_cost)
    L, best = loamx.lib(), C.c_uint32(77)
    assert L.loamx_frontiers_best(None, C.c_uint64(0), 0, C.byref(best)) == loamx.OK and best.value == fm.NONE    # n == 0
    best = C.c_uint32(77)
    assert L.loamx_frontiers_best(None, C.c_uint64(2), 0, C.byref(best)) == loamx.E_INVALID and best.value == 77
    a = records([1])
    assert L.loamx_frontiers_best(a.ctypes.data_as(C.c_void_p), C.c_uint64(1), 0, None) == loamx.E_INVALID and b"best" in L.loamx_last_error()


# ---- the model against values counted by hand ---------------------------------------------------------------------------------------------
def one(cells, **cfg):
    return fm.frontiers(cells, cfg)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("s,x0", [(2, 3), (3, 3), (20, 22)])
def test_square_in_unknown(conn, s, x0):
    """the FREE square of side s: its rim of 4 s - 4 cells is one frontier; a corner cell sees 5 unknown cells, an edge cell 3"""
    n = 70 if s == 20 else 9
    out, labels, stats, field = one(fm.square(n, n, x0, x0, s), connectivity=conn)
    assert stats == (4 * s - 4, 1, 1, 4 * s - 4, 0) and field is None and len(out) == 1
    r = out[0]
    assert r["min_cell"] == x0 * n + x0 and r["cells"] == 4 * s - 4 and r["unknown_links"] == 12 * (s - 2) + 20
    assert r["lo"].tolist() == [x0, x0] and r["hi"].tolist() == [x0 + s - 1, x0 + s - 1]
    assert r["sum_rx"] == r["sum_rz"] == (4 * s - 4) * (2 * x0 + s - 1) // 2    # symmetric about the centre
    assert (r["reachable"], r["best_cost"], r["best_cell"], r["reserved"]) == (0, rm.UNREACHABLE, fm.NONE, 0)
    inner = labels[x0 + 1:x0 + s - 1, x0 + 1:x0 + s - 1]
    assert int((labels == 0).sum()) == 4 * s - 4 and np.all(inner == fm.NONE) and int((labels == fm.NONE).sum()) == n * n - (4 * s - 4)


def test_one_cell_windows():
    for cls in (gm.FREE, gm.UNKNOWN, gm.OBSTACLE):
        out, labels, stats, _ = one(fm.filled(1, 1, cls))
        assert len(out) == 0 and stats == (0, 0, 0, 0, 0) and labels.tolist() == [[fm.NONE]]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", [(1, 70), (70, 1)])
def test_runs(conn, shape):
    """runs of three, FREE first: the ends of a FREE run are frontier cells, its middle is not; the first run's first cell is at the
    window's edge, and outside is not unknown: 1 + 2 * 11 frontiers of one cell, each with one unknown neighbour"""
    out, labels, stats, _ = one(fm.runs(*shape), connectivity=conn)
    assert stats == (23, 23, 23, 23, 0)
    assert out["min_cell"].tolist() == [2] + [c for k in range(1, 12) for c in (6 * k, 6 * k + 2)]
    assert np.all(out["cells"] == 1) and np.all(out["unknown_links"] == 1)
    idx = out["min_cell"].astype(np.int64)
    want_rx, want_rz = (np.zeros(23, np.int64), idx) if shape[0] == 1 else (idx, np.zeros(23, np.int64))
    assert out["sum_rx"].tolist() == want_rx.tolist() and out["sum_rz"].tolist() == want_rz.tolist()
    assert labels.reshape(-1)[idx].tolist() == list(range(23))


def test_staircase():
    cells = fm.staircase(70, 20, 45)    # through the tile corner (31, 31) -> (32, 32)
    out, labels, stats, _ = one(cells, connectivity=8)
    assert stats == (26, 1, 1, 26, 0) and out[0]["min_cell"] == 20 * 70 + 20 and out[0]["unknown_links"] == 24 * 6 + 2 * 7
    assert out[0]["lo"].tolist() == [20, 20] and out[0]["hi"].tolist() == [45, 45] and out[0]["sum_rx"] == sum(range(20, 46))
    out, labels, stats, _ = one(cells, connectivity=4)
    assert stats == (26, 26, 26, 26, 0) and out["min_cell"].tolist() == [i * 71 for i in range(20, 46)]
    assert [labels[i, i] for i in range(20, 46)] == list(range(26))
    assert one(cells, connectivity=4, min_cells=2)[2] == (26, 26, 0, 0, 0)
    assert one(cells, connectivity=8, min_unknown=7)[2] == (2, 2, 2, 2, 0)    # a stair has 6 unknown neighbours, the two ends 7
    assert one(cells, connectivity=8, min_unknown=8)[2] == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("conn", [4, 8])
def test_spiral(conn):
    cells = fm.spiral(70, 45)
    free = int((cells["cls"] == gm.FREE).sum())
    out, labels, stats, _ = one(cells, connectivity=conn)
    assert free > 1500 and stats == (free, 1, 1, free, 0) and out[0]["cells"] == free and out[0]["min_cell"] == 0
    assert out[0]["lo"].tolist() == [0, 0] and out[0]["hi"].tolist() == [69, 44]
    assert np.array_equal(labels == 0, cells["cls"] == gm.FREE)
    # the corridor is one cell wide and its turns one cell apart: rows 0, 2, 4 ... of the first column
    assert cells["cls"][:6, 0].tolist() == [gm.FREE, gm.UNKNOWN, gm.FREE, gm.FREE, gm.FREE, gm.FREE] and cells["cls"][1, :68].max() == gm.UNKNOWN


@pytest.mark.parametrize("conn", [4, 8])
def test_combs(conn):
    out, labels, stats, _ = one(fm.combs(), connectivity=conn)
    assert stats == (22 * 33 + 64 + 4 * 3 + 10, 2, 2, 812, 0)
    assert out["min_cell"].tolist() == [5 * 70 + 3, 41 * 70 + 2] and out["cells"].tolist() == [790, 22]
    assert out["lo"].tolist() == [[3, 5], [2, 41]] and out["hi"].tolist() == [[66, 38], [11, 44]]
    assert labels[5, 66] == 0 and labels[41, 11] == 1    # the last tooth's tip carries the first one's number
    assert one(fm.combs(), connectivity=conn, min_cells=23)[2] == (812, 2, 1, 790, 0)


def test_no_frontier_without_unknown_inside_the_window():
    for cells in (fm.filled(70, 70, gm.FREE), fm.no_unknown()):    # outside is not unknown; OBSTACLE and STEP are not unknown
        out, labels, stats, _ = one(cells)
        assert len(out) == 0 and stats == (0, 0, 0, 0, 0) and np.all(labels == fm.NONE)


def test_a_narrow_cell_is_no_frontier_cell_and_connects_nothing():
    cells = fm.narrow(3)
    assert one(cells)[2] == (3, 1, 1, 3, 0)
    out, labels, stats, _ = one(cells, min_clear2=3)
    assert stats == (2, 2, 2, 2, 0) and out["min_cell"].tolist() == [6, 8] and labels[1].tolist() == [fm.NONE, 0, fm.NONE, 1, fm.NONE]
    assert out["unknown_links"].tolist() == [7, 7]    # the narrow cell is FREE, not unknown


def test_costs_on_a_symmetric_grid():
    """the start in the middle of a FREE square: the middles of the four sides share the smallest cost; the smallest index wins"""
    cells = fm.square(21, 21, 5, 5, 11)
    for conn, cost in ((8, 50), (4, 50)):
        out, _, stats, field = fm.frontiers(cells, dict(connectivity=conn), dict(connectivity=conn), (10, 10))
        assert stats == (40, 1, 1, 40, 1) and out[0]["reachable"] == 40
        assert (out[0]["best_cost"], out[0]["best_cell"]) == (cost, 5 * 21 + 10) and field["cost"][10, 5] == field["cost"][5, 10] == cost
        assert fm.best(out) == 0 and fm.best(out, cost + 1) == fm.NONE


def test_a_frontier_behind_a_wall_is_unreachable():
    cells = fm.walled()
    out, _, stats, _ = fm.frontiers(cells, None, None, (5, 5))
    assert stats[1:3] == (2, 2) and stats[4] == 1 and out["reachable"].tolist() == [out[0]["cells"], 0]
    assert (out[1]["best_cost"], out[1]["best_cell"]) == (rm.UNREACHABLE, fm.NONE) and out[0]["best_cost"] == 40 and fm.best(out) == 0
    for start in ((40, 5), (19, 5)):    # outside the window; on the wall
        out, _, stats, _ = fm.frontiers(cells, None, None, start)
        assert stats[4] == 0 and np.all(out["reachable"] == 0) and fm.best(out) == fm.NONE


def test_random70_parameters_act():
    cells = fm.random70()
    seen = set()
    for cfg in (dict(), dict(min_unknown=3), dict(min_cells=4), dict(min_clear2=6), dict(connectivity=4)):
        out, labels, stats, _ = one(cells, **cfg)
        assert stats[0] >= stats[3] and stats[1] >= stats[2] == len(out) and stats[0] > 100
        assert int((labels != fm.NONE).sum()) == stats[3] == int(out["cells"].sum()) and np.all(np.diff(out["min_cell"].astype(np.int64)) > 0)
        seen.add(out.tobytes() + labels.tobytes())
    assert len(seen) == 5
