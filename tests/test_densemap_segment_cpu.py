"""CPU: the dense map's connected components (include/loamx.h, loamx_densemap_segment ...) — every new symbol declared and exported, the
two structs laid out as a C compiler lays them out, the defaults, every bound of loamx_densemap_segment_check, loamx_segment_box
against its formula; and the model the GPU tests check the device against (tests/densemap_segment_model.py), checked here against
cases worked out by hand and against the component counts of a separate prototype on the box scene of the ray-cast tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_carve_model as cm
import densemap_raycast_model as rm
import densemap_segment_model as sm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_segment_default_config", "loamx_densemap_segment_check", "loamx_densemap_segment", "loamx_segment_box")
LEAF = 0.5
LIM = 2 ** 20 - 1


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert "} loamx_densemap_segment_config;" in hdr and "} loamx_segment;" in hdr
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    assert callable(loamx.DenseMap.segment) and callable(loamx.segment_box) and callable(loamx.SegmentConfig)
    assert "#define LOAMX_SEGMENT_NONE 0xFFFFFFFFu\n" in hdr and loamx.SEGMENT_NONE == sm.NONE == 2 ** 32 - 1
    for k, name in enumerate(("ALL", "STATIC", "DYNAMIC")):
        assert f"#define LOAMX_SEGMENT_{name} {k}u" in hdr and getattr(loamx, "SEGMENT_" + name) == getattr(sm, name) == k
    assert "decided on the indices, not on the packed key" in hdr   # the rule the header owes its readers


@pytest.mark.parametrize("c_name,py", [("loamx_densemap_segment_config", "SegmentConfig"), ("loamx_segment", "Segment")])
def test_struct_layout_matches_c(tmp_path, c_name, py):
    struct = getattr(loamx, py)
    fields = [f for f, _ in struct._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     f'  printf("%zu\\n", sizeof({c_name}));\n' +
                     "".join(f'  printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(struct)
    assert got[1:] == [getattr(struct, f).offset for f in fields]
    if py == "Segment":
        assert got[0] == 72 == loamx.SEGMENT.itemsize == sm.SEGMENT.itemsize
        assert loamx.SEGMENT == sm.SEGMENT and list(loamx.SEGMENT.names) == fields
        assert got[1:] == [loamx.SEGMENT.fields[f][1] for f in fields]
    else:
        assert got[0] == 40 and fields == list(sm.DEFAULTS)


def as_dict(c):
    return {f: (tuple(getattr(c, f)) if f in ("lo", "hi") else getattr(c, f)) for f, _ in c._fields_}


def test_defaults():
    c = loamx.SegmentConfig()
    assert as_dict(c) == sm.DEFAULTS
    assert sm.DEFAULTS == dict(which=0, connectivity=26, min_points=1, min_voxels=1, lo=(-LIM,) * 3, hi=(LIM,) * 3)
    loamx.lib().loamx_densemap_segment_default_config(None)   # NULL: nothing to fill
    assert c.check() is c and sm.check(sm.DEFAULTS) is None
    d = loamx.SegmentConfig(connectivity=6, lo=(1, 2, 3)).copy(min_voxels=5)
    assert (d.connectivity, tuple(d.lo), d.min_voxels, tuple(d.hi)) == (6, (1, 2, 3), 5, (LIM,) * 3)


def axis(a, v, other=0):
    return tuple(v if k == a else other for k in range(3))


# (id, the field the message names, configurations accepted at the edge of the bound, configurations refused just beyond it)
BOUNDS = [("which", "which", [dict(which=0), dict(which=2)], [dict(which=3), dict(which=2 ** 32 - 1)]),
          ("connectivity", "connectivity", [dict(connectivity=6), dict(connectivity=18), dict(connectivity=26)],
           [dict(connectivity=v) for v in (0, 5, 7, 8, 17, 19, 25, 27)]),
          ("min_points", "min_points", [dict(min_points=1), dict(min_points=2 ** 32 - 1)], [dict(min_points=0)]),
          ("min_voxels", "min_voxels", [dict(min_voxels=1), dict(min_voxels=2 ** 32 - 1)], [dict(min_voxels=0)])]
for _a in range(3):
    BOUNDS.append((f"lo{_a}", "lo", [dict(lo=axis(_a, -LIM, -5)), dict(lo=axis(_a, LIM, -5), hi=axis(_a, LIM, 7))],
                   [dict(lo=axis(_a, -LIM - 1, -5)), dict(lo=axis(_a, LIM + 1, -5)), dict(lo=axis(_a, -2 ** 31, -5))]))
    BOUNDS.append((f"hi{_a}", "hi", [dict(hi=axis(_a, LIM, 5)), dict(hi=axis(_a, -LIM, 5), lo=axis(_a, -LIM, -7))],
                   [dict(hi=axis(_a, LIM + 1, 5)), dict(hi=axis(_a, -LIM - 1, 5), lo=axis(_a, -LIM, -7)), dict(hi=axis(_a, 2 ** 31 - 1, 5))]))
    BOUNDS.append((f"lo{_a}_le_hi{_a}", "lo", [dict(lo=axis(_a, 3), hi=axis(_a, 3))], [dict(lo=axis(_a, 4), hi=axis(_a, 3))]))


@pytest.mark.parametrize("name,field,good,bad", BOUNDS, ids=[b[0] for b in BOUNDS])
def test_check_bounds(name, field, good, bad):
    L = loamx.lib()
    for kw in good:
        c = loamx.SegmentConfig(**kw)
        assert L.loamx_densemap_segment_check(C.byref(c)) == loamx.OK, kw
        assert sm.check(dict(sm.DEFAULTS, **kw)) is None
    for kw in bad:
        c = loamx.SegmentConfig(**kw)
        assert L.loamx_densemap_segment_check(C.byref(c)) == loamx.E_INVALID, kw
        assert field.encode() in L.loamx_last_error(), (kw, L.loamx_last_error())
        assert sm.check(dict(sm.DEFAULTS, **kw)) == field
        with pytest.raises(loamx.LoamxError):
            c.check()


def test_check_null_arguments():
    L = loamx.lib()
    assert L.loamx_densemap_segment_check(None) == loamx.E_INVALID and b"cfg" in L.loamx_last_error()
    n, st = C.c_uint64(7), (C.c_uint64 * 6)()
    assert L.loamx_densemap_segment(None, None, None, None, C.c_uint64(0), C.byref(n), None, C.c_uint64(0), C.byref(n), st) == loamx.E_INVALID
    assert b"h is NULL" in L.loamx_last_error() and n.value == 7


# ---- loamx_segment_box against its formula
def record(lo, hi, sum_idx, voxels, points=1, min_key=0):
    r = np.zeros(1, sm.SEGMENT)
    r["lo"], r["hi"], r["sum_idx"], r["voxels"], r["points"], r["min_key"] = lo, hi, sum_idx, voxels, points, min_key
    return r[0]


@pytest.mark.parametrize("leaf", [0.5, 0.1, 0.3])
def test_segment_box(leaf):
    for rec in (record((0, 0, 0), (0, 0, 0), (0, 0, 0), 1),
                record((-3, -1, 2), (4, -1, 9), (7, -5, 40), 5),          # negative indices, a sum that does not divide
                record((-LIM, -LIM, -LIM), (LIM, LIM, LIM), (-3 * LIM, 0, 3 * LIM), 3),
                record((-7, -7, -7), (-7, -7, -7), (-7, -7, -7), 1),
                record((0, 0, 0), (99, 0, 0), (2 ** 40 + 1, -(2 ** 40) - 1, 1), 2 ** 33 + 7)):
        got = loamx.segment_box(rec, leaf)
        want = sm.segment_box(rec, leaf)
        for g, w in zip(got, want):
            assert g.dtype == np.float32 and g.tobytes() == w.tobytes(), (rec, got, want)
    lo, hi, ce = loamx.segment_box(record((-3, -1, 2), (4, -1, 9), (7, -5, 40), 5), 0.5)
    assert lo.tolist() == [-1.5, -0.5, 1.0] and hi.tolist() == [2.5, 0.0, 5.0]
    assert ce.tobytes() == np.array([(7 / 5 + 0.5) * 0.5, (-5 / 5 + 0.5) * 0.5, (40 / 5 + 0.5) * 0.5], np.float32).tobytes()
    lo, hi, ce = loamx.segment_box(record((-7, -7, -7), (-7, -7, -7), (-7, -7, -7), 1), 0.5)
    assert lo.tolist() == [-3.5] * 3 and hi.tolist() == [-3.0] * 3 and ce.tolist() == [-3.25] * 3   # voxel -7 spans [-3.5, -3.0)


def test_segment_box_refusals():
    L = loamx.lib()
    with pytest.raises(loamx.LoamxError) as e:
        loamx.segment_box(record((0, 0, 0), (0, 0, 0), (0, 0, 0), 0), 0.5)
    assert e.value.code == loamx.E_INVALID and "voxels" in str(e.value)
    r = np.zeros(1, sm.SEGMENT)
    r["voxels"] = 1
    out = np.full((3, 3), 7, np.float32)
    ptr = [o.ctypes.data_as(C.c_void_p) for o in out]
    for k in range(4):
        args = [r.ctypes.data_as(C.c_void_p)] + ptr
        args[k] = None
        assert L.loamx_segment_box(args[0], C.c_float(0.5), args[1], args[2], args[3]) == loamx.E_INVALID
        assert b"NULL" in L.loamx_last_error() and np.all(out == 7)


# ---- the model against cases worked out by hand
def seg(cells, counts=None, **cfg):
    return sm.segment(sm.model_of_cells(cells, LEAF, counts), **cfg)


@pytest.mark.parametrize("d,joined", [((1, 0, 0), (True, True, True)), ((0, 1, 0), (True, True, True)), ((0, 0, 1), (True, True, True)),
                                      ((1, 1, 0), (False, True, True)), ((0, 1, -1), (False, True, True)), ((-1, 0, 1), (False, True, True)),
                                      ((1, 1, 1), (False, False, True)), ((-1, 1, -1), (False, False, True)),
                                      ((2, 0, 0), (False, False, False)), ((1, 2, 0), (False, False, False))])
def test_model_pairs(d, joined):
    a = (-1, 3, 0)
    b = tuple(a[k] + d[k] for k in range(3))
    for conn, j in zip((6, 18, 26), joined):
        labels, rec, st = seg([a, b], connectivity=conn)
        assert st == dict(selected=2, components=1 if j else 2, kept=1 if j else 2, kept_voxels=2, largest=2 if j else 1)
        assert sorted(labels.tolist()) == ([0, 0] if j else [0, 1]) and len(rec) == st["kept"]
        assert rec[0]["min_key"] == min(cm.key_of(a), cm.key_of(b))


def test_model_l_of_three():
    cells = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (5, 5, 5)]
    labels, rec, st = seg(cells, counts=[1, 2, 3, 4], connectivity=6)
    assert st == dict(selected=4, components=2, kept=2, kept_voxels=4, largest=3)
    # keys ascend with iz, then iy, then ix: (0,0,0) < (1,0,0) < (1,1,0) < (5,5,5)
    assert labels.tolist() == [0, 0, 0, 1]
    r = rec[0]
    assert (r["min_key"], r["voxels"], r["points"]) == (cm.key_of((0, 0, 0)), 3, 6)
    assert r["lo"].tolist() == [0, 0, 0] and r["hi"].tolist() == [1, 1, 0] and r["sum_idx"].tolist() == [2, 1, 0]
    assert (rec[1]["voxels"], rec[1]["points"], rec[1]["sum_idx"].tolist()) == (1, 4, [5, 5, 5])
    # the two ends of the L touch by an edge only
    assert seg([(0, 0, 0), (1, 1, 0)], connectivity=6)[2]["components"] == 2 and seg([(0, 0, 0), (1, 1, 0)], connectivity=18)[2]["components"] == 1


def test_model_window_cuts_a_bar():
    bar = [(x, 0, 0) for x in range(-4, 5)]
    assert seg(bar)[2]["components"] == 1
    labels, rec, st = seg(bar, lo=(-LIM, -LIM, -LIM), hi=(-1, LIM, LIM))
    assert st == dict(selected=4, components=1, kept=1, kept_voxels=4, largest=4) and labels.tolist() == [0] * 4 + [sm.NONE] * 5
    # a window with a hole cannot be asked for, but two calls can: the voxel at x = 0 is outside both and connects nothing
    right = seg(bar, lo=(1, 0, 0), hi=(LIM, 0, 0))
    assert right[0].tolist() == [sm.NONE] * 5 + [0] * 4 and right[1][0]["lo"].tolist() == [1, 0, 0]
    # a U whose bottom bar the window leaves out: the two uprights, in one call
    u = bar + [(-4, y, 0) for y in (1, 2, 3)] + [(4, y, 0) for y in (1, 2, 3)]
    labels, rec, st = seg(u, lo=(-LIM, 1, -LIM), hi=(LIM, LIM, LIM))
    assert st == dict(selected=6, components=2, kept=2, kept_voxels=6, largest=3) and labels.tolist() == [sm.NONE] * 9 + [0, 1] * 3
    assert rec["lo"].tolist() == [[-4, 1, 0], [4, 1, 0]] and rec["hi"].tolist() == [[-4, 3, 0], [4, 3, 0]]
    # min_points cuts the same bar in two within one call
    labels, rec, st = seg(bar, counts=[2, 2, 2, 2, 1, 2, 2, 2, 2], min_points=2)
    assert st == dict(selected=8, components=2, kept=2, kept_voxels=8, largest=4) and labels.tolist() == [0] * 4 + [sm.NONE] + [1] * 4
    assert rec["points"].tolist() == [8, 8] and rec["sum_idx"][:, 0].tolist() == [-10, 10]


def test_model_min_voxels_renumbers():
    cells = [(0, 0, 0), (3, 0, 0), (4, 0, 0), (7, 0, 0), (9, 0, 0), (10, 0, 0), (11, 0, 0)]   # sizes 1, 2, 1, 3 in key order
    assert seg(cells)[0].tolist() == [0, 1, 1, 2, 3, 3, 3]
    labels, rec, st = seg(cells, min_voxels=2)
    assert labels.tolist() == [sm.NONE, 0, 0, sm.NONE, 1, 1, 1] and rec["voxels"].tolist() == [2, 3]
    assert st == dict(selected=7, components=4, kept=2, kept_voxels=5, largest=3)
    labels, rec, st = seg(cells, min_voxels=4)
    assert labels.tolist() == [sm.NONE] * 7 and len(rec) == 0 and st == dict(selected=7, components=4, kept=0, kept_voxels=0, largest=3)


def test_model_key_range_edges():
    # the packed keys of these two differ by one, their cells lie at opposite ends of x: not adjacent
    a, b = (LIM, 0, 0), (-LIM, 1, 0)
    assert cm.key_of(b) - cm.key_of(a) == 2
    assert seg([a, b])[2]["components"] == 2
    assert seg([(LIM, 0, 0), (LIM - 1, 1, -1)])[2]["components"] == 1 and seg([(-LIM, -LIM, -LIM), (-LIM + 1, -LIM, -LIM)])[2]["components"] == 1


# ---- the model against a separate prototype on the box scene (541 voxels, 23 dynamic, x -6..6, y -5..5, z -4..2)
TABLE = {(sm.ALL, 6): (15, [518, 3, 3, 2, 2, 2, 2, 2] + [1] * 7), (sm.ALL, 18): (2, [540, 1]), (sm.ALL, 26): (2, [540, 1]),
         (sm.STATIC, 6): (10, [507, 2, 2] + [1] * 7), (sm.STATIC, 18): (8, [508, 3, 2] + [1] * 5), (sm.STATIC, 26): (8, [508, 3, 2] + [1] * 5),
         (sm.DYNAMIC, 6): (15, [5, 4, 2] + [1] * 12), (sm.DYNAMIC, 18): (9, [7, 6, 3, 2] + [1] * 5), (sm.DYNAMIC, 26): (5, [11, 6, 3, 2, 1])}
Y_WINDOW = dict(lo=(-LIM, -4, -LIM), hi=(LIM, 4, LIM))   # floor and ceiling cut off


@pytest.fixture(scope="module")
def box():
    S = rm.box_cast_scene()
    m = cm.CarveModel(leaf=LEAF)
    for p, o in S["sweeps"]:
        assert m.add(p, o)
    assert len(m) == 541 and int(m.dynamic_mask().sum()) == 23
    cells = np.array([sm.cell_of(k) for k in m.keys.tolist()])
    assert cells.min(axis=0).tolist() == [-6, -5, -4] and cells.max(axis=0).tolist() == [6, 5, 2]
    return m


@pytest.mark.parametrize("which,conn", list(TABLE))
def test_box_scene_table(box, which, conn):
    n, want = TABLE[(which, conn)]
    got = sm.sizes(box, which=which, connectivity=conn)
    assert len(got) == n and got == want
    labels, rec, st = sm.segment(box, which=which, connectivity=conn)
    assert st["components"] == st["kept"] == n and st["largest"] == want[0] and st["selected"] == sum(want) == st["kept_voxels"]
    assert st["selected"] == {sm.ALL: 541, sm.STATIC: 518, sm.DYNAMIC: 23}[which]
    assert sorted(rec["voxels"].tolist(), reverse=True) == want and np.all(np.diff(rec["min_key"].astype(np.int64)) > 0)
    assert int((labels != sm.NONE).sum()) == st["selected"] and np.array_equal(np.bincount(labels[labels != sm.NONE]), rec["voxels"])


def test_box_scene_figures(box):
    assert sm.segment(box, connectivity=6, min_voxels=2)[2]["kept"] == 8 and sm.segment(box, connectivity=6, min_voxels=3)[2]["kept"] == 3
    assert sm.segment(box, which=sm.DYNAMIC, min_voxels=2)[2]["kept"] == 4 and sm.segment(box, which=sm.DYNAMIC, min_voxels=3)[2]["kept"] == 3
    for conn in (6, 18, 26):
        st = sm.segment(box, connectivity=conn, min_points=2)[2]
        assert (st["selected"], st["components"]) == (507, 2)
        st = sm.segment(box, connectivity=conn, min_points=3)[2]
        assert (st["selected"], st["components"]) == (506, 1)
    got = sm.sizes(box, connectivity=6, **Y_WINDOW)
    assert sum(got) == 359 and len(got) == 15 and got[:8] == [336, 3, 3, 2, 2, 2, 2, 2]
    assert sm.sizes(box, connectivity=18, **Y_WINDOW) == [358, 1] == sm.sizes(box, connectivity=26, **Y_WINDOW)
    got = sm.sizes(box, which=sm.STATIC, connectivity=6, **Y_WINDOW)
    assert (sum(got), len(got), got[0]) == (336, 10, 325)
    got = sm.sizes(box, which=sm.STATIC, connectivity=26, **Y_WINDOW)
    assert (sum(got), len(got), got[0]) == (336, 8, 326)
