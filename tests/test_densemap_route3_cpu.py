"""CPU: routing in 3-D over the distance field (include/loamx.h, loamx_densemap_route3 ...) — every new symbol declared and exported,
the struct laid out as a C compiler lays it out, the defaults, every bound of loamx_route3_check, loamx_route3_weight,
loamx_route3_move, loamx_route3_trace, loamx_route3_points and loamx_densemap_dist_cell_of against the model; and the model the GPU
tests check the device against (tests/densemap_route3_model.py), checked here against cases worked out by hand and against the
figures of a separate prototype of the definition."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_route3_model as r3
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_route3_default_config", "loamx_route3_check", "loamx_route3_weight", "loamx_route3_move", "loamx_densemap_route3",
               "loamx_densemap_route3_last", "loamx_densemap_route3_cells", "loamx_densemap_route3_trace", "loamx_route3_trace",
               "loamx_route3_points", "loamx_densemap_dist_cell_of")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    for name in ("loamx_densemap_route3_set_batch", "loamx_densemap_route3_active_rounds"):    # the hooks: exported, not declared
        assert hasattr(L, name) and name not in hdr, name
    assert "} loamx_route3_config;" in hdr
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for name in ("route3", "route3_last", "route3_cells", "route3_trace", "route3_set_batch"):
        assert callable(getattr(loamx.DenseMap, name)), name
    assert isinstance(loamx.DenseMap.route3_active_rounds, property)
    for name in ("Route3Config", "route3_weight", "route3_trace", "route3_points", "dist_cell_of"):
        assert callable(getattr(loamx, name)), name
    assert "#define LOAMX_ROUTE3_GOAL 26u\n" in hdr and loamx.ROUTE3_GOAL == r3.GOAL == 26
    assert "#define LOAMX_ROUTE3_NONE 27u\n" in hdr and loamx.ROUTE3_NONE == r3.NONE == 27
    assert loamx.ROUTE3_MOVES == r3.MOVES and len(r3.MOVES) == 26 == len(set(r3.MOVES)) and (0, 0, 0) not in r3.MOVES
    assert "(1,0,0) (-1,0,0) (0,1,0) (0,-1,0) (0,0,1) (0,0,-1)" in hdr and "(1,1,0) (-1,1,0) (1,-1,0) (-1,-1,0) (1,0,1)" in hdr
    assert loamx.ROUTE_CELL == r3.ROUTE_CELL


def test_struct_layout_matches_c(tmp_path):
    struct, c_name = loamx.Route3Config, "loamx_route3_config"
    fields = [f for f, _ in struct._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     f'  printf("%zu\\n", sizeof({c_name}));\n' +
                     "".join(f'  printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(struct) == 16
    assert got[1:] == [getattr(struct, f).offset for f in fields]
    assert fields == list(r3.DEFAULTS)


def test_defaults():
    c = loamx.Route3Config()
    assert {f: getattr(c, f) for f, _ in c._fields_} == r3.DEFAULTS
    assert r3.DEFAULTS == dict(connectivity=26, min_d2=1, soft_d2=0, soft_weight=0)
    loamx.lib().loamx_route3_default_config(None)   # NULL: nothing to fill
    assert c.check() is c and r3.check(r3.DEFAULTS) is None
    assert loamx.Route3Config(connectivity=6).copy(soft_weight=3).connectivity == 6
    assert loamx.lib().loamx_route3_check(None) == loamx.E_INVALID and b"cfg" in loamx.lib().loamx_last_error()


# (field, values accepted at the edge of the bound, values refused just beyond it)
BOUNDS = [("connectivity", (6, 18, 26), (0, 4, 5, 7, 8, 17, 19, 25, 27)),
          ("min_d2", (1, 65025, 2 ** 32 - 1), (0,)),
          ("soft_d2", (0, 65025), (65026, 2 ** 32 - 1)),
          ("soft_weight", (0, 15), (16,))]


@pytest.mark.parametrize("field,good,bad", BOUNDS, ids=[b[0] for b in BOUNDS])
def test_check_bounds(field, good, bad):
    L = loamx.lib()
    for v in good:
        c = loamx.Route3Config(**{field: v})
        assert L.loamx_route3_check(C.byref(c)) == loamx.OK, (field, v)
        assert r3.check(dict(r3.DEFAULTS, **{field: v})) is None
        assert L.loamx_route3_weight(C.c_uint32(9), C.byref(c)) >= 0
    for v in bad:
        c = loamx.Route3Config(**{field: v})
        assert L.loamx_route3_check(C.byref(c)) == loamx.E_INVALID, (field, v)
        assert field.encode() in L.loamx_last_error(), (field, L.loamx_last_error())
        assert r3.check(dict(r3.DEFAULTS, **{field: v})) == field
        with pytest.raises(loamx.LoamxError):
            c.check()
        assert L.loamx_route3_weight(C.c_uint32(9), C.byref(c)) == loamx.E_INVALID   # an unchecked configuration


def test_check_names_the_first_field_in_the_order_of_the_struct():
    L = loamx.lib()
    order = list(r3.DEFAULTS)
    bad = dict(connectivity=7, min_d2=0, soft_d2=70000, soft_weight=16)
    for i, name in enumerate(order):
        c = dict(r3.DEFAULTS, **{k: bad[k] for k in order[i:]})
        assert L.loamx_route3_check(C.byref(loamx.Route3Config(**c))) == loamx.E_INVALID and name.encode() in L.loamx_last_error()
        assert r3.check(c) == name


# ---- loamx_route3_weight and loamx_route3_move against the model
CONFIGS = [dict(), dict(min_d2=4, soft_d2=100, soft_weight=15), dict(connectivity=6, soft_d2=65025, soft_weight=7), dict(min_d2=65536)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=["defaults", "heavy", "soft_far", "all_blocked"])
def test_weight_matches_the_model(cfg):
    ladder = np.array([0, 1, 2, 3, 4, 5, 9, 50, 99, 100, 101, 121, 2000, 65024, 65025, 65535], np.uint16)
    got = loamx.route3_weight(ladder, loamx.Route3Config(**cfg))
    want = [r3.weight_of(v, r3.config(**cfg)) for v in ladder]
    assert got.dtype == np.uint8 and got.tolist() == want
    assert got[0] == 0 and got.max() <= 16    # an occupied cell is always blocked
    if not cfg:
        assert got.tolist() == [0] + [1] * (len(ladder) - 1)
    if cfg.get("soft_weight") == 15:
        # p reaches soft_weight only at d2 0, which min_d2 >= 1 never lets through: 15 is the largest weight met here
        assert got.tolist()[:6] == [0, 0, 0, 0, 1 + 15 * 96 // 100, 1 + 15 * 95 // 100] and got.max() == 15 and got[9] == 1
    if cfg.get("min_d2") == 65536:
        assert not got.any()    # above every d2: every cell blocked, and still a configuration that passes
    L = loamx.lib()
    assert L.loamx_route3_weight(C.c_uint32(9), None) == loamx.E_INVALID and b"cfg" in L.loamx_last_error()
    assert L.loamx_route3_weight(C.c_uint32(1), C.byref(loamx.Route3Config(soft_d2=1, soft_weight=15))) == 1
    assert L.loamx_route3_weight(C.c_uint32(1), C.byref(loamx.Route3Config(soft_d2=2, soft_weight=15))) == 8 == r3.weight_of(1, r3.config(soft_d2=2, soft_weight=15))


def test_move_table():
    L = loamx.lib()
    out = (C.c_int32 * 3)(7, 7, 7)
    for d, m in enumerate(r3.MOVES):
        assert L.loamx_route3_move(d, out) == loamx.OK and tuple(out) == m
        assert r3.SCALE[d] == (5 if d < 6 else 7 if d < 18 else 9) == 3 + 2 * sum(1 for v in m if v)
        assert len(r3.BETWEEN[d]) == (0 if d < 6 else 2 if d < 18 else 6)
    # each connectivity is a prefix, and every move has its opposite within the same prefix
    for conn in (6, 18, 26):
        assert {tuple(-v for v in m) for m in r3.MOVES[:conn]} == set(r3.MOVES[:conn])
    assert r3.MOVES[18:] == ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1), (1, 1, -1), (-1, 1, -1), (1, -1, -1), (-1, -1, -1))
    out = (C.c_int32 * 3)(7, 7, 7)
    assert L.loamx_route3_move(26, out) == loamx.E_INVALID and b"d must" in L.loamx_last_error() and tuple(out) == (7, 7, 7)
    assert L.loamx_route3_move(0, None) == loamx.E_INVALID and b"dxyz" in L.loamx_last_error()


# ---- the model against cases worked out by hand
def test_model_2x2x2_from_its_corner():
    f = r3.field(r3.open(2, 2, 2), None, [(0, 0, 0)])
    assert f["cost"].tolist() == [[[0, 10], [10, 14]], [[10, 14], [14, 18]]]
    assert f["next"].tolist() == [[[26, 1], [3, 9]], [[5, 13], [17, 25]]]
    f18 = r3.field(r3.open(2, 2, 2), dict(connectivity=18), [(0, 0, 0)])
    assert f18["cost"].tolist() == [[[0, 10], [10, 14]], [[10, 14], [14, 24]]] and f18["next"][1, 1, 1] == 1    # 10 + 14, the axial move first
    f6 = r3.field(r3.open(2, 2, 2), dict(connectivity=6), [(0, 0, 0)])
    assert f6["cost"].tolist() == [[[0, 10], [10, 20]], [[10, 20], [20, 30]]] and f6["next"][1, 1, 1] == 1


def test_model_no_corner_cutting():
    """2 x 2 x 2, goal (0, 0, 0), start (1, 1, 1): each of the six cells between them, blocked alone, forbids the space diagonal
    (d = 25); the face diagonals whose two side cells are open stay legal, so the start goes round at 14 + 10 = 24"""
    assert r3.field(r3.open(2, 2, 2), None, [(0, 0, 0)])[1, 1, 1].tolist() == (18, 25)
    for bx, by, bz in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]:
        d2 = r3.open(2, 2, 2)
        d2[bz, by, bx] = 0
        w = r3.weight(d2)
        legal = {d for d, *_ in r3.moves(w, 1, 1, 1, 26)}
        assert 25 not in legal, (bx, by, bz)
        f = r3.field(d2, None, [(0, 0, 0)])
        assert f[bz, by, bx].tolist() == (r3.UNREACHABLE, r3.NONE)
        assert f[1, 1, 1]["cost"] == 24 and r3.stats(d2, None, [(0, 0, 0)], f) == (7, 7, 1, 24)
        # a face diagonal from the start whose two side cells are open is still legal: e.g. with (1, 0, 0) blocked, (-1, -1, 0) to
        # (0, 0, 1) passes (0, 1, 1) and (1, 0, 1), both open, while (-1, 0, -1) to (0, 1, 0) would pass the corner of (1, 1, 0)
        # and (0, 1, 1)
        for d in range(6, 18):
            m = r3.MOVES[d]
            b = (1 + m[0], 1 + m[1], 1 + m[2])
            if not all(0 <= v < 2 for v in b):
                assert d not in legal
                continue
            sides = [(1 + sx, 1 + sy, 1 + sz) for sx, sy, sz in r3.BETWEEN[d]]
            assert len(sides) == 2
            assert (d in legal) == ((bx, by, bz) != b and (bx, by, bz) not in sides), (d, (bx, by, bz))
    # a face diagonal in a plane: a wall at (1, 0, 0) makes (1, 1, 0) go round, as on the 2-D grid
    d2 = r3.open(2, 2, 1)
    d2[0, 0, 1] = 0
    f = r3.field(d2, None, [(0, 0, 0)])
    assert f["cost"].tolist() == [[[0, r3.UNREACHABLE], [10, 20]]] and f["next"].tolist() == [[[26, 27], [3, 1]]]


def test_model_next_tie_break():
    """goals at (1, 0, 0) and (0, 1, 0) and (0, 0, 1): from (0, 0, 0) the three axial moves cost 10 each, and d = 0 wins"""
    f = r3.field(r3.open(2, 2, 2), None, [(1, 0, 0), (0, 1, 0), (0, 0, 1)])
    assert f[0, 0, 0].tolist() == (10, 0) and f[1, 1, 1].tolist() == (14, 9)    # (-1, -1, 0) to (0, 0, 1), before d = 13 and d = 17


def test_model_soft_penalty():
    """one row, d2 = 4, 1, 4, soft_d2 4, soft_weight 8: the middle cell pays p = floor(8 * 3 / 4) = 6, w = 7; moves of 5 * 8 = 40"""
    d2 = np.array([[[4, 1, 4]]], np.uint16)
    cfg = dict(soft_d2=4, soft_weight=8)
    assert r3.weight(d2, cfg) == [[[1, 7, 1]]]
    assert r3.field(d2, cfg, [(0, 0, 0)])["cost"].tolist() == [[[0, 40, 80]]]
    d2 = np.array([[[4, 1, 4]], [[4, 4, 4]]], np.uint16)    # a second plane of unit weights: over it and back, two face diagonals
    assert r3.field(d2, cfg, [(0, 0, 0)])["cost"].tolist() == [[[0, 40, 28]], [[10, 14, 24]]]
    assert r3.field(d2, dict(cfg, min_d2=2), [(0, 0, 0)])["cost"].tolist() == [[[0, r3.UNREACHABLE, 40]], [[10, 20, 30]]]    # no corner cutting: not 20 + 14 past the blocked cell


def test_model_goals():
    d2 = np.array([[[9, 0, 9]]], np.uint16)
    f = r3.field(d2, None, [(1, 0, 0), (5, 0, 0), (0, 7, 0), (0, 0, 1)])    # blocked, outside on each axis
    assert np.all(f["cost"] == r3.UNREACHABLE) and np.all(f["next"] == r3.NONE) and r3.stats(d2, None, [(1, 0, 0), (5, 0, 0)], f) == (2, 0, 0, 0)
    f = r3.field(d2, None, [(1, 0, 0), (2, 0, 0), (2, 0, 0)])
    assert f["cost"].tolist() == [[[r3.UNREACHABLE, r3.UNREACHABLE, 0]]] and r3.stats(d2, None, [(1, 0, 0), (2, 0, 0), (2, 0, 0)], f) == (2, 1, 2, 0)


def test_a_route_in_a_plane_costs_what_the_2d_route_costs():
    import densemap_route_model as rm
    rng = np.random.default_rng(4)
    blocked = rng.random((9, 11)) < 0.2
    blocked[0, 0] = False
    cells = rm.cells_of(np.where(blocked, 2, 1))
    f2 = rm.field(cells, None, [(0, 0)])
    d2 = np.where(blocked, 0, r3.FAR).astype(np.uint16)
    for shape, axes in (((9, 1, 11), (0, 2)), ((9, 11, 1), (0, 1)), ((1, 9, 11), (1, 2))):
        f3 = r3.field(d2.reshape(shape), None, [(0, 0, 0)])
        assert np.array_equal(f3["cost"].reshape(9, 11), f2["cost"]), shape


# ---- the model against the figures of the prototype: (traversable, reachable, largest cost, min_crossings at brick 8)
PROTOTYPE = {("open", 6): (4913, 4913, 480, 6), ("open", 18): (4913, 4913, 336, 3), ("open", 26): (4913, 4913, 288, 2),
             ("serpentine3", 6): (2540, 2540, 1600, 15), ("serpentine3", 18): (2540, 2540, 1324, 13), ("serpentine3", 26): (2540, 2540, 1324, 13)}


@pytest.mark.parametrize("name,conn", list(PROTOTYPE))
def test_model_against_the_prototype(name, conn):
    d2 = r3.open(17, 17, 17) if name == "open" else r3.serpentine3()
    cfg = dict(connectivity=conn)
    f = r3.field(d2, cfg, [(0, 0, 0)])
    st = r3.stats(d2, cfg, [(0, 0, 0)], f)
    assert st[2] == 1 and (st[0], st[1], st[3], r3.min_crossings(d2, cfg, [(0, 0, 0)], brick=8)) == PROTOTYPE[(name, conn)]
    if name == "open":    # by hand: 48 axial moves, 24 face diagonals, 16 space diagonals
        assert st[3] == {6: 48 * 10, 18: 24 * 14, 26: 16 * 18}[conn] == f[16, 16, 16]["cost"]


def test_serpentine3_layout():
    d2 = r3.serpentine3()
    assert d2.shape == (19, 9, 20) and d2.dtype == np.uint16
    floors = sorted(set(np.argwhere(d2 == 0)[:, 0].tolist()))
    assert floors == [3, 6, 9, 12, 15] and set(np.unique(d2).tolist()) == {0, r3.FAR}
    for i, z in enumerate(floors):
        holes = {(int(x), int(y)) for y, x in np.argwhere(d2[z] != 0)}
        assert holes == ({(18, 7), (19, 7), (18, 8), (19, 8)} if i % 2 == 0 else {(0, 0), (1, 0), (0, 1), (1, 1)})
    assert int((d2 != 0).sum()) == 2540


# ---- loamx_route3_trace against the model
@pytest.fixture(scope="module")
def serp():
    d2 = r3.serpentine3()
    return d2, r3.field(d2, None, [(0, 0, 0)])


def test_trace_matches_the_model(serp):
    d2, f = serp
    far = (19, 8, 18)
    for start in [(0, 0, 0), (1, 0, 0), far, (10, 4, 10), (0, 8, 18), (5, 5, 3), (20, 0, 0), (0, 9, 0), (0, 0, 19), (2 ** 32 - 1, 3, 3)]:
        want, n = r3.trace(f, start)
        got, m = loamx.route3_trace(f, start)
        assert m == n and got.dtype == np.uint32 and got.tobytes() == want.tobytes(), start
        if n:
            assert tuple(got[0]) == start and tuple(got[-1]) == (0, 0, 0)
    assert r3.trace(f, (5, 5, 3))[1] == 0 == r3.trace(f, (20, 0, 0))[1] and r3.trace(f, (0, 0, 0))[1] == 1    # a floor; outside; the goal itself
    want, n = r3.trace(f, far)
    assert n > 60
    s = (C.c_uint32 * 3)(*far)
    for cap in (0, 1, n - 1, n, n + 3):
        buf = np.full((cap + 2, 3), 0xABABABAB, np.uint32)
        ln = C.c_uint32(77)
        rc = loamx.lib().loamx_route3_trace(f.ctypes.data_as(C.c_void_p), 20, 9, 19, s, buf.ctypes.data_as(C.c_void_p) if cap else None,
                                            C.c_uint32(cap), C.byref(ln))
        assert rc == loamx.OK and ln.value == n
        k = min(cap, n)
        assert buf[:k].tobytes() == want[:k].tobytes() and np.all(buf[k:] == 0xABABABAB)    # beyond the route: untouched
        assert r3.trace(f, far, cap)[0].tobytes() == want[:k].tobytes()


def test_trace_refuses_a_corrupt_field(serp):
    L = loamx.lib()
    _, f = serp
    far = (19, 8, 18)
    route, n = r3.trace(f, far)
    mid = tuple(int(v) for v in route[n // 2])
    before = tuple(int(v) for v in route[n // 2 - 1])
    buf = np.full((n, 3), 0xABABABAB, np.uint32)
    ln = C.c_uint32(77)

    def call(field, nx=20, ny=9, nz=19, start=far, out=buf, cap=n, length=ln):
        return L.loamx_route3_trace(field.ctypes.data_as(C.c_void_p) if field is not None else None, nx, ny, nz,
                                    (C.c_uint32 * 3)(*start) if start is not None else None,
                                    out.ctypes.data_as(C.c_void_p) if out is not None else None, C.c_uint32(cap),
                                    C.byref(length) if length is not None else None)

    def corrupt(cell, **words):
        bad = f.copy()
        for k, v in words.items():
            bad[cell[2], cell[1], cell[0]][k] = v
        return bad

    back = r3.MOVES.index(tuple(b - m for b, m in zip(before, mid)))    # the direction from mid back to the cell before it
    cases = [(corrupt(mid, next=28), far, b"next"),                                               # a next above 27
             (corrupt((19, 0, 0), next=0), (19, 0, 0), b"leaves the window"),                     # steps to x = 20
             (corrupt((4, 0, 1), next=3), (4, 0, 1), b"leaves the window"),                       # steps to y = -1
             (corrupt((4, 4, 18), next=4), (4, 4, 18), b"leaves the window"),                     # steps to z = 19
             (corrupt(mid, cost=f[before[2], before[1], before[0]]["cost"]), far, b"strictly smaller"),    # an equal cost
             (corrupt(mid, next=back), far, b"strictly smaller"),                                 # back where it came from: a loop
             (corrupt(mid, cost=5, next=r3.NONE), far, b"no goal")]                               # the route runs dry
    for field, start, word in cases:
        assert call(field, start=start) == loamx.E_INVALID and word in L.loamx_last_error(), (word, L.loamx_last_error())
        assert np.all(buf == 0xABABABAB) and ln.value == 77    # nothing written
    for kw, word in ((dict(field=None), b"field"), (dict(out=None), b"out_xyz"), (dict(length=None), b"length"), (dict(start=None), b"start"),
                     (dict(nx=0), b"nx * ny * nz"), (dict(nz=0), b"nx * ny * nz"), (dict(nx=4096, ny=1025, nz=1), b"nx * ny * nz"),
                     (dict(nx=2 ** 31, ny=2 ** 31, nz=4), b"nx * ny * nz")):
        assert call(kw.pop("field", f), **kw) == loamx.E_INVALID and word in L.loamx_last_error(), word
        assert np.all(buf == 0xABABABAB) and ln.value == 77
    assert call(f) == loamx.OK and ln.value == n and buf.tobytes() == route.tobytes()


# ---- loamx_route3_points and loamx_densemap_dist_cell_of against their formulas
WINDOWS = [dict(cell_leaves=3, x0=-8, y0=-1, z0=-2, nx=6, ny=3, nz=7), dict(cell_leaves=2, x0=1, y0=4, z0=-5, nx=5, ny=2, nz=5),
           dict(cell_leaves=1, x0=-2 ** 21, y0=0, z0=2 ** 21, nx=3, ny=1, nz=2)]


@pytest.mark.parametrize("leaf", [0.5, 0.1])
@pytest.mark.parametrize("wc", WINDOWS, ids=["k3_negative", "k2", "far_corner"])
def test_route3_points(wc, leaf):
    cfg = loamx.DistConfig(**wc)
    route = [(x, y, z) for z in range(wc["nz"]) for y in range(wc["ny"]) for x in range(wc["nx"])]
    got, want = loamx.route3_points(cfg, leaf, route), r3.points(wc, leaf, route)
    assert got.dtype == np.float32 and got.shape == (len(route), 3) and got.tobytes() == want.tobytes()
    if wc["cell_leaves"] == 3 and leaf == 0.5:
        assert r3.points(wc, leaf, [(0, 0, 0), (5, 2, 6)]).tolist() == [[-11.25, -0.75, -2.25], [-3.75, 2.25, 6.75]]    # (first + r + 0.5) * 1.5
    L, out = loamx.lib(), np.full(3, 7, np.float32)
    for bad in ((wc["nx"], 0, 0), (0, wc["ny"], 0), (0, 0, wc["nz"])):
        xyz = np.array([bad], np.uint32)
        args = (C.byref(cfg), C.c_float(leaf), xyz.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p))
        assert L.loamx_route3_points(*args) == loamx.E_INVALID and b"route_xyz" in L.loamx_last_error() and out.tolist() == [7, 7, 7]
    assert L.loamx_route3_points(None, *args[1:]) == loamx.E_INVALID and b"dist_cfg" in L.loamx_last_error()
    assert L.loamx_route3_points(args[0], C.c_float(0), *args[2:]) == loamx.E_INVALID and b"leaf" in L.loamx_last_error()
    assert L.loamx_route3_points(*args[:2], None, 1, args[4]) == loamx.E_INVALID and b"route_xyz" in L.loamx_last_error()
    assert L.loamx_route3_points(*args[:4], None) == loamx.E_INVALID and b"out_xyz" in L.loamx_last_error()
    assert loamx.route3_points(cfg, leaf, []).shape == (0, 3)


@pytest.mark.parametrize("wc", WINDOWS, ids=["k3_negative", "k2", "far_corner"])
def test_dist_cell_of(wc):
    cfg = loamx.DistConfig(**wc)
    for leaf in (0.5, 0.1):
        e = float(np.float32(leaf)) * wc["cell_leaves"]
        xs = [(wc["x0"] + i) * e for i in (-1, 0, 1, wc["nx"] - 1, wc["nx"])]    # exactly on cell edges (where e is a binary fraction)
        xs += [(wc["x0"] + 0.5) * e, (wc["x0"] + wc["nx"]) * e - 1e-3, wc["x0"] * e - 1e-3, 0.0, -0.0]
        ys = [(wc["y0"] + i) * e for i in (-1, 0, wc["ny"] - 1, wc["ny"])] + [(wc["y0"] + 0.75) * e, -1e-4]
        zs = [(wc["z0"] + i) * e for i in (-1, 0, wc["nz"] - 1, wc["nz"])] + [(wc["z0"] + 0.25) * e]
        inside = 0
        for x in xs:
            for y in ys:
                for z in zs:
                    got, want = loamx.dist_cell_of(cfg, leaf, x, y, z), r3.cell_of(wc, leaf, x, y, z)
                    assert got == want, (leaf, x, y, z)
                    inside += got is not None
        assert 0 < inside < len(xs) * len(ys) * len(zs)
    if wc["cell_leaves"] == 3:    # e = 1.5, x0 = -8, y0 = -1: floor, not truncation, on the negative side
        assert loamx.dist_cell_of(cfg, 0.5, -12.0, -1.5, -3.0) == (0, 0, 0) and loamx.dist_cell_of(cfg, 0.5, -3.0, -1.5, -3.0) is None
        assert loamx.dist_cell_of(cfg, 0.5, -3.0001, -0.0001, 7.4999) == (5, 0, 6) and loamx.dist_cell_of(cfg, 0.5, -12.0, -1.5001, 0.0) is None
        assert loamx.dist_cell_of(cfg, 0.5, -12.0, 2.9999, 0.0) == (0, 2, 2) and loamx.dist_cell_of(cfg, 0.5, -12.0, 3.0, 0.0) is None
    L = loamx.lib()
    r, ins = (C.c_uint32 * 3)(77, 78, 79), C.c_int(5)
    far = (wc["x0"] - 3) * 0.5 * wc["cell_leaves"]
    f = C.c_float
    assert L.loamx_densemap_dist_cell_of(C.byref(cfg), f(0.5), f(far), f(0), f(0), r, C.byref(ins)) == loamx.OK
    assert (tuple(r), ins.value) == ((77, 78, 79), 0)    # outside: r untouched
    for args, word in (((None, f(0.5), f(0), f(0), f(0), r, C.byref(ins)), b"dist_cfg"),
                       ((C.byref(cfg), f(0.5), f(np.nan), f(0), f(0), r, C.byref(ins)), b"x must"),
                       ((C.byref(cfg), f(0.5), f(0), f(-np.inf), f(0), r, C.byref(ins)), b"y must"),
                       ((C.byref(cfg), f(0.5), f(0), f(0), f(np.inf), r, C.byref(ins)), b"z must"),
                       ((C.byref(cfg), f(-1), f(0), f(0), f(0), r, C.byref(ins)), b"leaf"),
                       ((C.byref(cfg), f(0.5), f(0), f(0), f(0), None, C.byref(ins)), b"r is NULL"),
                       ((C.byref(cfg), f(0.5), f(0), f(0), f(0), r, None), b"inside"),
                       ((C.byref(cfg.copy(d_max=255)), f(0.5), f(0), f(0), f(0), r, C.byref(ins)), b"d_max")):
        assert L.loamx_densemap_dist_cell_of(*args) == loamx.E_INVALID and word in L.loamx_last_error(), word
        assert (tuple(r), ins.value) == ((77, 78, 79), 0)


# ---- NULL handles: refused before anything is touched
def test_null_handle():
    L = loamx.lib()
    xyz = np.zeros((1, 3), np.uint32)
    p = xyz.ctypes.data_as(C.c_void_p)
    assert L.loamx_densemap_route3(None, None, None, None, p, 1, None, None) == loamx.E_INVALID and b"h is NULL" in L.loamx_last_error()
    assert L.loamx_densemap_route3_last(None, None, p, 1, None, None) == loamx.E_INVALID and b"h is NULL" in L.loamx_last_error()
    assert L.loamx_densemap_route3_cells(None, p, 1, 1, 1, None, p, 1, None, None) == loamx.E_INVALID and b"h is NULL" in L.loamx_last_error()
    assert L.loamx_densemap_route3_trace(None, p, 1, p, 1, p) == loamx.E_INVALID and b"h is NULL" in L.loamx_last_error()
    assert L.loamx_densemap_route3_set_batch(None, 4) == loamx.E_INVALID
    L.loamx_densemap_route3_active_rounds.restype = C.c_uint64
    assert L.loamx_densemap_route3_active_rounds(None) == 0
