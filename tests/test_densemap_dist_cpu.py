"""CPU: the dense map's distance field (include/loamx.h, loamx_densemap_dist ...) — every new symbol declared and exported, the two
structs laid out as a C compiler lays them out, the defaults, every bound of loamx_densemap_dist_check, loamx_densemap_dist_window
against its formula, the near word packed and unpacked, loamx_dist_metres; and the model the GPU tests check the device against
(tests/densemap_dist_model.py): its brute force against its separable statement on random small volumes, ties included, and against
cases worked out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_carve_model as cm
import densemap_dist_model as xm
import densemap_model as dm
import densemap_raycast_model as rm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_dist_default_config", "loamx_densemap_dist_check", "loamx_densemap_dist_window", "loamx_densemap_dist",
               "loamx_densemap_dist_query", "loamx_dist_near_unpack", "loamx_dist_metres")
LEAF = 0.5   # inv = 2 exactly: voxel i spans [0.5 i, 0.5 (i + 1))


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert "} loamx_densemap_dist_config;" in hdr and "} loamx_dist_sample;" in hdr
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    assert callable(loamx.DenseMap.dist) and callable(loamx.DenseMap.dist_query)
    for name in ("dist_window", "dist_near_unpack", "dist_metres", "DistConfig"):
        assert callable(getattr(loamx, name)), name
    assert "#define LOAMX_DIST_NONE 0xFFFFFFFFu\n" in hdr and "#define LOAMX_DIST_OUTSIDE 0xFFFFFFFFu\n" in hdr
    assert loamx.DIST_NONE == xm.NONE == 2 ** 32 - 1 and loamx.DIST_OUTSIDE == xm.OUTSIDE == 2 ** 32 - 1
    assert loamx.DIST_STATS == xm.STATS and loamx.DIST_QUERY_STATS == xm.QUERY_STATS
    assert "between cell centres" in hdr   # the caveat the header owes its readers


def test_struct_layout_matches_c(tmp_path):
    fields = [f for f, _ in loamx.DistConfig._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     '  printf("%zu\\n", sizeof(loamx_densemap_dist_config));\n' +
                     "".join(f'  printf("%zu\\n", offsetof(loamx_densemap_dist_config, {f}));\n' for f in fields) +
                     '  printf("%zu %zu %zu\\n", sizeof(loamx_dist_sample), offsetof(loamx_dist_sample, d2), offsetof(loamx_dist_sample, near));\n'
                     "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(loamx.DistConfig) == 36
    assert got[1:-3] == [getattr(loamx.DistConfig, f).offset for f in fields] and fields == list(xm.DEFAULTS)
    assert got[-3:] == [8, 0, 4] and loamx.DIST_SAMPLE.itemsize == 8 and loamx.DIST_SAMPLE == xm.DIST_SAMPLE


def test_defaults():
    c = loamx.DistConfig()
    assert {f: getattr(c, f) for f, _ in c._fields_} == xm.DEFAULTS
    assert xm.DEFAULTS == dict(cell_leaves=2, x0=0, y0=0, z0=0, nx=128, ny=32, nz=128, min_points=2, d_max=16)
    loamx.lib().loamx_densemap_dist_default_config(None)   # NULL: nothing to fill
    assert c.check() is c and xm.check(xm.DEFAULTS) is None
    assert loamx.DistConfig(nx=3, d_max=0).copy(nz=5).nx == 3


# (field, values accepted at the edge of the bound, values refused just beyond it, fields set beside it)
BOUNDS = [("cell_leaves", (1, 64), (0, 65), {}),
          ("x0", (-2 ** 21, 2 ** 21), (-2 ** 21 - 1, 2 ** 21 + 1), {}),
          ("y0", (-2 ** 21, 2 ** 21), (-2 ** 21 - 1, 2 ** 21 + 1), {}),
          ("z0", (-2 ** 21, 2 ** 21), (-2 ** 21 - 1, 2 ** 21 + 1), {}),
          ("nx", (1, 1024), (0, 1025), dict(ny=8, nz=8)),
          ("ny", (1, 1024), (0, 1025), dict(nx=8, nz=8)),
          ("nz", (1, 1024), (0, 1025), dict(nx=8, ny=8)),
          ("nx * ny * nz", (), (), {}),    # (its own test below: three fields make it)
          ("min_points", (1, 2 ** 32 - 1), (0,), {}),
          ("d_max", (0, 254), (255, 2 ** 32 - 1), {})]


@pytest.mark.parametrize("field,good,bad,beside", BOUNDS, ids=[b[0] for b in BOUNDS])
def test_check_bounds(field, good, bad, beside):
    L = loamx.lib()
    for v in good:
        c = loamx.DistConfig(**beside, **{field: v})
        assert L.loamx_densemap_dist_check(C.byref(c)) == loamx.OK, (field, v)
        assert xm.check(dict(xm.DEFAULTS, **beside, **{field: v})) is None
    for v in bad:
        c = loamx.DistConfig(**beside, **{field: v})
        assert L.loamx_densemap_dist_check(C.byref(c)) == loamx.E_INVALID, (field, v)
        assert field.encode() in L.loamx_last_error(), (field, L.loamx_last_error())
        assert xm.check(dict(xm.DEFAULTS, **beside, **{field: v})) == field
        with pytest.raises(loamx.LoamxError):
            c.check()


def test_check_the_product_and_null():
    L = loamx.lib()
    for shape, ok in (((1024, 64, 1024), True), ((1024, 65, 1024), False), ((512, 512, 256), True), ((512, 512, 257), False),
                      ((1024, 1024, 1024), False)):
        c = loamx.DistConfig(nx=shape[0], ny=shape[1], nz=shape[2])
        want = dict(xm.DEFAULTS, nx=shape[0], ny=shape[1], nz=shape[2])
        assert (L.loamx_densemap_dist_check(C.byref(c)) == loamx.OK) == ok == (xm.check(want) is None), shape
        if not ok:
            assert b"nx * ny * nz" in L.loamx_last_error() and xm.check(want) == "nx * ny * nz"
    assert L.loamx_densemap_dist_check(None) == loamx.E_INVALID and b"cfg" in L.loamx_last_error()
    # the first field out of bounds is the one named
    c = loamx.DistConfig(cell_leaves=0, d_max=999)
    assert L.loamx_densemap_dist_check(C.byref(c)) == loamx.E_INVALID and b"cell_leaves" in L.loamx_last_error()


def test_null_handle_is_refused_without_a_device():
    L = loamx.lib()
    st = (C.c_uint64 * 5)()
    d2 = np.full(4, 0xABCD, np.uint16)
    assert L.loamx_densemap_dist(None, None, None, d2.ctypes.data_as(C.c_void_p), None, st) == loamx.E_INVALID
    assert b"h is NULL" in L.loamx_last_error() and np.all(d2 == 0xABCD)
    pts = np.zeros((2, 4), np.float32)
    cloud = loamx.cloud_of(pts)
    assert L.loamx_densemap_dist_query(None, C.byref(cloud), C.c_uint32(0), None, C.c_uint64(0), st) == loamx.E_INVALID
    assert b"h is NULL" in L.loamx_last_error()


# ---- loamx_densemap_dist_window against its formula
@pytest.mark.parametrize("leaf,k,centre,half", [(0.5, 3, (-7.3, 2.2, 0.4), (4.0, 1.0, 2.5)),    # a negative centre with k = 3
                                                (0.5, 2, (3.0, -3.0, 3.0), (2.0, 2.0, 0.0)),     # exactly on cell edges (e = 1)
                                                (0.1, 2, (12.34, -0.05, 1.0), (25.0, 3.0, 25.0)),   # a leaf that is no binary fraction
                                                (0.2, 1, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),      # no extent: the one cell of the centre
                                                (0.5, 64, (-1e5, 1e5, -3e4), (1000.0, 500.0, 0.0))])
def test_dist_window(leaf, k, centre, half):
    c = loamx.dist_window(leaf, *centre, half, cell_leaves=k)
    for a, (first, count) in enumerate((("x0", "nx"), ("y0", "ny"), ("z0", "nz"))):
        assert (getattr(c, first), getattr(c, count)) == xm.window(leaf, centre[a], half[a], k), first
    assert c.cell_leaves == k and c.check() is c
    assert (c.min_points, c.d_max) == (2, 16)    # the other fields are left alone
    if (leaf, k) == (0.5, 3):    # e = 1.5: x from floor(-11.3 / 1.5) = -8 to floor(-3.3 / 1.5) = -3, y from floor(0.8) = 0 to 2, z from floor(-1.4) = -2 to 1
        assert (c.x0, c.nx, c.y0, c.ny, c.z0, c.nz) == (-8, 6, 0, 3, -2, 4)
    if (leaf, k) == (0.5, 2):    # the edge 5.0 belongs to cell 5, the edge -5.0 to cell -5
        assert (c.x0, c.nx, c.y0, c.ny, c.z0, c.nz) == (1, 5, -5, 5, 3, 1)
    if (leaf, k) == (0.2, 1):
        assert (c.x0, c.nx, c.y0, c.ny, c.z0, c.nz) == (0, 1, 0, 1, 0, 1)
    # one number serves the three axes
    s = loamx.dist_window(0.5, 1.0, 2.0, 3.0, 4.0)
    t = loamx.dist_window(0.5, 1.0, 2.0, 3.0, (4.0, 4.0, 4.0))
    assert bytes(s) == bytes(t)


def test_dist_window_refusals():
    L = loamx.lib()
    c = loamx.DistConfig(cell_leaves=1, x0=5, nx=7)
    F3 = C.c_float * 3
    for leaf, centre, half, word in ((0.5, (0, 0, 0), (300.0, 1, 1), b"nx"),            # 1201 cells
                                     (0.5, (0, 0, 0), (1, 256.25, 1), b"ny"),           # 1026 cells; 255.75 below gives 1024
                                     (0.5, (0, 0, 0), (1, 1, 1e4), b"nz"),
                                     (0.5, (2e6, 0, 0), (1, 1, 1), b"x0"),
                                     (0.5, (0, -2e6, 0), (1, 1, 1), b"y0"),
                                     (0.5, (0, 0, 2e6), (1, 1, 1), b"z0"),
                                     (0.5, (0, 0, 0), (255.75, 255.75, 255.75), b"nx * ny * nz"),   # 1024^3
                                     (0.0, (0, 0, 0), (1, 1, 1), b"leaf"),
                                     (0.5, (np.nan, 0, 0), (1, 1, 1), b"centre"),
                                     (0.5, (0, 0, np.inf), (1, 1, 1), b"centre"),
                                     (0.5, (0, 0, 0), (1, -1.0, 1), b"half_extent")):
        assert L.loamx_densemap_dist_window(C.c_float(leaf), F3(*centre), F3(*half), C.byref(c)) == loamx.E_INVALID, (centre, half)
        assert word in L.loamx_last_error(), (word, L.loamx_last_error())
        assert (c.cell_leaves, c.x0, c.nx, c.y0, c.ny, c.z0, c.nz) == (1, 5, 7, 0, 32, 0, 128)    # unchanged
    assert L.loamx_densemap_dist_window(C.c_float(0.5), F3(), F3(), None) == loamx.E_INVALID
    assert L.loamx_densemap_dist_window(C.c_float(0.5), None, F3(), C.byref(c)) == loamx.E_INVALID and b"centre" in L.loamx_last_error()
    assert L.loamx_densemap_dist_window(C.c_float(0.5), F3(), None, C.byref(c)) == loamx.E_INVALID and b"half_extent" in L.loamx_last_error()
    big = loamx.dist_window(0.5, 0.0, 0.0, 0.0, (255.75, 15.75, 255.75), cell_leaves=1)
    assert (big.x0, big.nx, big.y0, big.ny, big.z0, big.nz) == (-512, 1024, -32, 64, -512, 1024) and big.check() is big
    with pytest.raises(loamx.LoamxError):
        loamx.dist_window(0.5, 0.0, 0.0, 0.0, 1.0, cell_leaves=65)


# ---- the near word and the metres
def test_near_pack_and_unpack():
    L = loamx.lib()
    for cell in ((0, 0, 0), (1, 2, 3), (1023, 0, 0), (0, 1023, 0), (0, 0, 1023), (1023, 1023, 1023), (5, 1023, 512)):
        w = xm.pack(*cell)
        assert w < 2 ** 30 and loamx.dist_near_unpack(w) == cell == xm.unpack(w)
    rx, ry, rz = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    for bad in (loamx.DIST_NONE, 1 << 30, 1 << 31):
        assert L.loamx_dist_near_unpack(C.c_uint32(bad), C.byref(rx), C.byref(ry), C.byref(rz)) == loamx.E_INVALID
        assert b"near" in L.loamx_last_error() and (rx.value, ry.value, rz.value) == (7, 7, 7)    # nothing written
    assert L.loamx_dist_near_unpack(C.c_uint32(0), None, C.byref(ry), C.byref(rz)) == loamx.E_INVALID
    with pytest.raises(loamx.LoamxError):
        loamx.dist_near_unpack(loamx.DIST_NONE)


def test_dist_metres():
    assert loamx.dist_metres(0, 0.5, 2) == 0.0
    assert loamx.dist_metres(25, 0.5, 2) == 5.0
    for d2, leaf, k in ((2, 0.1, 3), (65025, 0.05, 64), (3, 0.2, 1)):
        assert loamx.dist_metres(d2, leaf, k) == float(np.sqrt(np.float64(d2)) * np.float64(np.float32(leaf)) * np.float64(k))


# ---- the model: the brute force against the separable statement
def test_model_brute_force_equals_the_separable_passes():
    rng = np.random.default_rng(17)
    ties = 0
    for t in range(60):
        shape = tuple(int(v) for v in rng.integers(1, 8, 3))
        R = int(rng.integers(0, 6))
        occ = rng.random(shape) < rng.choice([0.02, 0.1, 0.4])
        a, b = xm.field(occ, R), xm.separable(occ, R)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (t, shape, R)
        assert a[0].dtype == np.uint16 and a[1].dtype == np.uint32
        # how many cells had a choice: more than one occupied cell at the distance
        sites = np.argwhere(occ)
        for z, y, x in np.argwhere(a[1] != xm.NONE).tolist():
            ties += int((((sites - (z, y, x)) ** 2).sum(1) == int(a[0][z, y, x])).sum() > 1)
    assert ties >= 100    # (a statement about these inputs: the tie rule is exercised on hundreds of cells)


def test_model_designed_ties():
    """Two, four and eight occupied cells at one distance: near is the smallest (rz, ry, rx)."""
    occ = np.zeros((3, 3, 3), bool)
    occ[0, 0, 0] = occ[0, 0, 2] = True
    d2, near = xm.field(occ, 5)
    assert d2[0, 0, 1] == 1 and near[0, 0, 1] == xm.pack(0, 0, 0)    # two at distance 1 along x: the smaller x
    occ[0, 2, 0] = occ[0, 2, 2] = True
    d2, near = xm.field(occ, 5)
    assert d2[0, 1, 1] == 2 and near[0, 1, 1] == xm.pack(0, 0, 0)    # four at distance 2 in the plane
    assert d2[0, 2, 1] == 1 and near[0, 2, 1] == xm.pack(0, 2, 0)    # the nearer pair wins over the smaller y
    occ[2] = occ[0]
    d2, near = xm.field(occ, 5)
    assert d2[1, 1, 1] == 3 and near[1, 1, 1] == xm.pack(0, 0, 0)    # eight corners at distance 3
    assert d2[2, 1, 1] == 2 and near[2, 1, 1] == xm.pack(0, 0, 2)    # four in the cell's own plane: rz = 2 although rz = 0 is smaller
    assert np.array_equal(d2, xm.separable(occ, 5)[0]) and np.array_equal(near, xm.separable(occ, 5)[1])
    # the cap: R = 1 keeps only distance 1; everything else is (R + 1)^2 = 4 and names nobody
    d2, near = xm.field(occ, 1)
    assert d2[1, 1, 1] == 4 and near[1, 1, 1] == xm.NONE and d2[0, 0, 1] == 1 and d2[0, 0, 0] == 0 and near[0, 0, 0] == xm.pack(0, 0, 0)
    # R = 0: 0 on occupied cells, 1 elsewhere; an empty volume: every cell capped
    d2, near = xm.field(occ, 0)
    assert np.array_equal(d2, np.where(occ, 0, 1)) and np.all((near == xm.NONE) == ~occ)
    d2, near = xm.field(np.zeros((2, 3, 4), bool), 7)
    assert np.all(d2 == 64) and np.all(near == xm.NONE)


def pts(*xyz):
    p = np.zeros((len(xyz), 4), np.float32)
    p[:, :3] = xyz
    return p


def test_model_floor_division_and_min_points():
    """k = 3: voxel index -1 lies in cell -1 and -4 in cell -2 on every axis (truncation would give 0 and -1)."""
    m = dm.Model(leaf=LEAF)
    m.add(pts((-0.25, -0.25, -0.25), (-1.75, 0.1, 0.1), (-1.75, 0.1, 0.1)), (0.0, 0.0, 0.0))
    occ, voxels = xm.occupied(m, cell_leaves=3, x0=-2, y0=-2, z0=-2, nx=3, ny=3, nz=3, min_points=1)
    assert voxels == 2 and np.argwhere(occ).tolist() == [[1, 1, 1], [2, 2, 0]]    # (rz, ry, rx)
    occ, voxels = xm.occupied(m, cell_leaves=3, x0=-2, y0=-2, z0=-2, nx=3, ny=3, nz=3, min_points=2)
    assert voxels == 1 and np.argwhere(occ).tolist() == [[2, 2, 0]]
    # the centre cell reaches every cell of the 3 x 3 x 3 window within 3; the corner cell is nearer to its own three neighbours
    d2, near, st = xm.dist(m, cell_leaves=3, x0=-2, y0=-2, z0=-2, nx=3, ny=3, nz=3, min_points=1, d_max=2)
    assert st == dict(voxels=2, occupied=2, within=27, max_d2=3) and d2[0, 0, 2] == 3 and near[0, 0, 2] == xm.pack(1, 1, 1)
    assert d2[1, 1, 0] == 1 and near[1, 1, 0] == xm.pack(1, 1, 1) and near[2, 1, 0] == xm.pack(0, 2, 2)
    # d_max 1: the two cells, the six neighbours of the centre and the three of the corner; everything else is capped at 4
    d2, near, st = xm.dist(m, cell_leaves=3, x0=-2, y0=-2, z0=-2, nx=3, ny=3, nz=3, min_points=1, d_max=1)
    assert st == dict(voxels=2, occupied=2, within=11, max_d2=1) and d2[0, 0, 2] == 4 and near[0, 0, 2] == xm.NONE


def test_model_cell_of_point():
    """leaf 0.5, k = 2, the window [-2, 2) cells on every axis: a cell is one metre.  A point on a face belongs to the cell above
    it; -0.0 is 0; a NaN, an infinity and a point beyond the key range have no cell."""
    cfg = dict(cell_leaves=2, x0=-2, y0=-2, z0=-2, nx=4, ny=4, nz=4)
    p = pts((0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (-1e-6, 0.0, 0.0), (1.999, 1.999, 1.999),
            (2.0, 0.0, 0.0), (-2.0, -2.0, -2.0), (-2.001, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, 6e5), (0.0, 0.0, 5.2e5))
    inside, record = xm.cells_of_points(p, LEAF, **cfg)
    assert inside.tolist() == [True, True, True, True, True, True, False, True, False, False, False, False, False]
    rec = lambda rx, ry, rz: (rz * 4 + ry) * 4 + rx
    assert record[inside].tolist() == [rec(2, 2, 2), rec(2, 2, 2), rec(3, 2, 2), rec(1, 2, 2), rec(1, 2, 2), rec(3, 3, 3), rec(0, 0, 0)]
    d2 = np.arange(64, dtype=np.uint16).reshape(4, 4, 4)
    near = np.where(d2 % 2 == 0, xm.NONE, 5).astype(np.uint32)
    out, st = xm.query(d2, near, p, LEAF, min_d2=42, **cfg)
    assert out["d2"].tolist()[:2] == [42, 42] and out["d2"][6] == xm.OUTSIDE and out["near"][6] == xm.NONE
    assert st == dict(inside=7, outside=6, capped=3, below=3, best=(0 << 32) | 7)    # records 42, 42, 43, 41, 41, 63 and 0
    assert xm.query(d2, near, p[8:], LEAF, **cfg)[1] == dict(inside=0, outside=5, capped=0, below=0, best=2 ** 64 - 1)


def test_model_on_the_scene_of_the_gpu_test():
    """the recipe of tests/test_gpu_densemap_dist.py: 541 voxels, 23 of them dynamic, and the occupied cells its windows must show"""
    S = rm.box_cast_scene()
    m = cm.CarveModel(leaf=S["leaf"])
    for p, o in S["sweeps"]:
        m.add(p, o)
    assert len(m) == 541 and int(m.dynamic_mask().sum()) == 23
    for cfg, rule, want in ((dict(cell_leaves=1, x0=-8, y0=-6, z0=-5, nx=17, ny=13, nz=9), None, OCCUPIED["k1", None]),
                            (dict(cell_leaves=1, x0=-8, y0=-6, z0=-5, nx=17, ny=13, nz=9), cm.DEFAULT_RULE, OCCUPIED["k1", cm.DEFAULT_RULE]),
                            (dict(cell_leaves=2, x0=-4, y0=-4, z0=-3, nx=9, ny=8, nz=6), None, OCCUPIED["k2", None]),
                            (dict(cell_leaves=3, x0=-3, y0=-3, z0=-3, nx=7, ny=6, nz=5), None, OCCUPIED["k3", None])):
        occ, voxels = xm.occupied(m, rule, min_points=1, **cfg)
        assert (voxels, int(occ.sum())) == want, (cfg, rule)


# (qualifying voxels, occupied cells) per (window, rule), from a separate prototype of the definition that counts straight from the points
OCCUPIED = {("k1", None): (541, 541), ("k1", cm.DEFAULT_RULE): (518, 518), ("k2", None): (541, 148), ("k3", None): (541, 60)}
