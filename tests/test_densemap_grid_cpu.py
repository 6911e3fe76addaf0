"""CPU: the dense map's navigation grid (include/loamx.h, loamx_densemap_grid ...) — every new symbol declared and exported, the two
structs laid out as a C compiler lays them out, the defaults, every bound of loamx_densemap_grid_check, loamx_densemap_grid_window
against its formula, loamx_grid_occupancy and loamx_write_grid_pgm byte for byte; and the model the GPU tests check the device against
(tests/densemap_grid_model.py), checked here against cases worked out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_carve_model as cm
import densemap_grid_model as gm
import densemap_model as dm
import densemap_raycast_model as rm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_grid_default_config", "loamx_densemap_grid_check", "loamx_densemap_grid_window", "loamx_densemap_grid",
               "loamx_grid_occupancy", "loamx_write_grid_pgm")
LEAF = 0.5   # inv = 2 exactly: voxel i spans [0.5 i, 0.5 (i + 1))


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert "} loamx_densemap_grid_config;" in hdr and "} loamx_grid_cell;" in hdr
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    assert callable(loamx.DenseMap.grid)
    for name in ("grid_window", "grid_occupancy", "write_grid_pgm", "GridConfig"):
        assert callable(getattr(loamx, name)), name
    for k, name in enumerate(("UNKNOWN", "FREE", "OBSTACLE", "STEP")):
        assert f"#define LOAMX_GRID_{name} {k}\n" in hdr and getattr(loamx, "GRID_" + name) == getattr(gm, name) == k
    assert "A step beyond the window's edge" in hdr   # the limit the header owes its readers


@pytest.mark.parametrize("c_name,py", [("loamx_densemap_grid_config", "GridConfig"), ("loamx_grid_cell", "GridCell")])
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
    if py == "GridCell":
        assert got[0] == 24 == loamx.GRID_CELL.itemsize == gm.GRID_CELL.itemsize
        assert loamx.GRID_CELL == gm.GRID_CELL and loamx.GRID_NONE == gm.NONE == 2 ** 31 - 1
    else:
        assert fields == list(gm.DEFAULTS)


def test_defaults():
    c = loamx.GridConfig()
    assert {f: getattr(c, f) for f, _ in c._fields_} == gm.DEFAULTS
    assert gm.DEFAULTS == dict(cell_leaves=2, x0=0, z0=0, nx=256, nz=256, min_points=2, y_min=-2 ** 20, y_max=2 ** 20, band_lo=3, band_hi=20,
                               min_obstacle_voxels=1, max_step=2, clear_max=10)
    loamx.lib().loamx_densemap_grid_default_config(None)   # NULL: nothing to fill
    assert c.check() is c and gm.check(gm.DEFAULTS) is None
    assert loamx.GridConfig(nx=3, clear_max=0).copy(nz=5).nx == 3


# (field, values accepted at the edge of the bound, values refused just beyond it, fields set beside it)
BOUNDS = [("cell_leaves", (1, 64), (0, 65), {}),
          ("x0", (-2 ** 21, 2 ** 21), (-2 ** 21 - 1, 2 ** 21 + 1), {}),
          ("z0", (-2 ** 21, 2 ** 21), (-2 ** 21 - 1, 2 ** 21 + 1), {}),
          ("nx", (1, 8192), (0, 8193), {}),
          ("nz", (1, 8192), (0, 8193), {}),
          ("min_points", (1, 2 ** 32 - 1), (0,), {}),
          ("y_min", (7, -2 ** 31), (8,), dict(y_max=7)),
          ("band_lo", (1, 9), (0,), dict(band_hi=9)),
          ("band_hi", (5, 2 ** 32 - 1), (4,), dict(band_lo=5)),
          ("min_obstacle_voxels", (1, 2 ** 32 - 1), (0,), {}),
          ("max_step", (0, 2 ** 32 - 1), (), {}),
          ("clear_max", (0, 64), (65,), {})]


@pytest.mark.parametrize("field,good,bad,beside", BOUNDS, ids=[b[0] for b in BOUNDS])
def test_check_bounds(field, good, bad, beside):
    L = loamx.lib()
    for v in good:
        c = loamx.GridConfig(**beside, **{field: v})
        assert L.loamx_densemap_grid_check(C.byref(c)) == loamx.OK, (field, v)
        assert gm.check(dict(gm.DEFAULTS, **beside, **{field: v})) is None
    for v in bad:
        c = loamx.GridConfig(**beside, **{field: v})
        assert L.loamx_densemap_grid_check(C.byref(c)) == loamx.E_INVALID, (field, v)
        assert field.encode() in L.loamx_last_error(), (field, L.loamx_last_error())
        assert gm.check(dict(gm.DEFAULTS, **beside, **{field: v})) == field
        with pytest.raises(loamx.LoamxError):
            c.check()


def test_check_the_product_and_null():
    L = loamx.lib()
    # nx * nz <= 2^26: its last accepted value is 8192 x 8192; a larger product needs a factor above 8192, which its own bound refuses first
    assert L.loamx_densemap_grid_check(C.byref(loamx.GridConfig(nx=8192, nz=8192))) == loamx.OK
    assert L.loamx_densemap_grid_check(None) == loamx.E_INVALID and b"cfg" in L.loamx_last_error()
    out = np.zeros(4, loamx.GRID_CELL)
    assert L.loamx_densemap_grid(None, None, None, out.ctypes.data_as(C.c_void_p)) == loamx.E_INVALID and b"h is NULL" in L.loamx_last_error()


# ---- loamx_densemap_grid_window against its formula
@pytest.mark.parametrize("leaf,k,cx,cz,half", [(0.5, 3, -7.3, 2.2, 4.0),      # a negative centre with k = 3
                                               (0.5, 2, 3.0, -3.0, 2.0),      # exactly on a cell edge on both sides (e = 1)
                                               (0.1, 2, 12.34, -0.05, 25.0),  # a leaf that is no binary fraction
                                               (0.2, 1, 0.0, 0.0, 0.0),       # no extent: the one cell of the centre
                                               (0.5, 64, -1e5, 1e5, 1000.0)])
def test_grid_window(leaf, k, cx, cz, half):
    c = loamx.grid_window(leaf, cx, cz, half, cell_leaves=k)
    assert (c.x0, c.nx) == gm.window(leaf, cx, half, k) and (c.z0, c.nz) == gm.window(leaf, cz, half, k)
    assert c.cell_leaves == k and c.check() is c
    rest = {f: getattr(c, f) for f in gm.DEFAULTS if f not in ("cell_leaves", "x0", "z0", "nx", "nz")}
    assert rest == {f: gm.DEFAULTS[f] for f in rest}    # the other fields are left alone
    if (leaf, k, cx) == (0.5, 3, -7.3):
        assert (c.x0, c.nx, c.z0, c.nz) == (-8, 6, -2, 7)          # e = 1.5: x from floor(-11.3 / 1.5) = -8 to floor(-3.3 / 1.5) = -3, z from floor(-1.2) = -2 to 4
    if (leaf, k, cx) == (0.5, 2, 3.0):
        assert (c.x0, c.nx, c.z0, c.nz) == (1, 5, -5, 5)           # the edge 5.0 belongs to cell 5, the edge -5.0 to cell -5
    if half == 0.0:
        assert (c.x0, c.nx, c.z0, c.nz) == (0, 1, 0, 1)


def test_grid_window_refusals():
    L = loamx.lib()
    c = loamx.GridConfig(cell_leaves=1, x0=5, nx=7)
    for args, word in (((0.5, 0.0, 0.0, 5000.0), b"nx"),            # 20001 cells
                       ((0.5, 0.0, 0.0, 2048.25), b"nx"),           # 8194 cells; 2047.75 below gives 8192
                       ((0.5, 2e6, 0.0, 1.0), b"x0"),
                       ((0.5, 0.0, -2e6, 1.0), b"z0"),
                       ((0.0, 0.0, 0.0, 1.0), b"leaf"),
                       ((0.5, np.nan, 0.0, 1.0), b"centre_x"),
                       ((0.5, 0.0, np.inf, 1.0), b"centre_z"),
                       ((0.5, 0.0, 0.0, -1.0), b"half_extent")):
        assert L.loamx_densemap_grid_window(*(C.c_float(a) for a in args), C.byref(c)) == loamx.E_INVALID, args
        assert word in L.loamx_last_error(), (args, L.loamx_last_error())
        assert (c.cell_leaves, c.x0, c.nx, c.z0, c.nz) == (1, 5, 7, 0, 256)    # unchanged
    assert L.loamx_densemap_grid_window(C.c_float(0.5), C.c_float(0), C.c_float(0), C.c_float(1), None) == loamx.E_INVALID
    big = loamx.grid_window(0.5, 0.0, 0.0, 2047.75, cell_leaves=1)
    assert (big.x0, big.nx, big.z0, big.nz) == (-4096, 8192, -4096, 8192)
    with pytest.raises(loamx.LoamxError):
        loamx.grid_window(0.5, 0.0, 0.0, 1.0, cell_leaves=65)


# ---- loamx_grid_occupancy and loamx_write_grid_pgm on hand-written cells
def cells_of(cls):
    a = np.zeros(np.shape(cls), loamx.GRID_CELL)
    a["cls"] = cls
    return a


def test_grid_occupancy():
    cells = cells_of([[gm.FREE, gm.OBSTACLE, gm.UNKNOWN], [gm.STEP, gm.FREE, gm.UNKNOWN]])
    occ = loamx.grid_occupancy(cells)
    assert occ.dtype == np.int8 and occ.tolist() == [[0, 100, -1], [100, 0, -1]] and np.array_equal(occ, gm.occupancy(cells))
    assert loamx.grid_occupancy(cells[:0]).shape == (0, 3)
    bad = cells_of([gm.FREE, 4])
    out = np.full(2, 7, np.int8)
    L = loamx.lib()
    assert L.loamx_grid_occupancy(bad.ctypes.data_as(C.c_void_p), C.c_uint64(2), out.ctypes.data_as(C.c_void_p)) == loamx.E_INVALID
    assert b"cls" in L.loamx_last_error() and out.tolist() == [7, 7]    # nothing written


def test_write_grid_pgm(tmp_path):
    # nx = 2, nz = 3: cells[cz - z0, cx - x0]
    cells = cells_of([[gm.FREE, gm.OBSTACLE], [gm.UNKNOWN, gm.STEP], [gm.FREE, gm.UNKNOWN]])
    cfg = loamx.GridConfig(cell_leaves=2, x0=-3, z0=4, nx=2, nz=3)
    stem = str(tmp_path / "nav")
    loamx.write_grid_pgm(stem, cells, cfg, 0.25)
    # width nz = 3, height nx = 2; row 0 is the cells of cx = x0 + 1 along cz, row 1 those of cx = x0
    assert open(stem + ".pgm", "rb").read() == b"P5\n3 2\n255\n" + bytes([0, 0, 205, 254, 205, 254])
    assert bytes([0, 0, 205, 254, 205, 254]) == gm.pgm_bytes(cells)
    assert open(stem + ".yaml").read() == ("image: nav.pgm\nresolution: 0.5\norigin: [2, -1.5, 0]\nnegate: 0\n"
                                           "occupied_thresh: 0.65\nfree_thresh: 0.196\n")
    loamx.write_grid_pgm(stem, cells, cfg, 0.1)    # resolution = (double)0.1f * 2, nine significant digits
    res = float(np.float32(0.1)) * 2
    assert "%.9g" % res == "0.200000003"
    assert open(stem + ".yaml").read().splitlines()[1:3] == ["resolution: 0.200000003", "origin: [%.9g, %.9g, 0]" % (4 * res, -3 * res)]
    L = loamx.lib()
    p = cells.ctypes.data_as(C.c_void_p)
    assert L.loamx_write_grid_pgm(None, p, C.byref(cfg), C.c_float(0.25)) == loamx.E_INVALID and b"stem" in L.loamx_last_error()
    assert L.loamx_write_grid_pgm(stem.encode(), None, C.byref(cfg), C.c_float(0.25)) == loamx.E_INVALID and b"cells" in L.loamx_last_error()
    assert L.loamx_write_grid_pgm(stem.encode(), p, None, C.c_float(0.25)) == loamx.E_INVALID and b"cfg" in L.loamx_last_error()
    assert L.loamx_write_grid_pgm(stem.encode(), p, C.byref(cfg), C.c_float(0.0)) == loamx.E_INVALID and b"leaf" in L.loamx_last_error()
    assert L.loamx_write_grid_pgm(str(tmp_path / "no" / "nav").encode(), p, C.byref(cfg), C.c_float(0.25)) == loamx.E_INVALID


# ---- the model against cases worked out by hand (leaf 0.5; a point at ((i + f) * 0.5) lies in voxel i at the fraction f)
def pts(*xyz):
    p = np.zeros((len(xyz), 4), np.float32)
    p[:, :3] = xyz
    return p


def model_of(*xyz):
    m = dm.Model(leaf=LEAF)
    m.add(pts(*xyz), (0.0, 0.0, 0.0))
    return m


def test_model_a_lone_point_under_the_floor():
    """One column, k = 1: three points in voxel (0, 0, 0), the floor, and one stray point in voxel (0, -3, 0).  With min_points 1 the
    stray voxel is the ground, the floor lies 3 leaves above it, inside the default band 3..20: one obstacle voxel, OBSTACLE.  With
    min_points 2 the stray voxel does not qualify: the ground is the floor, nothing above it, FREE."""
    m = model_of((0.2, 0.2, 0.2), (0.3, 0.2, 0.2), (0.2, 0.2, 0.3), (0.2, -1.3, 0.2))
    g = gm.grid(m, nx=1, nz=1, cell_leaves=1, min_points=1)[0, 0]
    assert (g["ground"], g["obstacles"], g["overhead"], g["cls"], g["clear2"]) == (-3, 1, gm.NONE, gm.OBSTACLE, 0)
    assert abs(g["elevation"] + 1.3) < 1e-6
    g = gm.grid(m, nx=1, nz=1, cell_leaves=1, min_points=2)[0, 0]
    assert (g["ground"], g["obstacles"], g["overhead"], g["cls"], g["clear2"]) == (0, 0, gm.NONE, gm.FREE, 121)
    assert abs(g["elevation"] - 0.2) < 1e-6
    # a band that ends below the floor turns it into the overhead
    g = gm.grid(m, nx=1, nz=1, cell_leaves=1, min_points=1, band_lo=1, band_hi=2)[0, 0]
    assert (g["ground"], g["obstacles"], g["overhead"], g["cls"]) == (-3, 0, 0, gm.FREE)


def test_model_floor_division():
    """k = 3: ix = -1 and ix = -3 lie in cell -1, ix = -4 in cell -2 (truncation would give 0, -1, -1).  Window x0 = -2, nx = 3."""
    m = model_of((-0.25, 0.1, 0.1), (-1.25, 0.1, 0.1), (-1.75, 0.1, 0.1))
    assert sorted(gm.indices_of(k)[0] for k in m.keys) == [-4, -3, -1]
    g = gm.grid(m, cell_leaves=3, x0=-2, z0=0, nx=3, nz=1, min_points=1)
    assert g["cls"].tolist() == [[gm.FREE, gm.FREE, gm.UNKNOWN]] and g["ground"].tolist() == [[0, 0, gm.NONE]]
    # iz alike, on the other axis of the record index: record (cz - z0) * nx + (cx - x0)
    m = model_of((0.1, 0.1, -0.25), (0.1, 0.1, -2.25))    # iz = -1 -> cz = -1, iz = -5 -> cz = -2
    g = gm.grid(m, cell_leaves=3, x0=0, z0=-2, nx=2, nz=3, min_points=1)
    assert g["cls"].tolist() == [[gm.FREE, gm.UNKNOWN], [gm.FREE, gm.UNKNOWN], [gm.UNKNOWN, gm.UNKNOWN]]


def test_model_elevation_pools_the_ground_layer():
    """k = 2: voxel (0, 0, 0) holds one point at the fraction 1/4 of its height, voxel (1, 0, 1) three at 3/4.  Both are the ground
    layer of cell (0, 0): SSn = 4, SSy = (1 * 1/4 + 3 * 3/4) * 2^20, elevation = (0 + 10/16) * 0.5 = 0.3125 exactly.  A voxel one
    layer up, in the same cell, is neither pooled nor (band 3..20) an obstacle."""
    m = model_of((0.1, 0.125, 0.1), (0.6, 0.375, 0.6), (0.7, 0.375, 0.7), (0.6, 0.375, 0.7), (0.1, 0.625, 0.1))
    g = gm.grid(m, cell_leaves=2, nx=1, nz=1, min_points=1)[0, 0]
    assert (g["ground"], g["obstacles"], g["cls"]) == (0, 0, gm.FREE) and g["elevation"] == np.float32(0.3125)
    # the record of the download of a single voxel is the same expression: a one-voxel ground layer gives its y
    one = model_of((0.1, 0.125, 0.1), (0.2, 0.2, 0.2))
    assert gm.grid(one, cell_leaves=2, nx=1, nz=1)[0, 0]["elevation"] == one.points()[0, 1]


def test_model_staircase():
    """Ground levels 0, 1, 4 in three neighbouring cells, max_step 2: |0 - 1| = 1 is no step, |1 - 4| = 3 is one and marks both of
    its sides: FREE, STEP, STEP.  With max_step 3 all three are FREE; with the window cut after the second cell the step is not seen."""
    m = dm.Model(leaf=LEAF)
    m.add(gm.staircase_points([0, 1, 4], LEAF, 1, depth=1), (0.0, 0.0, 0.0))
    g = gm.grid(m, cell_leaves=1, nx=3, nz=1)
    assert g["ground"].tolist() == [[0, 1, 4]] and g["cls"].tolist() == [[gm.FREE, gm.STEP, gm.STEP]]
    assert g["clear2"].tolist() == [[1, 0, 0]]
    assert gm.grid(m, cell_leaves=1, nx=3, nz=1, max_step=3)["cls"].tolist() == [[gm.FREE] * 3]
    assert gm.grid(m, cell_leaves=1, nx=2, nz=1)["cls"].tolist() == [[gm.FREE, gm.FREE]]


def test_model_clear2_around_one_obstacle():
    """A 7 x 7 floor (k = 1, two points per voxel) with one voxel 3 leaves above it over the centre cell.  R = 0: 0 on the obstacle,
    1 elsewhere.  R = 1: the four neighbours have 1, everything else, the diagonals (D = 2 > 1) included, the cap 4.  R = 2: 1, 2 and
    4 as they are, the knight's moves (D = 5 > 4) and beyond the cap 9."""
    xyz = [((ix + 0.5) * LEAF, 0.25, (iz + 0.5) * LEAF) for ix in range(7) for iz in range(7)] * 2
    xyz += [(3.5 * LEAF, 3.25 * LEAF, 3.5 * LEAF)] * 2
    m = model_of(*xyz)
    for R in (0, 1, 2):
        g = gm.grid(m, cell_leaves=1, nx=7, nz=7, clear_max=R)
        assert gm.class_counts(g) == (0, 48, 1, 0) and g["cls"][3, 3] == gm.OBSTACLE
        want = [[(x - 3) ** 2 + (z - 3) ** 2 for x in range(7)] for z in range(7)]
        want = [[d if d <= R * R else (R + 1) ** 2 for d in row] for row in want]
        assert g["clear2"].tolist() == want
    assert g["clear2"][3].tolist() == [9, 4, 1, 0, 1, 4, 9] and g["clear2"][2].tolist() == [9, 9, 2, 1, 2, 9, 9]
    # an obstacle outside the window does not count
    assert gm.grid(m, cell_leaves=1, nx=3, nz=7, clear_max=2)["clear2"].max() == 9 == gm.grid(m, cell_leaves=1, nx=3, nz=7, clear_max=2)["clear2"].min()


def test_model_rule_and_the_scene_of_the_gpu_test():
    """the recipe of tests/test_gpu_densemap_grid.py: 541 voxels, 23 of them dynamic, and the class counts its windows must show"""
    S = rm.box_cast_scene()
    m = cm.CarveModel(leaf=S["leaf"])
    for p, o in S["sweeps"]:
        m.add(p, o)
    assert len(m) == 541 and int(m.dynamic_mask().sum()) == 23
    base = dict(min_points=1, band_lo=1, band_hi=4, max_step=1, clear_max=3)
    for k, (x0, z0, nx, nz), rule, want in ((1, (-8, -5, 17, 11), None, (96, 38, 53)), (1, (-8, -5, 17, 11), cm.DEFAULT_RULE, (96, 48, 43)),
                                            (2, (-4, -3, 9, 6), None, (26, 3, 25)), (3, (-3, -2, 6, 4), None, (9, 0, 15))):
        g = gm.grid(m, rule, cell_leaves=k, x0=x0, z0=z0, nx=nx, nz=nz, **base)
        assert gm.class_counts(g)[:3] == want, (k, rule)
