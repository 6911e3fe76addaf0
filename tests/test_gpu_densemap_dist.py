"""GPU: the dense map's distance field (include/loamx.h, loamx_densemap_dist and loamx_densemap_dist_query) against its model
(tests/densemap_dist_model.py over the models of the map and of carving).  Leaf 0.5, initial_slots 1024, the box scene of the ray-cast
tests with carving on: 541 voxels (the table grows), 23 of them dynamic under the default rule.  Every compared quantity is an integer:
the bytes of d2 and of near equal the model's, no tolerance anywhere; beside that the occupied-cell counts of the three windows are the
ones worked out with a separate prototype of the definition, which counts straight from the points, so that a model and a kernel that
are wrong together still trip."""
import ctypes as C

import numpy as np
import pytest

import densemap_carve_model as cm
import densemap_dist_model as xm
import densemap_grid_model as gm
import densemap_model as dm
import densemap_raycast_model as rm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

LEAF = 0.5
BASE = dict(min_points=1, d_max=3)
# the box's voxels span ix -6..6, iy -5..5, iz -4..2
WINDOWS = {"k1": dict(cell_leaves=1, x0=-8, y0=-6, z0=-5, nx=17, ny=13, nz=9), "k2": dict(cell_leaves=2, x0=-4, y0=-4, z0=-3, nx=9, ny=8, nz=6),
           "k3": dict(cell_leaves=3, x0=-3, y0=-3, z0=-3, nx=7, ny=6, nz=5)}
# (qualifying voxels, occupied cells) per (window, rule)
OCCUPIED = {("k1", None): (541, 541), ("k1", cm.DEFAULT_RULE): (518, 518), ("k2", None): (541, 148), ("k2", cm.DEFAULT_RULE): (518, 138),
            ("k3", None): (541, 60), ("k3", cm.DEFAULT_RULE): (518, 59)}


def new_map(initial_slots=1024, carving=True):
    d = loamx.DenseMap(leaf=LEAF, initial_slots=initial_slots)
    if carving:
        d.enable_carving()
    return d


def feed(target, sweeps):
    for p, o in sweeps:
        r = target.add(p, o)
        assert r == loamx.OK or r is True
    return target


def device_dist(d, rule=None, **cfg):
    d2, near = d.dist(static=None if rule is None else loamx.StaticRule(*rule), want_near=True, **cfg)
    return d2, near, dict(d.dist_stats)


def exports(d):
    st = d.stats()
    st.pop("slots")
    return dict(stats=st, points=d.points().tobytes(), misses=d.misses().tobytes(), carve_stats=d.carve_stats())


def explain(got, want):
    """the first cell that differs (for the assertion message)"""
    for name, g, w in (("d2", got[0], want[0]), ("near", got[1], want[1])):
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"{name}: {g.shape} {g.dtype}, {w.shape} {w.dtype}"
        for z, y, x in np.argwhere(g != w).tolist():
            return f"{name}[z {z}, y {y}, x {x}]: got {g[z, y, x]}, want {w[z, y, x]}"
    return f"stats: got {got[2]}, want {want[2]}"


def check(got, want):
    ok = (got[0].dtype == np.uint16 and got[1].dtype == np.uint32 and got[0].shape == want[0].shape == got[1].shape
          and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2])
    assert ok, explain(got, want)


@pytest.fixture(scope="module")
def scene():
    S = rm.box_cast_scene()
    S["model"] = feed(cm.CarveModel(leaf=LEAF), S["sweeps"])
    S["map"] = feed(new_map(), S["sweeps"])
    assert len(S["model"]) == len(S["map"]) == 541 and int(S["model"].dynamic_mask().sum()) == 23
    assert S["map"].rehashes >= 1 and S["map"].stats()["slots"] > 1024
    assert S["map"].points().tobytes() == S["model"].points().tobytes() and S["map"].misses().tobytes() == S["model"].misses().tobytes()
    S["want"] = {}
    return S


def want_of(S, rule=None, **cfg):
    """the model's field of a setting, computed once"""
    key = (rule, tuple(sorted(cfg.items())))
    if key not in S["want"]:
        S["want"][key] = xm.dist(S["model"], rule, **cfg)
    return S["want"][key]


# ---- 1: the three windows with and without the rule, and the counts of the prototype ---------------------------------------------------
@pytest.mark.parametrize("rule", [None, cm.DEFAULT_RULE], ids=["plain", "rule"])
@pytest.mark.parametrize("win", list(WINDOWS))
def test_windows_equal_the_model(scene, win, rule):
    cfg = dict(BASE, **WINDOWS[win])
    got = device_dist(scene["map"], rule, **cfg)
    print(win, rule, got[2])
    check(got, want_of(scene, rule, **cfg))
    d2, near, st = got
    assert d2.shape == (cfg["nz"], cfg["ny"], cfg["nx"])
    assert (st["voxels"], st["occupied"]) == OCCUPIED[(win, rule)]
    assert int((d2 == 0).sum()) == st["occupied"] and int((near != xm.NONE).sum()) == st["within"] and st["max_d2"] <= 9
    assert np.all((d2 == 16) == (near == xm.NONE)) and np.all(d2[near != xm.NONE] <= 9)
    # an occupied cell names itself, and every named cell is occupied
    zz, yy, xx = np.nonzero(d2 == 0)
    assert np.array_equal(near[d2 == 0], xm.pack(xx, yy, zz).astype(np.uint32))
    named = np.unique(near[near != xm.NONE])
    assert np.all(d2[named >> 20, (named >> 10) & 1023, named & 1023] == 0)
    if rule is not None:
        plain = want_of(scene, None, **cfg)
        assert d2.tobytes() != plain[0].tobytes() and near.tobytes() != plain[1].tobytes()    # the rule changes at least one cell


# ---- 2: windows of other shapes, and the settings -------------------------------------------------------------------------------------------
SHAPES = {"x_is_1": dict(cell_leaves=1, x0=-6, y0=-6, z0=-5, nx=1, ny=13, nz=9), "y_is_1": dict(cell_leaves=1, x0=-8, y0=-5, z0=-5, nx=17, ny=1, nz=9),
          "z_is_1": dict(cell_leaves=1, x0=-8, y0=-6, z0=2, nx=17, ny=13, nz=1),
          "37x5x53": dict(cell_leaves=1, x0=-18, y0=-6, z0=-26, nx=37, ny=5, nz=53, d_max=40),
          "65x3x129": dict(cell_leaves=1, x0=-32, y0=-5, z0=-64, nx=65, ny=3, nz=129, d_max=70),
          "129x2x65": dict(cell_leaves=1, x0=-64, y0=4, z0=-32, nx=129, ny=2, nz=65, d_max=100),
          "3x70x3": dict(cell_leaves=1, x0=-7, y0=-35, z0=-5, nx=3, ny=70, nz=3, d_max=33),
          "2x300x2_R254": dict(cell_leaves=1, x0=-6, y0=-150, z0=-4, nx=2, ny=300, nz=2, d_max=254),    # the largest halo, along y
          "2x2x300_R254": dict(cell_leaves=1, x0=-6, y0=-5, z0=-150, nx=2, ny=2, nz=300, d_max=254),    # and along z
          "outside": dict(cell_leaves=1, x0=100, y0=7, z0=-200, nx=19, ny=3, nz=7),
          "far_corner": dict(cell_leaves=64, x0=-2 ** 21, y0=-1, z0=2 ** 21, nx=3, ny=2, nz=2),
          "R0": dict(WINDOWS["k1"], d_max=0), "R1": dict(WINDOWS["k1"], d_max=1), "R254": dict(WINDOWS["k1"], d_max=254),
          "R40": dict(WINDOWS["k2"], d_max=40),    # larger than the window
          "min_points5": dict(WINDOWS["k1"], min_points=5), "min_points_above_all": dict(WINDOWS["k1"], min_points=10 ** 6)}


@pytest.mark.parametrize("rule", [None, cm.DEFAULT_RULE], ids=["plain", "rule"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_window_shapes(scene, shape, rule):
    cfg = dict(BASE, **SHAPES[shape])
    got = device_dist(scene["map"], rule, **cfg)
    check(got, want_of(scene, rule, **cfg))
    d2, near, st = got
    R = cfg["d_max"]
    if shape in ("outside", "far_corner", "min_points_above_all"):
        assert st == dict(voxels=0, occupied=0, within=0, max_d2=0) and np.all(d2 == (R + 1) ** 2) and np.all(near == xm.NONE)
    else:
        assert st["occupied"] > 0 and st["within"] >= st["occupied"]
    if shape in ("37x5x53", "65x3x129", "129x2x65", "3x70x3", "2x300x2_R254", "2x2x300_R254"):    # more than one word and more than one tile, distances far beyond one tile
        assert st["max_d2"] > 20 * 20 and len(np.unique(d2)) > 50
    if shape == "R0":
        assert np.all((d2 == 0) | (d2 == 1)) and st["within"] == st["occupied"] and st["max_d2"] == 0
    if shape == "R1":
        assert set(np.unique(d2).tolist()) == {0, 1, 4}
    if shape in ("R254", "R40"):    # every cell of the window is within R of the box
        assert st["within"] == d2.size and d2.max() == st["max_d2"] < 17 * 17 + 13 * 13 + 9 * 9
    if shape == "min_points5" and rule is None:
        assert (st["voxels"], st["occupied"]) == (504, 504)    # the prototype's


def test_one_cell_windows(scene):
    ix, iy, iz = gm.indices_of(scene["model"].keys[0])
    got = device_dist(scene["map"], cell_leaves=1, x0=ix, y0=iy, z0=iz, nx=1, ny=1, nz=1, **BASE)
    assert got[0].tolist() == [[[0]]] and got[1].tolist() == [[[0]]] and got[2] == dict(voxels=1, occupied=1, within=1, max_d2=0)
    assert xm.occupied(scene["model"], cell_leaves=1, x0=0, y0=0, z0=0, nx=1, ny=1, nz=1, min_points=1)[1] == 0    # mid-air, inside the box
    got = device_dist(scene["map"], cell_leaves=1, x0=0, y0=0, z0=0, nx=1, ny=1, nz=1, **BASE)
    assert got[0].tolist() == [[[16]]] and got[1].tolist() == [[[xm.NONE]]] and got[2] == dict(voxels=0, occupied=0, within=0, max_d2=0)


def test_a_cut_window_ignores_what_lies_outside(scene):
    """the window ix -5 .. -2, iy -2 .. 2, iz -2 .. 0 lies just inside the -x wall (ix = -6): in the whole box its first column is one
    cell from the wall, in the cut window the wall is no obstacle and only the six mid-air voxels inside count"""
    whole = want_of(scene, **dict(BASE, **WINDOWS["k1"], d_max=20))
    cfg = dict(BASE, cell_leaves=1, x0=-5, y0=-2, z0=-2, nx=4, ny=5, nz=3, d_max=20)
    got = device_dist(scene["map"], **cfg)
    check(got, want_of(scene, **cfg))
    assert (got[2]["voxels"], got[2]["occupied"]) == (6, 6)    # the prototype's
    sub = whole[0][3:6, 4:9, 3:7]
    assert np.all(sub[:, :, 0] == 1) and got[0][0, 0, 0] == 6 and np.any(got[0] > sub)
    assert np.all(got[0] >= sub) and np.array_equal(got[0] == 0, sub == 0)
    # half of the box: the bytes are the model's, the counts the prototype's
    cfg = dict(BASE, cell_leaves=1, x0=0, y0=-6, z0=-5, nx=5, ny=13, nz=9, d_max=20)
    got = device_dist(scene["map"], **cfg)
    check(got, want_of(scene, **cfg))
    assert (got[2]["voxels"], got[2]["occupied"]) == (181, 181)


# ---- 3: ties ---------------------------------------------------------------------------------------------------------------------------------
def test_designed_ties():
    """Eight single-voxel adds at the corners of a cube of side 4 whose lowest corner is voxel (-2, -2, -2), window 7 x 7 x 7 from
    (-3, -3, -3): the cells on the cube's mid-planes are equidistant from two, four and eight corners."""
    corners = [(x, y, z) for z in (-2, 2) for y in (-2, 2) for x in (-2, 2)]
    d, m = new_map(carving=False), dm.Model(leaf=LEAF)
    for c in corners:
        p = np.zeros((1, 4), np.float32)
        p[0, :3] = [(v + 0.5) * LEAF for v in c]
        feed(d, [(p, (0.0, 0.0, 0.0))])
        feed(m, [(p, (0.0, 0.0, 0.0))])
    cfg = dict(cell_leaves=1, x0=-3, y0=-3, z0=-3, nx=7, ny=7, nz=7, min_points=1, d_max=6)
    got = device_dist(d, **cfg)
    check(got, xm.dist(m, **cfg))
    d2, near, st = got
    assert st["occupied"] == 8
    assert d2[3, 3, 3] == 12 and near[3, 3, 3] == xm.pack(1, 1, 1)    # eight at distance 12: the smallest (rz, ry, rx)
    assert d2[1, 3, 3] == 8 and near[1, 3, 3] == xm.pack(1, 1, 1)     # four in the plane rz = 1
    assert d2[5, 3, 3] == 8 and near[5, 3, 3] == xm.pack(1, 1, 5)     # four in the plane rz = 5: the plane decides before y and x
    assert d2[3, 1, 3] == 8 and near[3, 1, 3] == xm.pack(1, 1, 1) and d2[3, 5, 3] == 8 and near[3, 5, 3] == xm.pack(1, 5, 1)
    assert d2[1, 1, 3] == 4 and near[1, 1, 3] == xm.pack(1, 1, 1) and d2[5, 5, 3] == 4 and near[5, 5, 3] == xm.pack(1, 5, 5)    # two
    assert d2[3, 5, 5] == 4 and near[3, 5, 5] == xm.pack(5, 5, 1) and d2[5, 3, 1] == 4 and near[5, 3, 1] == xm.pack(1, 1, 5)
    # the same with the cap between the distances: 4 and 8 stay, 12 is capped
    got = device_dist(d, **dict(cfg, d_max=3))
    check(got, xm.dist(m, **dict(cfg, d_max=3)))
    assert got[0][3, 3, 3] == 16 and got[1][3, 3, 3] == xm.NONE and got[0][1, 3, 3] == 8 and got[1][5, 3, 3] == xm.pack(1, 1, 5)


# ---- 4: independence of the table, and buffers that grow ------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["wide", "loaded"])
def test_field_does_not_depend_on_the_table(scene, tmp_path, how):
    if how == "wide":
        d = feed(new_map(initial_slots=1 << 20), scene["sweeps"])
        assert d.stats()["slots"] == 1 << 20 and d.rehashes == 0
    else:
        path = str(tmp_path / "map.lxdm")
        scene["map"].save(path)
        d = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
        d.load(path)
    for cfg in [dict(BASE, **w) for w in WINDOWS.values()] + [dict(BASE, **SHAPES["37x5x53"])]:
        for rule in (None, cm.DEFAULT_RULE):
            got = device_dist(d, rule, **cfg)
            check(got, want_of(scene, rule, **cfg))
            check(got, device_dist(scene["map"], rule, **cfg))


def test_small_large_small_window_on_one_handle(scene):
    d = feed(new_map(), scene["sweeps"])    # a handle of its own: its buffers have never been allocated
    large = dict(BASE, cell_leaves=1, x0=-40, y0=-10, z0=-30, nx=80, ny=20, nz=60, d_max=9)
    small = dict(BASE, **WINDOWS["k3"])
    for cfg in (small, large, small, dict(BASE, **WINDOWS["k1"]), large, small):
        check(device_dist(d, **cfg), want_of(scene, **cfg))
    assert want_of(scene, **large)[2]["occupied"] == OCCUPIED[("k1", None)][1]    # the whole box inside the large window


def test_the_map_is_untouched(scene):
    d = scene["map"]
    before = exports(d)
    for i in range(6):
        cfg = dict(BASE, **list(WINDOWS.values())[i % 3], d_max=i)
        rule = cm.DEFAULT_RULE if i % 2 else None
        check(device_dist(d, rule, **cfg), want_of(scene, rule, **cfg))
        d.dist_query(scene["sweeps"][0][0])
    assert exports(d) == before


# ---- 5: want_d2 / want_near, NULL cfg, the empty map -----------------------------------------------------------------------------------------
def test_planes_wanted_and_defaults(scene):
    d = scene["map"]
    cfg = dict(BASE, **WINDOWS["k2"])
    want = want_of(scene, **cfg)
    d2, near = d.dist(**cfg)
    assert near is None and d2.tobytes() == want[0].tobytes() and d.dist_stats == want[2]
    d2, near = d.dist(want_d2=False, want_near=True, **cfg)
    assert d2 is None and near.tobytes() == want[1].tobytes() and d.dist_stats == want[2]
    assert d.dist(want_d2=False, **cfg) == (None, None) and d.dist_stats == want[2]
    # NULL cfg: the defaults (128 x 32 x 128 from the origin, k = 2, min_points 2, d_max 16)
    L = loamx.lib()
    out = np.zeros((128, 32, 128), np.uint16)
    st = (C.c_uint64 * 4)()
    assert L.loamx_densemap_dist(d.h, None, None, out.ctypes.data_as(C.c_void_p), None, st) == loamx.OK
    want = want_of(scene)
    assert out.tobytes() == want[0].tobytes() and dict(zip(xm.STATS, (int(v) for v in st))) == want[2] and want[2]["occupied"] > 0
    check(device_dist(d), want)


@pytest.mark.parametrize("carving", [False, True])
def test_empty_map(carving):
    d = new_map(carving=carving)
    for cfg in (dict(), dict(BASE, **WINDOWS["k1"]), dict(cell_leaves=1, nx=37, ny=5, nz=53, d_max=0)):
        got = device_dist(d, cm.DEFAULT_RULE if carving else None, **cfg)
        check(got, xm.dist(cm.CarveModel(leaf=LEAF) if carving else dm.Model(leaf=LEAF), cm.DEFAULT_RULE if carving else None, **cfg))
        R = cfg.get("d_max", 16)
        assert np.all(got[0] == (R + 1) ** 2) and np.all(got[1] == xm.NONE) and got[2] == dict(voxels=0, occupied=0, within=0, max_d2=0)
    assert len(d) == 0 and d.stats()["offered"] == 0


# ---- 6: the query ----------------------------------------------------------------------------------------------------------------------------
QCFG = dict(BASE, **WINDOWS["k2"], d_max=1)    # d2 is 0, 1 or the cap 4; cells of one metre: cx in [-4, 5), cy in [-4, 4), cz in [-3, 3)


def query_points():
    e = [(0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (1.0, 0.0, 0.0), (-1.0, 1.0, -1.0), (-1e-6, 0.0, 0.0), (-1.0000001, 0.0, 0.0),
         (4.999, 3.999, 2.999), (-4.0, -4.0, -3.0), (0.5, 0.5, 0.5), (2.999999, -3.0, 2.0),
         (5.0, 0.0, 0.0), (-4.001, 0.0, 0.0), (0.0, 4.0, 0.0), (0.0, 0.0, -3.0001), (100.0, 100.0, 100.0),    # outside the window
         (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf), (6e5, 0.0, 0.0), (0.0, -5.3e5, 0.0), (5.2e5, 0.0, 0.0)]
    p = np.zeros((len(e), 4), np.float32)
    p[:, :3] = e
    rng = np.random.default_rng(23)
    r = np.zeros((300, 4), np.float32)
    r[:, :3] = rng.uniform([-5, -5, -4], [6, 5, 4], (300, 3))
    return np.concatenate([p, r])


def test_query(scene):
    d = scene["map"]
    d2, near, _ = device_dist(d, **QCFG)
    p = query_points()
    for min_d2 in (0, 5, 4, 1):
        got, st = d.dist_query(p, min_d2=min_d2)
        want, wst = xm.query(d2, near, p, LEAF, min_d2=min_d2, **QCFG)
        assert got.dtype == loamx.DIST_SAMPLE and got.tobytes() == want.tobytes() and st == wst, (min_d2, st, wst)
    assert st["inside"] + st["outside"] == len(p) and st["outside"] >= 11 and st["capped"] > 0 and 0 < st["below"] < st["inside"]
    assert np.all(got["d2"][10:21] == xm.OUTSIDE) and np.all(got["near"][10:21] == xm.NONE) and np.all(got["d2"][:10] != xm.OUTSIDE)
    assert got[0].tobytes() == got[1].tobytes() and got["d2"][2] == d2[3, 4, 5] and got["d2"][3] == d2[2, 5, 3] and got["d2"][4] == d2[3, 4, 3]
    # counts only
    none, st2 = d.dist_query(p, min_d2=1, records=False)
    assert none is None and st2 == st
    # the packed minimum: the smaller index of two points that share it
    zz, yy, xx = (int(v[0]) for v in np.nonzero(d2 == 0))
    hit = np.zeros((1, 4), np.float32)
    hit[0, :3] = (xx - 4 + 0.5, yy - 4 + 0.5, zz - 3 + 0.5)
    free = p[np.flatnonzero(want["d2"] != 0)[:5]]
    got, st = d.dist_query(np.concatenate([free, hit, free, hit, hit]))
    assert st["best"] == (0 << 32) | 5 and got["d2"][5] == 0 and loamx.dist_near_unpack(got["near"][5]) == (xx, yy, zz)
    got, st = d.dist_query(free[:1])
    assert st["best"] == (int(got["d2"][0]) << 32) | 0
    assert d.dist_query(p[10:21])[1] == dict(inside=0, outside=11, capped=0, below=0, best=2 ** 64 - 1)
    # an empty cloud
    got, st = d.dist_query(np.zeros((0, 4), np.float32))
    assert len(got) == 0 and st == dict(inside=0, outside=0, capped=0, below=0, best=2 ** 64 - 1)
    # (N, 8) records
    got8, st8 = d.dist_query(loamx.to_pcl_layout(p), min_d2=4)
    want, wst = xm.query(d2, near, p, LEAF, min_d2=4, **QCFG)
    assert got8.tobytes() == want.tobytes() and st8 == wst


def test_query_refusals(scene):
    L = loamx.lib()
    p = query_points()
    cloud = loamx.cloud_of(p)
    buf = np.full(len(p) * 8, 0xAB, np.uint8)
    st = (C.c_uint64 * 5)(*[77] * 5)
    fresh = feed(new_map(), scene["sweeps"][:1])
    args = (C.byref(cloud), C.c_uint32(0), buf.ctypes.data_as(C.c_void_p), C.c_uint64(len(p)), st)
    assert L.loamx_densemap_dist_query(fresh.h, *args) == loamx.E_INVALID and b"no distance field" in L.loamx_last_error()
    fresh.dist(want_d2=False, **QCFG)
    assert L.loamx_densemap_dist_query(fresh.h, C.byref(cloud), C.c_uint32(0), buf.ctypes.data_as(C.c_void_p), C.c_uint64(len(p) - 1), st) == loamx.E_CAPACITY
    assert L.loamx_densemap_dist_query(fresh.h, None, C.c_uint32(0), None, C.c_uint64(0), st) == loamx.E_INVALID and b"points" in L.loamx_last_error()
    assert L.loamx_densemap_dist_query(fresh.h, C.byref(cloud), C.c_uint32(0), None, C.c_uint64(0), None) == loamx.E_INVALID and b"stats" in L.loamx_last_error()
    assert buf.tobytes() == bytes([0xAB]) * len(buf) and list(st) == [77] * 5    # nothing written
    assert L.loamx_densemap_dist_query(fresh.h, *args) == loamx.OK and list(st)[0] > 0 and buf.tobytes() != bytes([0xAB]) * len(buf)
    fresh.reset()
    with pytest.raises(loamx.LoamxError) as e:
        fresh.dist_query(p)
    assert e.value.code == loamx.E_INVALID and "no distance field" in str(e.value)
    fresh.dist(**QCFG)    # the empty map's field: every point inside is capped
    got, qs = fresh.dist_query(p)
    assert qs["capped"] == qs["inside"] > 0 and np.all(got["d2"][got["d2"] != xm.OUTSIDE] == 4)


# ---- 7: refusals leave the field of the call before ------------------------------------------------------------------------------------------
def test_refusals_keep_the_field(scene):
    d, L = scene["map"], loamx.lib()
    before = exports(d)
    plain = feed(new_map(carving=False), scene["sweeps"][:1])
    good = loamx.DistConfig(**QCFG)
    n = good.nx * good.ny * good.nz
    p = query_points()
    want_d2, want_near, _ = device_dist(d, **QCFG)
    ref, ref_st = d.dist_query(p, min_d2=4)
    plain.dist(good)
    plain_ref = plain.dist_query(p)[0].tobytes()
    b2, bn = np.full(n, 0xABAB, np.uint16), np.full(n, 0xABABABAB, np.uint32)
    p2, pn = b2.ctypes.data_as(C.c_void_p), bn.ctypes.data_as(C.c_void_p)
    st = (C.c_uint64 * 4)(*[77] * 4)
    rule, bad_rule = loamx.StaticRule(), loamx.StaticRule(den=0)
    cases = [(lambda: L.loamx_densemap_dist(plain.h, C.byref(good), C.byref(rule), p2, pn, st), b"carving"),
             (lambda: L.loamx_densemap_dist(d.h, C.byref(good), C.byref(bad_rule), p2, pn, st), b"den"),
             (lambda: L.loamx_densemap_dist(d.h, C.byref(good.copy(d_max=255)), None, p2, pn, st), b"d_max"),
             (lambda: L.loamx_densemap_dist(d.h, C.byref(good.copy(nx=0)), None, p2, pn, st), b"nx"),
             (lambda: L.loamx_densemap_dist(d.h, C.byref(good.copy(ny=1025)), None, p2, pn, st), b"ny"),
             (lambda: L.loamx_densemap_dist(d.h, C.byref(good.copy(nx=1024, ny=1024, nz=65)), None, p2, pn, st), b"nx * ny * nz"),
             (lambda: L.loamx_densemap_dist(d.h, C.byref(good.copy(cell_leaves=65)), None, p2, pn, st), b"cell_leaves"),
             (lambda: L.loamx_densemap_dist(d.h, C.byref(good.copy(z0=2 ** 21 + 1)), None, p2, pn, st), b"z0"),
             (lambda: L.loamx_densemap_dist(d.h, C.byref(good.copy(min_points=0)), None, p2, pn, st), b"min_points"),
             (lambda: L.loamx_densemap_dist(d.h, C.byref(good), None, p2, pn, None), b"stats is NULL"),
             (lambda: L.loamx_densemap_dist(None, C.byref(good), None, p2, pn, st), b"h is NULL")]
    for call, word in cases:
        assert call() == loamx.E_INVALID and word in L.loamx_last_error(), word
        assert np.all(b2 == 0xABAB) and np.all(bn == 0xABABABAB) and list(st) == [77] * 4    # nothing written
        got, got_st = d.dist_query(p, min_d2=4)    # the field of the call before answers as before
        assert got.tobytes() == ref.tobytes() and got_st == ref_st, word
        assert plain.dist_query(p)[0].tobytes() == plain_ref, word
    with pytest.raises(loamx.LoamxError) as e:
        d.dist(good, d_max=300)
    assert e.value.code == loamx.E_INVALID and "d_max" in str(e.value)
    with pytest.raises(loamx.LoamxError) as e:
        plain.dist(good, static=rule)
    assert e.value.code == loamx.E_INVALID and "carving" in str(e.value)
    assert exports(d) == before
    assert L.loamx_densemap_dist(d.h, C.byref(good), None, p2, pn, st) == loamx.OK
    assert b2.tobytes() == want_d2.tobytes() and bn.tobytes() == want_near.tobytes()
