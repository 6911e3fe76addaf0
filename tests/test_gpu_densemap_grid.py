"""GPU: the dense map's navigation grid (include/loamx.h, loamx_densemap_grid and what precedes it) against its model
(tests/densemap_grid_model.py over the models of the map and of carving).  Leaf 0.5, initial_slots 1024, the box scene of the ray-cast
tests with carving on: 541 voxels (the table grows), 23 of them dynamic under the default rule.  Every compared quantity is an integer
or the bits of a float: the bytes of the whole cell array equal the model's, no tolerance anywhere; beside that the class counts of the
three windows are the ones worked out with a separate prototype of the definition, so that a model and a kernel that are wrong together
still trip."""
import copy
import ctypes as C

import numpy as np
import pytest

import densemap_carve_model as cm
import densemap_grid_model as gm
import densemap_model as dm
import densemap_raycast_model as rm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

LEAF = 0.5
BASE = dict(min_points=1, band_lo=1, band_hi=4, max_step=1, clear_max=3)
WINDOWS = {"k1": dict(cell_leaves=1, x0=-8, z0=-5, nx=17, nz=11), "k2": dict(cell_leaves=2, x0=-4, z0=-3, nx=9, nz=6),
           "k3": dict(cell_leaves=3, x0=-3, z0=-2, nx=6, nz=4)}
# (UNKNOWN, FREE, OBSTACLE) cells per (window, rule)
CLASS_COUNTS = {("k1", None): (96, 38, 53), ("k1", cm.DEFAULT_RULE): (96, 48, 43), ("k2", None): (26, 3, 25), ("k3", None): (9, 0, 15)}


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


def device_grid(d, rule=None, **cfg):
    return d.grid(static=None if rule is None else loamx.StaticRule(*rule), **cfg)


def exports(d):
    st = d.stats()
    st.pop("slots")
    return dict(stats=st, points=d.points().tobytes(), misses=d.misses().tobytes(), carve_stats=d.carve_stats())


def explain(got, want):
    """the first cell that differs (for the assertion message)"""
    if got.shape != want.shape:
        return f"shapes {got.shape}, {want.shape}"
    for z, x in np.argwhere(np.array([[got[z, x].tobytes() != want[z, x].tobytes() for x in range(got.shape[1])] for z in range(got.shape[0])])):
        return f"cell [z {z}, x {x}]: got {got[z, x]}, want {want[z, x]}"
    return "equal"


def check(got, want):
    assert got.dtype == gm.GRID_CELL == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), explain(got, want)


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


def want_of(S, rule=None, model=None, tag="scene", **cfg):
    """the model's grid of a setting, computed once"""
    key = (tag, rule, tuple(sorted(cfg.items())))
    if key not in S["want"]:
        S["want"][key] = gm.grid(S["model"] if model is None else model, rule, **cfg)
    return S["want"][key]


# ---- 1: the three windows with and without the rule, and the class counts of the prototype ------------------------------------------
@pytest.mark.parametrize("rule", [None, cm.DEFAULT_RULE], ids=["plain", "rule"])
@pytest.mark.parametrize("win", list(WINDOWS))
def test_windows_equal_the_model(scene, win, rule):
    cfg = dict(BASE, **WINDOWS[win])
    got = device_grid(scene["map"], rule, **cfg)
    counts = gm.class_counts(got)
    print(win, rule, counts)
    check(got, want_of(scene, rule, **cfg))
    assert got.shape == (cfg["nz"], cfg["nx"]) and sum(counts) == cfg["nx"] * cfg["nz"]
    if (win, rule) in CLASS_COUNTS:
        assert counts[:3] == CLASS_COUNTS[(win, rule)]
    if rule is not None:
        assert got.tobytes() != want_of(scene, None, **cfg).tobytes()    # the rule changes at least one cell
    known = got["cls"] != gm.UNKNOWN
    assert np.all(got["ground"][~known] == gm.NONE) and np.all(got["elevation"][~known] == 0) and np.all(got["ground"][known] < gm.NONE)
    assert np.all(got["clear2"][got["cls"] >= gm.OBSTACLE] == 0) and np.all(got["clear2"][got["cls"] < gm.OBSTACLE] > 0)


# ---- 2: windows of other shapes ---------------------------------------------------------------------------------------------------------
SHAPES = {"one_cell": dict(cell_leaves=1, x0=0, z0=0, nx=1, nz=1), "one_cell_k3": dict(cell_leaves=3, x0=-1, z0=-1, nx=1, nz=1),
          "outside": dict(cell_leaves=1, x0=100, z0=-200, nx=19, nz=7), "half_box": dict(cell_leaves=1, x0=0, z0=-5, nx=9, nz=11),
          "37x53": dict(cell_leaves=1, x0=-18, z0=-26, nx=37, nz=53), "53x37_R64": dict(cell_leaves=1, x0=-30, z0=-9, nx=53, nz=37, clear_max=64),
          "far_corner": dict(cell_leaves=64, x0=-2 ** 21, z0=2 ** 21, nx=3, nz=2)}


@pytest.mark.parametrize("rule", [None, cm.DEFAULT_RULE], ids=["plain", "rule"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_window_shapes(scene, shape, rule):
    cfg = dict(BASE, **SHAPES[shape])
    got = device_grid(scene["map"], rule, **cfg)
    check(got, want_of(scene, rule, **cfg))
    if shape in ("outside", "far_corner"):
        assert gm.class_counts(got) == (cfg["nx"] * cfg["nz"], 0, 0, 0) and np.all(got["clear2"] == 16)    # (R + 1)^2
        assert np.all(got["ground"] == gm.NONE) and np.all(got["overhead"] == gm.NONE) and not got["obstacles"].any()
    if shape == "half_box":    # the cut column is the k1 window's from its ninth column on, but for the distances to what was cut off
        whole = want_of(scene, rule, **dict(BASE, **WINDOWS["k1"]))
        for f in ("ground", "elevation", "obstacles", "overhead"):
            assert np.array_equal(got[f], whole[f][:, 8:])
    if shape == "37x53":
        assert gm.class_counts(got)[1] > 0 and gm.class_counts(got)[2] > 0
    if shape == "53x37_R64":    # more than one tile of the clear kernel each way, and every distance inside the cap
        assert got["clear2"].max() < 65 * 65 and len(np.unique(got["clear2"])) > 20


# ---- 3: the settings ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 1, 5, 64])
def test_clear_max(scene, R):
    cfg = dict(BASE, **WINDOWS["k1"], clear_max=R)
    got = device_grid(scene["map"], **cfg)
    check(got, want_of(scene, **cfg))
    free = got["cls"] < gm.OBSTACLE
    assert np.all(got["clear2"][~free] == 0) and got["clear2"][free].min() >= 1 and got["clear2"].max() <= (R + 1) ** 2
    if R == 0:
        assert np.all(got["clear2"][free] == 1)
    if R == 1:
        assert set(np.unique(got["clear2"]).tolist()) == {0, 1, 4}


@pytest.mark.parametrize("name,kw", [("slab", dict(y_min=-4, y_max=3)), ("min_points5", dict(min_points=5)),
                                     ("min_obstacle_voxels3", dict(min_obstacle_voxels=3)), ("band", dict(band_lo=2, band_hi=2)),
                                     ("defaults", None)])
def test_settings(scene, name, kw):
    cfg = dict(BASE, **WINDOWS["k1"], **kw) if kw is not None else dict(WINDOWS["k1"])    # defaults: only the window is set
    base = want_of(scene, **dict(BASE, **WINDOWS["k1"]))
    for rule in (None, cm.DEFAULT_RULE):
        got = device_grid(scene["map"], rule, **cfg)
        check(got, want_of(scene, rule, **cfg))
    got = device_grid(scene["map"], **cfg)
    assert got.tobytes() != base.tobytes()    # the setting matters in this scene
    if name == "slab":    # without the floor (iy = -5) the ground is the walls' next layer
        lowest = base["ground"][base["cls"] != gm.UNKNOWN].min()
        assert lowest < -4 and got["ground"].min() == -4 and np.all(got["ground"][base["ground"] == lowest] > lowest)
        assert got["overhead"][got["overhead"] != gm.NONE].max(initial=-99) <= 3
    if name == "min_obstacle_voxels3":
        assert gm.class_counts(got)[2] < gm.class_counts(base)[2] and np.array_equal(got["obstacles"], base["obstacles"])


# ---- 4: a staircase built by hand ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_staircase(k):
    levels = [0, 1, 4, 4, 2, -3]    # steps of 1, 3, 0, 2 and 5 leaves; the bands start at cell -2: negative indices, floor division
    p = gm.staircase_points(levels, LEAF, k, depth=3, first=-2)
    d, m = new_map(carving=False), dm.Model(leaf=LEAF)
    for t in (d, m):
        feed(t, [(p, (0.0, 0.0, 0.0))])
    for max_step in (0, 1, 2, 4, 5):
        cfg = dict(cell_leaves=k, x0=-3, z0=-1, nx=8, nz=5, max_step=max_step)
        got = device_grid(d, **cfg)
        check(got, gm.grid(m, **cfg))
        row = got["cls"][2, 1:7].tolist()
        diffs = [abs(a - b) for a, b in zip(levels, levels[1:])]
        want = [gm.STEP if (i > 0 and diffs[i - 1] > max_step) or (i < 5 and diffs[i] > max_step) else gm.FREE for i in range(6)]
        assert row == want and got["ground"][2, 1:7].tolist() == levels    # both sides of a step are marked
        assert got["cls"][0].tolist() == [gm.UNKNOWN] * 8 and got["cls"][:, 0].tolist() == [gm.UNKNOWN] * 5
    # the window cut between the levels 1 and 4: the step beyond its edge is not seen
    got = device_grid(d, cell_leaves=k, x0=-2, z0=0, nx=2, nz=3, max_step=2)
    assert np.all(got["cls"] == gm.FREE)


# ---- 5: independence of the order of the points, of the calls and of the table ------------------------------------------------------------
@pytest.mark.parametrize("how", ["shuffled7", "wide", "loaded", "pruned"])
def test_grid_does_not_depend_on_the_table(scene, tmp_path, how):
    sweeps = scene["sweeps"]
    cfgs = [dict(BASE, **w) for w in WINDOWS.values()] + [dict(BASE, **SHAPES["37x53"])]
    rules = [None, cm.DEFAULT_RULE]
    if how == "shuffled7":    # no carving, no rule: the miss counts, and with them a rule's verdicts, depend on the split into calls
        allp = np.concatenate([p for p, _ in sweeps])
        allp = allp[np.random.default_rng(5).permutation(len(allp))]
        d = feed(new_map(carving=False), [(part, (0.0, 0.0, 0.0)) for part in np.array_split(allp, 7)])
        rules = [None]
    elif how == "wide":
        d = feed(new_map(initial_slots=1 << 20), sweeps)
        assert d.stats()["slots"] == 1 << 20 and d.rehashes == 0
    elif how == "loaded":
        path = str(tmp_path / "map.lxdm")
        scene["map"].save(path)
        d = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
        d.load(path)
    else:
        d = feed(new_map(), sweeps)
        model = copy.deepcopy(scene["model"])
        assert d.prune() == model.prune() == 23
        for cfg in cfgs:    # without its dynamic voxels the map answers as the whole map does under the rule
            got = device_grid(d, **cfg)
            check(got, want_of(scene, cm.DEFAULT_RULE, **cfg))
            check(got, want_of(scene, None, model, "pruned", **cfg))
        return
    for cfg in cfgs:
        for rule in rules:
            got = device_grid(d, rule, **cfg)
            check(got, want_of(scene, rule, **cfg))
            assert got.tobytes() == device_grid(scene["map"], rule, **cfg).tobytes()


# ---- 6: the map is only read, and the planes keep nothing from an earlier window ------------------------------------------------------------
def test_the_map_is_untouched(scene):
    d = scene["map"]
    before = exports(d)
    for i in range(10):
        cfg = dict(BASE, **list(WINDOWS.values())[i % 3], clear_max=i)
        check(device_grid(d, cm.DEFAULT_RULE if i % 2 else None, **cfg), want_of(scene, cm.DEFAULT_RULE if i % 2 else None, **cfg))
    assert exports(d) == before


def test_large_then_small_window(scene):
    d = feed(new_map(), scene["sweeps"])    # a handle of its own: its planes have never been allocated
    large = dict(BASE, cell_leaves=1, x0=-150, z0=-100, nx=300, nz=200, clear_max=9)
    small = dict(BASE, **WINDOWS["k3"])
    for cfg in (large, small, dict(BASE, **WINDOWS["k1"]), small):
        check(device_grid(d, **cfg), want_of(scene, **cfg))
    assert gm.class_counts(want_of(scene, **large))[1:3] == CLASS_COUNTS[("k1", None)][1:]    # the k1 window inside a sea of UNKNOWN


# ---- 7: refusals, and the empty map -----------------------------------------------------------------------------------------------------------
def test_refusals(scene):
    d, L = scene["map"], loamx.lib()
    before = exports(d)
    plain = feed(new_map(carving=False), scene["sweeps"][:1])
    good = loamx.GridConfig(**dict(BASE, **WINDOWS["k1"]))
    n = good.nx * good.nz
    buf = np.full(n * 24, 0xAB, np.uint8)
    bp = buf.ctypes.data_as(C.c_void_p)
    rule, bad_rule = loamx.StaticRule(), loamx.StaticRule(den=0)
    cases = [(lambda: L.loamx_densemap_grid(plain.h, C.byref(good), C.byref(rule), bp), b"carving"),
             (lambda: L.loamx_densemap_grid(d.h, C.byref(good), C.byref(bad_rule), bp), b"den"),
             (lambda: L.loamx_densemap_grid(d.h, C.byref(good.copy(clear_max=65)), None, bp), b"clear_max"),
             (lambda: L.loamx_densemap_grid(d.h, C.byref(good.copy(nx=0)), None, bp), b"nx"),
             (lambda: L.loamx_densemap_grid(d.h, C.byref(good.copy(cell_leaves=65)), None, bp), b"cell_leaves"),
             (lambda: L.loamx_densemap_grid(d.h, C.byref(good.copy(band_lo=0)), None, bp), b"band_lo"),
             (lambda: L.loamx_densemap_grid(d.h, C.byref(good), None, None), b"out is NULL"),
             (lambda: L.loamx_densemap_grid(None, C.byref(good), None, bp), b"h is NULL")]
    for call, word in cases:
        assert call() == loamx.E_INVALID and word in L.loamx_last_error(), word
        assert buf.tobytes() == bytes([0xAB]) * (n * 24)    # nothing written
    with pytest.raises(loamx.LoamxError) as e:
        d.grid(good, y_min=1, y_max=0)
    assert e.value.code == loamx.E_INVALID and "y_min" in str(e.value)
    with pytest.raises(loamx.LoamxError) as e:
        plain.grid(good, static=rule)
    assert e.value.code == loamx.E_INVALID and "carving" in str(e.value)
    # the handles are what they were, and the call after a refusal is right
    assert exports(d) == before
    assert L.loamx_densemap_grid(d.h, C.byref(good), None, bp) == loamx.OK
    assert buf.tobytes() == want_of(scene, **dict(BASE, **WINDOWS["k1"])).tobytes()
    # NULL cfg: the defaults
    out = np.zeros((256, 256), loamx.GRID_CELL)
    assert L.loamx_densemap_grid(d.h, None, None, out.ctypes.data_as(C.c_void_p)) == loamx.OK
    check(out, want_of(scene))
    check(d.grid(), out)


@pytest.mark.parametrize("carving", [False, True])
def test_empty_map(carving):
    d = new_map(carving=carving)
    for cfg in (dict(), dict(BASE, **WINDOWS["k1"]), dict(cell_leaves=1, nx=37, nz=53, clear_max=0)):
        got = d.grid(static=loamx.StaticRule() if carving else None, **cfg)
        check(got, gm.grid(dm.Model(leaf=LEAF), **cfg))
        R = cfg.get("clear_max", 10)
        assert np.all(got["cls"] == gm.UNKNOWN) and np.all(got["clear2"] == (R + 1) ** 2) and np.all(got["ground"] == gm.NONE)
    assert len(d) == 0 and d.stats()["offered"] == 0
