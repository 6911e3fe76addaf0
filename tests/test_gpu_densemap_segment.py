"""GPU: the dense map's connected components (include/loamx.h, loamx_densemap_segment) against their model
(tests/densemap_segment_model.py over the models of the map and of carving).  Leaf 0.5 and initial_slots 1024 unless stated; the
scenes are points at voxel centres fed through DenseMap.add.  Every compared quantity is an integer: the bytes of the labels and of
the records and the first five stats equal the model's, no tolerance anywhere; beside that the component counts are the ones worked
out by hand or with a separate prototype of the definition, so that a model and a kernel that are wrong together still trip."""
import ctypes as C

import numpy as np
import pytest

import densemap_carve_model as cm
import densemap_file_model as flm
import densemap_frontier_model as frm
import densemap_model as dm
import densemap_raycast_model as rm
import densemap_region_model as rgm
import densemap_route_model as rtm
import densemap_segment_cloud_model as scm
import densemap_segment_model as sm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

LEAF = 0.5
LIM = 2 ** 20 - 1
PAT = 0xa5a5a5a5
ORIGIN = (0.0, 0.0, 0.0)


def new_map(initial_slots=1024, carving=False):
    d = loamx.DenseMap(leaf=LEAF, initial_slots=initial_slots)
    if carving:
        d.enable_carving()
    return d


def feed(target, sweeps):
    for p, o in sweeps:
        r = target.add(p, o)
        assert r == loamx.OK or r is True
    return target


def sweeps_of(cells, counts=None, parts=1):
    """the points of the cells as `parts` adds"""
    p = sm.points_of_cells(cells, LEAF, counts)
    return [(q, ORIGIN) for q in np.array_split(p, parts) if len(q)]


def pair_of(cells, counts=None, parts=1, initial_slots=1024):
    """(device map, model) fed with the same adds"""
    sw = sweeps_of(cells, counts, parts)
    d, m = feed(new_map(initial_slots), sw), feed(dm.Model(leaf=LEAF), sw)
    assert len(d) == len(m) == len(set(map(tuple, np.asarray(cells).reshape(-1, 3).tolist())))
    return d, m


def explain(got, want):
    for j, (g, w) in enumerate(zip(got, want)):
        if g.tobytes() != w.tobytes():
            return f"item {j}: got {g}, want {w}"
    return f"lengths {len(got)}, {len(want)}"


def check(d, model, rule=None, **cfg):
    """one device call against the model: the bytes of both outputs and the five exact stats; returns the device's triple"""
    labels, segs, st = d.segment(static=None if rule is None else loamx.StaticRule(*rule), **cfg)
    wl, ws, wst = sm.segment(model, rule, **cfg)
    assert labels.dtype == np.uint32 and labels.tobytes() == wl.tobytes(), explain(labels, wl)
    assert segs.dtype == sm.SEGMENT and segs.tobytes() == ws.tobytes(), explain(segs, ws)
    assert {k: st[k] for k in sm.STAT_KEYS} == wst, (st, wst)
    return labels, segs, st


# ---- 1: empty and single ------------------------------------------------------------------------------------------------------------------
def test_empty_map():
    d = new_map()
    labels, segs, st = d.segment()
    assert len(labels) == 0 and len(segs) == 0 and all(v == 0 for v in st.values())
    rc, nv, ns, stats, _, _ = raw(d)
    assert (rc, nv, ns, stats) == (loamx.OK, 0, 0, [0] * 6)


@pytest.mark.parametrize("cell", [(0, 0, 0), (-1, -1, -1), (5, -7, 11)])
def test_single_voxel(cell):
    d, m = pair_of([cell], counts=[3])
    for conn in (6, 18, 26):
        labels, segs, st = check(d, m, connectivity=conn)
        assert labels.tolist() == [0] and (st["selected"], st["components"], st["kept"], st["largest"]) == (1, 1, 1, 1)
        r = segs[0]
        assert (r["min_key"], r["voxels"], r["points"]) == (cm.key_of(cell), 1, 3)
        assert r["lo"].tolist() == list(cell) == r["hi"].tolist() == r["sum_idx"].tolist()
    assert check(d, m, min_points=4)[2]["selected"] == 0


# ---- 2: pairs that share a face, an edge or a corner ------------------------------------------------------------------------------------------
PAIRS = {"face_x_across_zero": ((-1, 0, 0), (1, 0, 0), 1), "face_y": ((3, -2, 1), (0, 1, 0), 1), "face_z_negative": ((-5, -5, -5), (0, 0, -1), 1),
         "edge_xy": ((-1, 0, 2), (1, 1, 0), 2), "edge_yz_negative": ((-3, -1, -1), (0, 1, -1), 2), "edge_xz": ((0, 4, 0), (-1, 0, 1), 2),
         "corner": ((-1, -1, -1), (1, 1, 1), 3), "corner_mixed": ((0, 0, 0), (-1, 1, -1), 3), "corner_negative": ((-8, -9, -10), (1, -1, -1), 3)}


@pytest.mark.parametrize("conn", [6, 18, 26])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_pairs(pair, conn):
    a, d_, dist = PAIRS[pair]
    b = tuple(a[k] + d_[k] for k in range(3))
    d, m = pair_of([a, b])
    labels, segs, st = check(d, m, connectivity=conn)
    joined = dist <= {6: 1, 18: 2, 26: 3}[conn]
    assert st["components"] == (1 if joined else 2) and sorted(labels.tolist()) == ([0, 0] if joined else [0, 1])
    assert segs[0]["min_key"] == min(cm.key_of(a), cm.key_of(b))


# ---- 3: the edges of the key range ----------------------------------------------------------------------------------------------------------
EDGE_CELLS = [(LIM, 0, 0), (LIM - 1, 0, 0), (-LIM, 1, 0), (-LIM + 1, 1, 0),          # keys that differ by 2 across the x / y boundary
              (7, LIM, 0), (7, LIM - 1, 0), (7, -LIM, 1), (7, -LIM + 1, 1),          # and across the y / z boundary
              (0, 9, LIM), (0, 9, LIM - 1), (0, 9, -LIM), (0, 9, -LIM + 1),
              (LIM, LIM, LIM), (LIM - 1, LIM - 1, LIM - 1), (-LIM, -LIM, -LIM), (-LIM + 1, -LIM, -LIM + 1)]


@pytest.mark.parametrize("conn", [6, 18, 26])
def test_key_range_edges(conn):
    p = sm.points_of_cells(EDGE_CELLS, LEAF)
    assert abs(float(p[0, 0])) == 524287.75 and float(p[2, 0]) == -524287.25   # exact in f32
    d, m = pair_of(EDGE_CELLS)
    labels, segs, st = check(d, m, connectivity=conn)
    lab = dict(zip(m.keys.tolist(), labels.tolist()))
    of = lambda c: lab[cm.key_of(c)]
    for k in range(0, 12, 2):    # every edge voxel joins its in-range neighbour
        assert of(EDGE_CELLS[k]) == of(EDGE_CELLS[k + 1])
    assert of((LIM, 0, 0)) != of((-LIM, 1, 0)) and of((7, LIM, 0)) != of((7, -LIM, 1)) and of((0, 9, LIM)) != of((0, 9, -LIM))
    assert (of((LIM, LIM, LIM)) == of((LIM - 1, LIM - 1, LIM - 1))) == (conn == 26)
    assert (of((-LIM, -LIM, -LIM)) == of((-LIM + 1, -LIM, -LIM + 1))) == (conn >= 18)
    assert st["components"] == {6: 10, 18: 9, 26: 8}[conn]


# ---- 4: the long chain: a serpentine -----------------------------------------------------------------------------------------------------------
def serpentine(rows=24, width=24):
    """rows of `width` voxels two apart in y, joined alternately at the ends: one voxel wide, 24 * 24 + 23 = 599 voxels"""
    cells = []
    for r in range(rows):
        xs = range(width) if r % 2 == 0 else range(width - 1, -1, -1)
        cells += [(x, 2 * r, 0) for x in xs]
        if r + 1 < rows:
            cells.append((width - 1 if r % 2 == 0 else 0, 2 * r + 1, 0))
    return cells


@pytest.mark.parametrize("cut", [False, True], ids=["whole", "cut"])
def test_serpentine(cut):
    cells = serpentine()
    assert len(cells) == 599 and cm.key_of(cells[0]) == min(cm.key_of(c) for c in cells)   # the smallest key is at one end
    if cut:
        cells.remove((12, 24, 0))
    d, m = pair_of(cells[::-1], parts=8)   # (fed from the far end, in eight adds)
    assert d.rehashes >= 1 and d.stats()["slots"] > 1024
    for conn in (6, 18, 26):
        labels, segs, st = check(d, m, connectivity=conn)
        assert st["components"] == (2 if cut else 1) and st["largest"] == (312 if cut else 599)
        assert segs[0]["min_key"] == cm.key_of((0, 0, 0))
    if cut:
        # twelve rows, their twelve joints and x 0..11 of the thirteenth before the gap; x 13..23 and the rest behind it
        assert segs["voxels"].tolist() == [312, 286] and segs[1]["min_key"] == cm.key_of((13, 24, 0))


# ---- 5: many components, one component --------------------------------------------------------------------------------------------------------
def test_checkerboard():
    cells = [(i - 4, j - 4, k - 4) for i in range(8) for j in range(8) for k in range(8) if (i + j + k) % 2 == 0]
    d, m = pair_of(cells)
    for conn, n in ((6, 256), (18, 1), (26, 1)):
        labels, segs, st = check(d, m, connectivity=conn)
        assert (st["selected"], st["components"], st["largest"]) == (256, n, 256 // n)
    assert check(d, m, connectivity=6)[0].tolist() == list(range(256))   # every voxel its own component, numbered by key
    assert check(d, m, connectivity=6, min_voxels=2)[2]["kept"] == 0


def combs():
    """two combs whose teeth interleave in x and meet tip to tip by corners only"""
    a = [(x, 0, 0) for x in range(9)] + [(x, 0, z) for x in range(0, 9, 2) for z in (1, 2)]
    b = [(u, 1, 5) for u in range(1, 8)] + [(u, 1, z) for u in range(1, 8, 2) for z in (3, 4)]
    return a, b


def test_combs():
    a, b = combs()
    d, m = pair_of(a + b)
    for conn, n in ((6, 2), (18, 2), (26, 1)):
        labels, segs, st = check(d, m, connectivity=conn)
        assert st["components"] == n and st["selected"] == len(a) + len(b) == 34
    segs = check(d, m, connectivity=18)[1]
    assert segs["voxels"].tolist() == [len(a), len(b)] and segs[1]["lo"].tolist() == [1, 1, 3] and segs[1]["hi"].tolist() == [7, 1, 5]


@pytest.fixture(scope="module")
def cube():
    rng = np.random.default_rng(20)
    flat = rng.choice(16 ** 3, 2000, replace=False)
    cells = np.stack([flat % 16 - 8, (flat // 16) % 16 - 8, flat // 256 - 8], axis=1)
    counts = rng.integers(1, 4, 2000)
    d, m = pair_of(cells, counts, parts=3)
    assert d.rehashes >= 1
    return d, m


@pytest.mark.parametrize("conn", [6, 18, 26])
def test_random_cube(cube, conn):
    d, m = cube
    labels, segs, st = check(d, m, connectivity=conn)
    assert st["selected"] == 2000 and st["largest"] > 100 and st["components"] >= (50 if conn == 6 else 1)
    assert len(np.unique(segs["voxels"])) >= (4 if conn == 6 else 1)
    check(d, m, connectivity=conn, min_voxels=3)
    check(d, m, connectivity=conn, min_points=2)


# ---- 6: the window ------------------------------------------------------------------------------------------------------------------------------
def test_window_cuts_a_bar(cube):
    u = [(x, 0, 0) for x in range(-4, 5)] + [(-4, y, 0) for y in range(1, 4)] + [(4, y, 0) for y in range(1, 4)]   # a U
    d, m = pair_of(u)
    assert check(d, m)[2]["components"] == 1
    labels, segs, st = check(d, m, lo=(-LIM, 1, -LIM), hi=(LIM, LIM, LIM))   # without the bottom bar: the two uprights
    assert (st["selected"], st["components"]) == (6, 2) and segs["voxels"].tolist() == [3, 3] and int((labels == sm.NONE).sum()) == 9
    labels, segs, st = check(d, m, lo=(-3, 0, 0), hi=(3, 0, 0))              # the bar's middle alone
    assert (st["selected"], st["components"]) == (7, 1) and segs[0]["lo"].tolist() == [-3, 0, 0]
    assert check(d, m, lo=(50, 50, 50), hi=(60, 60, 60))[2]["selected"] == 0
    # lo == hi on one axis: a single slab of the random cube
    dc, mc = cube
    for a in range(3):
        lo, hi = [-LIM] * 3, [LIM] * 3
        lo[a] = hi[a] = -2
        for conn in (6, 26):
            labels, segs, st = check(dc, mc, connectivity=conn, lo=tuple(lo), hi=tuple(hi))
            assert 0 < st["selected"] < 2000 and np.all(segs["lo"][:, a] == -2) and np.all(segs["hi"][:, a] == -2)


# ---- 7: the box scene of the ray-cast tests, with carving -------------------------------------------------------------------------------------
TABLE = {(sm.ALL, 6): (15, [518, 3, 3, 2, 2, 2, 2, 2] + [1] * 7), (sm.ALL, 18): (2, [540, 1]), (sm.ALL, 26): (2, [540, 1]),
         (sm.STATIC, 6): (10, [507, 2, 2] + [1] * 7), (sm.STATIC, 18): (8, [508, 3, 2] + [1] * 5), (sm.STATIC, 26): (8, [508, 3, 2] + [1] * 5),
         (sm.DYNAMIC, 6): (15, [5, 4, 2] + [1] * 12), (sm.DYNAMIC, 18): (9, [7, 6, 3, 2] + [1] * 5), (sm.DYNAMIC, 26): (5, [11, 6, 3, 2, 1])}
Y_WINDOW = dict(lo=(-LIM, -4, -LIM), hi=(LIM, 4, LIM))


def exports(d):
    st = d.stats()
    return dict(stats=st, points=d.points().tobytes(), misses=d.misses().tobytes(), carve_stats=d.carve_stats())


@pytest.fixture(scope="module")
def scene():
    S = rm.box_cast_scene()
    S["model"] = feed(cm.CarveModel(leaf=LEAF), S["sweeps"])
    S["map"] = feed(new_map(carving=True), S["sweeps"])
    assert len(S["model"]) == len(S["map"]) == 541 and int(S["model"].dynamic_mask().sum()) == 23
    assert S["map"].rehashes >= 1 and S["map"].stats()["slots"] > 1024
    assert S["map"].points().tobytes() == S["model"].points().tobytes() and S["map"].misses().tobytes() == S["model"].misses().tobytes()
    return S


@pytest.mark.parametrize("which,conn", list(TABLE))
def test_box_scene_table(scene, which, conn):
    n, want = TABLE[(which, conn)]
    labels, segs, st = check(scene["map"], scene["model"], which=which, connectivity=conn)
    assert st["components"] == n and sorted(segs["voxels"].tolist(), reverse=True) == want and st["largest"] == want[0]
    assert st["selected"] == {sm.ALL: 541, sm.STATIC: 518, sm.DYNAMIC: 23}[which] == int((labels != sm.NONE).sum())


def test_box_scene_figures(scene):
    d, m = scene["map"], scene["model"]
    assert check(d, m, connectivity=6, min_voxels=2)[2]["kept"] == 8 and check(d, m, connectivity=6, min_voxels=3)[2]["kept"] == 3
    assert check(d, m, which=sm.DYNAMIC, min_voxels=2)[2]["kept"] == 4 and check(d, m, which=sm.DYNAMIC, min_voxels=3)[2]["kept"] == 3
    for conn in (6, 18, 26):
        st = check(d, m, connectivity=conn, min_points=2)[2]
        assert (st["selected"], st["components"]) == (507, 2)
        st = check(d, m, connectivity=conn, min_points=3)[2]
        assert (st["selected"], st["components"]) == (506, 1)
    for which, conn, sel, n, head in ((sm.ALL, 6, 359, 15, [336, 3, 3, 2, 2, 2, 2, 2]), (sm.ALL, 18, 359, 2, [358, 1]), (sm.ALL, 26, 359, 2, [358, 1]),
                                      (sm.STATIC, 6, 336, 10, [325]), (sm.STATIC, 26, 336, 8, [326])):
        segs, st = check(d, m, which=which, connectivity=conn, **Y_WINDOW)[1:]
        assert (st["selected"], st["components"]) == (sel, n) and sorted(segs["voxels"].tolist(), reverse=True)[:len(head)] == head


def test_box_scene_rules(scene):
    d, m = scene["map"], scene["model"]
    other = (40, 1, 1)   # dynamic only from 40 misses on: four of the 23 have fewer
    assert int(m.dynamic_mask(other).sum()) == 19
    for which in (sm.STATIC, sm.DYNAMIC):
        got = check(d, m, rule=other, which=which, connectivity=18)
        default = check(d, m, rule=None, which=which, connectivity=18)
        explicit = check(d, m, rule=cm.DEFAULT_RULE, which=which, connectivity=18)
        assert default[0].tobytes() == explicit[0].tobytes() and default[1].tobytes() == explicit[1].tobytes()
        assert got[0].tobytes() != default[0].tobytes()
    # with ALL the rule is not read: not even a den of 0 matters
    labels, segs, st = d.segment(static=loamx.StaticRule(1, 1, 0))
    assert labels.tobytes() == sm.segment(m)[0].tobytes()


def test_map_is_untouched(scene):
    d = scene["map"]
    before = exports(d)
    for which in (sm.ALL, sm.STATIC, sm.DYNAMIC):
        d.segment(which=which, connectivity=6)
        d.segment(which=which, labels=False, min_voxels=3, **Y_WINDOW)
    assert exports(d) == before


# ---- 8: the outputs depend on the set of voxels alone ---------------------------------------------------------------------------------------------
def test_invariance(scene, tmp_path):
    sweeps = scene["sweeps"]
    m = feed(dm.Model(leaf=LEAF), sweeps)
    maps = {"1024": feed(new_map(1024), sweeps), "65536": feed(new_map(1 << 16), sweeps), "reversed": feed(new_map(1024), sweeps[::-1])}
    assert maps["1024"].stats()["slots"] != maps["65536"].stats()["slots"] == 1 << 16 and maps["65536"].rehashes == 0
    maps["1024"].save(str(tmp_path / "box.lxdm"))
    maps["loaded"] = new_map(1024)
    maps["loaded"].load(str(tmp_path / "box.lxdm"))
    for cfg in (dict(connectivity=6), dict(connectivity=26, min_voxels=2), dict(connectivity=18, min_points=2, **Y_WINDOW)):
        want = sm.segment(m, **cfg)
        for name, d in maps.items():
            for _ in range(2):   # the same call twice
                labels, segs, st = check(d, m, **cfg)
                assert labels.tobytes() == want[0].tobytes() and segs.tobytes() == want[1].tobytes(), name


def test_call_grow_call():
    cells = serpentine(rows=8)   # 199 voxels: fits 1024 slots
    d, m = pair_of(cells)
    assert d.rehashes == 0
    check(d, m, connectivity=6)
    more = [(x, y, 1) for x in range(0, 24) for y in range(0, 40, 2)]   # a layer above that touches every row
    sw = sweeps_of(more, parts=4)
    feed(d, sw), feed(m, sw)
    assert d.rehashes >= 1 and len(d) == len(m) == 199 + len(more)
    labels, segs, st = check(d, m, connectivity=6)
    assert st["components"] == 13    # the serpentine and the eight rows above it, and twelve rows beyond its end
    check(d, m, connectivity=26)


# ---- 9: one scan state behind the region export, both labellers and the download of one handle ----------------------------------------------------
def test_one_scan_state_serves_every_user_of_a_handle():
    """download_region, segment, frontiers_cells, segment_cloud and download in turn on one handle, twice over and once more after the
    table has grown: the three users of the handle's chained-scan state (the region's compaction, the segments' two scans, the
    frontiers' scan) follow each other at four blocks of slots and five of cells, and every result equals its model"""
    cells = serpentine(rows=12)   # 299 voxels in 1,024 slots: four blocks of 256
    d, m = pair_of(cells)
    assert d.rehashes == 0 and d.stats()["slots"] == 1024
    rng = np.random.default_rng(33)
    cls = rng.choice(4, size=(33, 33), p=[0.25, 0.6, 0.1, 0.05])   # 2 x 2 tiles; 1,089 cells: five blocks of 256, the last of 65
    clear2 = rng.integers(1, 30, size=(33, 33))
    clear2[cls >= frm.gm.OBSTACLE] = 0
    grid = rtm.cells_of(cls, clear2)
    want_fr = frm.frontiers(grid, dict(connectivity=8))[:3]
    assert want_fr[2][1] >= 2    # (several frontiers)
    # two sheets three cells above the map (new: they enter, before and after the growth) and a row that touches it (known: rejected)
    cloud = sm.points_of_cells([(x, y, 3) for x in range(24) for y in range(12) if y != 5] + [(x, 0, 1) for x in range(24)], LEAF)
    reg = rgm.region([-rgm.IMAX] * 3, [11, rgm.IMAX, rgm.IMAX])   # x index <= 11: half of every row
    hr = loamx.DenseMapRegion(reg["lo"], reg["hi"], reg["side"])

    def round_():
        """one round against the models; every word it produced but the two schedule-dependent 'hooks lost' statistics"""
        sel = rgm.select(flm.records_of(m), reg)
        assert 0 < len(sel["keys"]) < len(m)
        got = [d.region_points(hr).tobytes()]
        assert got[-1] == dm.export(sel["keys"], sel["vals"], LEAF).tobytes()
        labels, segs, st = check(d, m, connectivity=6)
        got += [labels.tobytes(), segs.tobytes(), [st[k] for k in sm.STAT_KEYS]]
        lab, out = d.frontiers_cells(grid, connectivity=8)
        fst = d.frontier_stats
        assert out.tobytes() == want_fr[0].tobytes() and lab.tobytes() == want_fr[1].tobytes()
        assert tuple(fst[k] for k in loamx.FRONTIER_STATS[:5]) == want_fr[2]
        got += [lab.tobytes(), out.tobytes(), [fst[k] for k in loamx.FRONTIER_STATS[:5]]]
        cl, cs, cst = d.segment_cloud(cloud, ORIGIN)
        wl, ws, wst, _ = scm.segment_cloud(m, cloud, ORIGIN, None)
        assert cl.tobytes() == wl.tobytes() and cs.tobytes() == ws.tobytes() and {k: cst[k] for k in scm.STAT_KEYS} == wst
        assert (wst["entered"], wst["rejected"], wst["components"]) == (24 * 11, 24, 2)
        got += [cl.tobytes(), cs.tobytes(), [cst[k] for k in scm.STAT_KEYS]]
        got.append(d.points().tobytes())
        assert got[-1] == m.points().tobytes()
        return got

    first = round_()
    assert round_() == first
    more = sweeps_of([(x, y, 1) for x in range(24) for y in range(0, 40, 2)])   # one larger add: the table grows
    feed(d, more), feed(m, more)
    assert d.rehashes >= 1 and d.stats()["slots"] > 1024 and len(d) == len(m) == 299 + 480
    assert round_() != first


# ---- 10: the outputs and the refusals ---------------------------------------------------------------------------------------------------------------
def raw(d, cfg=None, rule=None, n_lab=None, n_seg=None, lab_cap=None, seg_cap=None, null=()):
    """loamx_densemap_segment itself, every output pre-filled with a pattern: (rc, n_voxels, n_segs, stats, labels, segs);
    n_lab / n_seg None: that output is NULL; null: the names of pointer arguments to pass as NULL"""
    L = loamx.lib()
    lab = None if n_lab is None else np.full(max(n_lab, 1), PAT, np.uint32)
    segs = None if n_seg is None else np.frombuffer(bytes([0xa5]) * (72 * max(n_seg, 1)), sm.SEGMENT).copy()
    nv, ns, st = C.c_uint64(PAT), C.c_uint64(PAT), (C.c_uint64 * 6)(*([PAT] * 6))
    rc = L.loamx_densemap_segment(None if "h" in null else d.h, None if cfg is None else C.byref(cfg), None if rule is None else C.byref(rule),
                                  None if lab is None else lab.ctypes.data_as(C.c_void_p), C.c_uint64((n_lab or 0) if lab_cap is None else lab_cap),
                                  None if "n_voxels" in null else C.byref(nv),
                                  None if segs is None else segs.ctypes.data_as(C.c_void_p), C.c_uint64((n_seg or 0) if seg_cap is None else seg_cap),
                                  None if "n_segs" in null else C.byref(ns), None if "stats" in null else st)
    return rc, nv.value, ns.value, list(st), lab, segs


def test_null_outputs_and_capacity(scene):
    d, m = scene["map"], scene["model"]
    cfg = loamx.SegmentConfig(connectivity=6)
    wl, ws, wst = sm.segment(m, connectivity=6)
    rc, nv, ns, st, lab, segs = raw(d, cfg, n_lab=541, n_seg=15)
    assert (rc, nv, ns) == (loamx.OK, 541, 15) and lab.tobytes() == wl.tobytes() and segs.tobytes() == ws.tobytes()
    assert st[:5] == [wst[k] for k in sm.STAT_KEYS]
    rc, nv, ns, st2, lab, segs = raw(d, cfg, n_lab=None, n_seg=15)          # no labels
    assert (rc, nv, ns, st2[:5]) == (loamx.OK, 541, 15, st[:5]) and segs.tobytes() == ws.tobytes()
    rc, nv, ns, st2, lab, segs = raw(d, cfg, n_lab=541, n_seg=None)         # no records
    assert (rc, nv, ns, st2[:5]) == (loamx.OK, 541, 15, st[:5]) and lab.tobytes() == wl.tobytes()
    rc, nv, ns, st2, lab, segs = raw(d, cfg)                                # neither
    assert (rc, nv, ns, st2[:5]) == (loamx.OK, 541, 15, st[:5])
    assert d.segment(connectivity=6, labels=False)[0] is None
    # a capacity one short, for either output: nothing written but the needed counts
    for kw in (dict(lab_cap=540), dict(seg_cap=14), dict(lab_cap=0, seg_cap=0)):
        rc, nv, ns, st2, lab, segs = raw(d, cfg, n_lab=541, n_seg=15, **kw)
        assert (rc, nv, ns) == (loamx.E_CAPACITY, 541, 15)
        assert np.all(lab == PAT) and segs.tobytes() == bytes([0xa5]) * (72 * 15) and st2 == [PAT] * 6
    rc, nv, ns, _, _, _ = raw(d, cfg, n_lab=None, n_seg=None, lab_cap=0, seg_cap=0)   # a NULL output needs no room
    assert rc == loamx.OK


def test_refusals_leave_everything_untouched(scene):
    d = scene["map"]
    plain = feed(new_map(carving=False), scene["sweeps"][:1])
    before = exports(d)
    good = loamx.StaticRule()
    cases = [("h", d, None, None, ("h",)), ("n_voxels", d, None, None, ("n_voxels",)), ("n_segs", d, None, None, ("n_segs",)),
             ("stats", d, None, None, ("stats",)),
             ("which", d, loamx.SegmentConfig(which=3), None, ()),
             ("connectivity", d, loamx.SegmentConfig(connectivity=8), None, ()), ("connectivity", d, loamx.SegmentConfig(connectivity=0), None, ()),
             ("min_points", d, loamx.SegmentConfig(min_points=0), None, ()), ("min_voxels", d, loamx.SegmentConfig(min_voxels=0), None, ()),
             ("lo", d, loamx.SegmentConfig(lo=(1, 0, 0), hi=(0, 0, 0)), None, ()), ("lo", d, loamx.SegmentConfig(lo=(0, 0, 3), hi=(0, 0, 2)), None, ()),
             ("lo", d, loamx.SegmentConfig(lo=(0, -LIM - 1, 0)), None, ()), ("hi", d, loamx.SegmentConfig(hi=(0, 0, LIM + 1)), None, ()),
             ("carving", plain, loamx.SegmentConfig(which=sm.STATIC), None, ()), ("carving", plain, loamx.SegmentConfig(which=sm.DYNAMIC), good, ()),
             ("den", d, loamx.SegmentConfig(which=sm.STATIC), loamx.StaticRule(3, 1, 0), ()),
             ("den", d, loamx.SegmentConfig(which=sm.DYNAMIC), loamx.StaticRule(1, 0, 0), ())]
    L = loamx.lib()
    for word, target, cfg, rule, null in cases:
        rc, nv, ns, st, lab, segs = raw(target, cfg, rule, n_lab=541, n_seg=16, null=null)
        assert rc == loamx.E_INVALID, word
        assert word.encode() in L.loamx_last_error(), (word, L.loamx_last_error())
        assert nv == PAT and ns == PAT and st == [PAT] * 6 and np.all(lab == PAT) and segs.tobytes() == bytes([0xa5]) * (72 * 16), word
    assert exports(d) == before
    check(d, scene["model"], which=sm.STATIC, connectivity=6)        # the handle is as it was
    check(plain, feed(dm.Model(leaf=LEAF), scene["sweeps"][:1]))     # ALL needs no carving
