"""GPU: the objects of a sweep that is not in the map (include/loamx.h, loamx_densemap_segment_cloud and its from_* forms) against
their model (tests/densemap_segment_cloud_model.py, a composition of the models of the map, of carving and of the components).  Leaf
0.5 and points at voxel centres (sm.points_of_cells), so the cells are exact.  Every comparison is of bytes: the labels, the records
and stats[0..11] equal the model's, no tolerance anywhere; beside that the counts worked out by hand are asserted, so that a model and
a kernel that are wrong together still trip."""
import ctypes as C
import time

import numpy as np
import pytest

import densemap_carve_model as cm
import densemap_model as dm
import densemap_raycast_model as rm
import densemap_segment_cloud_model as scm
import densemap_segment_model as sm
from loam_velodyne_amd import loamx, synth
from test_gpu_densemap_segment import EDGE_CELLS, PAIRS

pytestmark = pytest.mark.gpu

LEAF = 0.5
LIM = 2 ** 20 - 1
PAT = 0xa5a5a5a5
ORIGIN = (0.0, 0.0, 0.0)
NONE = sm.NONE


def new_map(initial_slots=1024, carving=False, **kw):
    d = loamx.DenseMap(leaf=LEAF, initial_slots=initial_slots, **kw)
    if carving:
        d.enable_carving()
    return d


def feed(target, points, origin=ORIGIN):
    r = target.add(points, origin)
    assert r == loamx.OK or r is True


def pair_of(cells=(), counts=None, parts=1, initial_slots=1024):
    """(device map, model) holding the cells' points, fed in `parts` adds"""
    d, m = new_map(initial_slots), dm.Model(leaf=LEAF)
    if len(cells):
        for q in np.array_split(sm.points_of_cells(cells, LEAF, counts), parts):
            if len(q):
                feed(d, q), feed(m, q)
    return d, m


def explain(got, want):
    for j, (g, w) in enumerate(zip(got, want)):
        if g.tobytes() != w.tobytes():
            return f"item {j}: got {g}, want {w}"
    return f"lengths {len(got)}, {len(want)}"


def check(d, model, points, origin=ORIGIN, rule=None, **cfg):
    """one device call against the model: the bytes of both outputs and the twelve exact stats; returns the device's triple"""
    labels, segs, st = d.segment_cloud(points, origin, static=None if rule is None else loamx.StaticRule(*rule), **cfg)
    wl, ws, wst, _ = scm.segment_cloud(model, points, origin, rule, **cfg)
    assert labels.dtype == np.uint32 and labels.tobytes() == wl.tobytes(), explain(labels, wl)
    assert segs.dtype == sm.SEGMENT and segs.tobytes() == ws.tobytes(), explain(segs, ws)
    assert {k: st[k] for k in scm.STAT_KEYS} == wst, (st, wst)
    return labels, segs, st


def cloud_of_cells(cells, counts=None):
    return sm.points_of_cells(cells, LEAF, counts)


# ---- 1: counts and thread tails --------------------------------------------------------------------------------------------------------------
def test_empty_cloud_and_empty_map():
    d, m = pair_of([(0, 0, 0)])
    labels, segs, st = check(d, m, np.zeros((0, 4), np.float32))
    assert len(labels) == 0 and len(segs) == 0 and all(v == 0 for v in st.values())
    e, em = pair_of()
    cloud = cloud_of_cells([(0, 0, 0), (1, 0, 0), (5, 5, 5)])
    for which, entered in ((scm.ALL, 3), (scm.NEW, 3), (scm.KNOWN, 0)):   # nothing is near in an empty map
        labels, segs, st = check(e, em, cloud, which=which)
        assert (st["entered"], st["rejected"], st["kept"]) == (entered, 3 - entered, 2 if entered else 0)


def test_one_point():
    d, m = pair_of([(9, 9, 9)])
    labels, segs, st = check(d, m, cloud_of_cells([(-2, 3, -4)]))
    assert labels.tolist() == [0] and segs[0]["min_key"] == cm.key_of((-2, 3, -4)) and (segs[0]["voxels"], segs[0]["points"]) == (1, 1)
    assert check(d, m, cloud_of_cells([(9, 9, 8)]))[0].tolist() == [NONE]
    assert check(d, m, cloud_of_cells([(9, 9, 8)]), which=scm.KNOWN)[0].tolist() == [0]


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_thread_tails(n):
    d, m = pair_of([(0, 0, 0)])
    far = [(3 * k, 10, 0) for k in range(n)]     # n voxels, no two adjacent
    labels, segs, st = check(d, m, cloud_of_cells(far))
    assert (st["voxels"], st["components"], st["labelled"]) == (n, n, n) and labels.tolist() == list(range(n))
    one = cloud_of_cells([(4, 4, 4)], counts=[n])   # the combine within a wave, across waves, across blocks
    labels, segs, st = check(d, m, one)
    assert (st["voxels"], st["entered"], int(segs[0]["points"])) == (1, n, n) and labels.tolist() == [0] * n
    row = cloud_of_cells([(k, 20, 0) for k in range(n)])   # one component of n voxels
    assert check(d, m, row)[2]["largest"] == n


# ---- 2: the margin and the map test -----------------------------------------------------------------------------------------------------------
DIRS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (0, -1, 1), (-1, 0, -1), (1, 1, 1), (-1, -1, -1), (1, -1, 1)]


@pytest.mark.parametrize("margin", [0, 1, 2])
@pytest.mark.parametrize("base", [(0, 0, 0), (-3, -2, -5), (1, -1, 0)])
def test_margin_is_exact(margin, base):
    d, m = pair_of([base])
    for u in DIRS:
        inside = tuple(base[a] + margin * u[a] for a in range(3))
        outside = tuple(base[a] + (margin + 1) * u[a] for a in range(3))
        cloud = cloud_of_cells([inside, outside])
        labels, _, st = check(d, m, cloud, margin=margin)
        assert labels.tolist() == [NONE, 0] and (st["rejected"], st["entered"]) == (1, 1), (u, labels)
        labels, _, st = check(d, m, cloud, margin=margin, which=scm.KNOWN)
        assert labels.tolist() == [0, NONE], (u, labels)
    # all of them in one cloud, so that lanes of one wave leave the probe loop at different places
    cells = [tuple(base[a] + k * u[a] for a in range(3)) for u in DIRS for k in (margin, margin + 1)]
    check(d, m, cloud_of_cells(cells), margin=margin, min_voxels=1, connectivity=6)


@pytest.mark.parametrize("axes", [(0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)])
def test_clipped_neighbourhood(axes):
    for sign in (1, -1):
        corner = tuple(sign * LIM if a in axes else 3 for a in range(3))
        inside = tuple(sign * (LIM - 2) if a in axes else 3 for a in range(3))   # two cells in: the last one margin 2 reaches
        beyond = tuple(sign * (LIM - 3) if a in axes else 3 for a in range(3))
        cloud = cloud_of_cells([corner])
        e, em = pair_of([(0, 0, 0)])
        assert check(e, em, cloud, margin=2)[0].tolist() == [0]                    # nothing near, and nothing faults
        d, m = pair_of([inside])
        assert check(d, m, cloud, margin=2)[0].tolist() == [NONE] and check(d, m, cloud, margin=1)[0].tolist() == [0]
        d, m = pair_of([beyond])
        assert check(d, m, cloud, margin=2)[0].tolist() == [0]
        # a voxel at the far end of the key range is no neighbour: the packed keys wrap, the indices do not
        wrapped = tuple(-sign * LIM if a in axes else 3 for a in range(3))
        d, m = pair_of([wrapped])
        assert check(d, m, cloud, margin=2)[0].tolist() == [0]


@pytest.mark.parametrize("k", [1, 2, 5])
def test_map_min_points(k):
    cells, counts = [(0, 0, 0), (10, 0, 0)], [max(k - 1, 1), k]
    d, m = pair_of(cells, counts)
    cloud = cloud_of_cells([(0, 0, 1), (10, 0, 1)])
    labels, _, st = check(d, m, cloud, map_min_points=k)
    assert labels.tolist() == ([NONE, NONE] if k == 1 else [0, NONE])      # n = k - 1 is not mapped, n = k is
    assert check(d, m, cloud, map_min_points=k + 1)[0].tolist() == [0, 1]


@pytest.fixture(scope="module")
def carved():
    S = rm.box_cast_scene()
    m, d = cm.CarveModel(leaf=LEAF), new_map(carving=True)
    for p, o in S["sweeps"]:
        feed(m, p, o), feed(d, p, o)
    assert len(m) == len(d) == 541 and int(m.dynamic_mask().sum()) == 23
    return dict(map=d, model=m, sweeps=S["sweeps"])


def test_rule_unmaps_dynamic_voxels(carved):
    d, m = carved["map"], carved["model"]
    dyn = m.dynamic_mask()
    cells = [sm.cell_of(k) for k in m.keys.tolist()]
    cloud = cloud_of_cells(cells)     # one point in every voxel of the map
    labels, _, st = check(d, m, cloud, rule=cm.DEFAULT_RULE, margin=0)
    assert st["entered"] == 23 and np.array_equal(labels != NONE, dyn)      # under the rule the dynamic voxels are not mapped
    labels, _, st = check(d, m, cloud, rule=None, margin=0)
    assert st["entered"] == 0 and st["rejected"] == 541                       # without it every voxel is
    other = (40, 1, 1)
    assert check(d, m, cloud, rule=other, margin=0)[2]["entered"] == int(m.dynamic_mask(other).sum()) == 19
    check(d, m, cloud, rule=cm.DEFAULT_RULE, margin=1, which=scm.KNOWN)
    check(d, m, cloud, rule=cm.DEFAULT_RULE, margin=2, map_min_points=2)


# ---- 3: admission ------------------------------------------------------------------------------------------------------------------------------
def test_admission():
    o = (1.25, -0.75, 2.25)
    kw = dict(min_range=1.0, max_range=6.0)
    d, m = new_map(**kw), dm.Model(leaf=LEAF, **kw)
    base = cloud_of_cells([(20, 0, 0)])
    feed(d, base, (10.0, 0.0, 0.0)), feed(m, base, (10.0, 0.0, 0.0))
    p = np.zeros((14, 4), np.float32)
    p[:, :3] = np.asarray(o, np.float32) + 3.0                # admitted unless changed below
    p[0, 0], p[1, 1], p[2, 2] = np.nan, np.inf, -np.inf
    p[3, :3] = (524288.25, o[1], o[2])                        # cell 2^20: beyond max_range first
    p[4, :3] = np.asarray(o, np.float32) + 0.25               # inside min_range
    p[5, :3] = (o[0] + 6.25, o[1], o[2])                      # beyond max_range
    p[6, :3] = (o[0] + 6.0, o[1], o[2])                       # on it: admitted
    p[7, :3] = (o[0], o[1] - 1.0, o[2])                       # on min_range: admitted
    p[8, :3] = (o[0], o[1], o[2])                             # the origin itself
    labels, segs, st = check(d, m, p, o, which=scm.ALL)
    assert labels[:6].tolist() == [NONE] * 6 and np.all(labels[6:8] != NONE) and labels[8] == NONE
    fresh = new_map(**kw)
    feed(fresh, p, o)
    fs = fresh.stats()
    assert (st["dropped_range"], st["dropped_key"], st["entered"]) == (fs["dropped_range"], fs["dropped_key"], fs["added"])
    # without a range filter the same cloud meets the key rule
    d0, m0 = pair_of([(20, 0, 0)])
    labels, segs, st = check(d0, m0, p, o, which=scm.ALL)
    f0 = new_map()
    feed(f0, p, o)
    assert (st["dropped_range"], st["dropped_key"]) == (f0.stats()["dropped_range"], f0.stats()["dropped_key"]) and st["dropped_key"] >= 3
    edge = np.zeros((4, 4), np.float32)
    edge[:, :3] = [(524288.0, 0.25, 0.25), (0.25, -524288.25, 0.25), (524287.75, 0.25, 0.25), (0.25, 0.25, -524287.25)]
    labels, _, st = check(d0, m0, edge, which=scm.NEW, margin=2)
    assert labels.tolist() == [NONE, NONE, 1, 0]      # cells (LIM, 0, 0) and (0, 0, -LIM): the second has the smaller key
    assert st["dropped_key"] == 2


# ---- 4: clustering -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [6, 18, 26])
def test_pairs_and_edges_as_clouds(conn):
    d, m = pair_of([(100, 100, 100)])
    for name, (a, d_, dist) in PAIRS.items():
        b = tuple(a[k] + d_[k] for k in range(3))
        labels, segs, st = check(d, m, cloud_of_cells([a, b]), connectivity=conn)
        joined = dist <= {6: 1, 18: 2, 26: 3}[conn]
        assert st["components"] == (1 if joined else 2) and sorted(labels.tolist()) == ([0, 0] if joined else [0, 1]), name
    labels, segs, st = check(d, m, cloud_of_cells(EDGE_CELLS), connectivity=conn)
    assert st["components"] == {6: 10, 18: 9, 26: 8}[conn]
    check(d, m, cloud_of_cells(EDGE_CELLS), connectivity=conn, which=scm.ALL, margin=2)


def test_window_min_points_min_voxels():
    d, m = pair_of([(0, 30, 0)])
    u = [(x, 0, 0) for x in range(-4, 5)] + [(-4, y, 0) for y in range(1, 4)] + [(4, y, 0) for y in range(1, 4)]   # a U
    cloud = cloud_of_cells(u)
    assert check(d, m, cloud)[2]["components"] == 1
    labels, segs, st = check(d, m, cloud, lo=(-LIM, 1, -LIM), hi=(LIM, LIM, LIM))   # without the bottom bar: the two uprights
    assert (st["selected"], st["components"], st["labelled"]) == (6, 2, 6) and int((labels == NONE).sum()) == 9
    labels, segs, st = check(d, m, cloud, lo=(-3, 0, 0), hi=(3, 0, 0))                # the bar's middle alone
    assert (st["selected"], st["components"]) == (7, 1) and segs[0]["lo"].tolist() == [-3, 0, 0]
    bar = [(x, 5, 5) for x in range(9)]
    cloud = cloud_of_cells(bar + [(20, 5, 5)], counts=[2, 2, 2, 2, 1, 2, 2, 2, 3, 2])
    labels, segs, st = check(d, m, cloud, min_points=2)     # the bar cut in two; the points of the dropped voxel get NONE
    assert (st["voxels"], st["selected"], st["components"], st["labelled"]) == (10, 9, 3, 19) and segs["points"].tolist() == [8, 9, 2]
    labels, segs, st = check(d, m, cloud, min_points=2, min_voxels=2)
    assert (st["kept"], st["kept_voxels"], st["labelled"], st["largest"]) == (2, 8, 17, 4) and labels[-2:].tolist() == [NONE, NONE]
    assert check(d, m, cloud, min_voxels=11)[2]["labelled"] == 0


# ---- 5: a box scene: floor and walls in the map, a sweep that adds three boxes ------------------------------------------------------------------
def room():
    floor = [(x, -4, z) for x in range(-12, 13) for z in range(-12, 13)]
    walls = [(x, y, z) for y in range(-3, 5) for x in range(-12, 13) for z in range(-12, 13) if abs(x) == 12 or abs(z) == 12]
    boxes = [[(x, y, z) for x in range(-6, -3) for y in range(-3, 0) for z in range(2, 5)],        # stands on the floor
             [(x, y, z) for x in range(9, 12) for y in range(-1, 2) for z in range(-2, 1)],         # touches the wall at x = 12
             [(x, y, z) for x in range(2, 5) for y in range(1, 3) for z in range(-8, -6)]]          # hangs in the air
    return floor, walls, boxes


def scene_map_points():
    floor, walls, _ = room()
    return sm.points_of_cells(floor + walls, LEAF, np.random.default_rng(8).integers(1, 4, len(floor) + len(walls)))


@pytest.fixture(scope="module")
def scene():
    floor, walls, boxes = room()
    rng = np.random.default_rng(9)
    d, m = new_map(), dm.Model(leaf=LEAF)
    for q in np.array_split(scene_map_points(), 3):
        feed(d, q), feed(m, q)
    assert d.rehashes >= 1 and len(d) == len(m) == len(floor) + len(walls)
    cells = floor + walls + [c for b in boxes for c in b]
    cloud = cloud_of_cells(cells, rng.integers(10, 18, len(cells)))
    cloud = cloud[rng.permutation(len(cloud))]
    assert 15000 < len(cloud) < 25000
    return dict(map=d, model=m, cloud=cloud, boxes=boxes)


def test_equivalence_on_the_device(scene):
    d, m, cloud = scene["map"], scene["model"], scene["cloud"]
    labels, segs, st = check(d, m, cloud, which=scm.ALL)
    assert st["entered"] == len(cloud) and st["components"] == 2       # the room with two of the boxes, and the one in the air
    fresh = new_map()
    feed(fresh, cloud[labels != NONE])
    fl, fsegs, fst = fresh.segment()
    assert fsegs.tobytes() == segs.tobytes() and fst["components"] == st["components"] and fst["selected"] == st["voxels"]
    # NEW, margin 1: the three boxes, less the layers beside the floor and the wall
    labels, segs, st = check(d, m, cloud)
    assert (st["components"], st["kept"]) == (3, 3) and sorted(segs["voxels"].tolist()) == [3 * 2 * 2, 3 * 2 * 3, 2 * 3 * 3]
    fresh = new_map()
    feed(fresh, cloud[labels != NONE])
    assert fresh.segment()[1].tobytes() == segs.tobytes()
    assert check(d, m, cloud, margin=0)[2]["components"] == 3 and check(d, m, cloud, margin=2)[2]["components"] == 3
    check(d, m, cloud, which=scm.KNOWN)
    check(d, m, cloud, which=scm.KNOWN, connectivity=6, min_points=7, min_voxels=2)


def test_invariance(scene):
    m, cloud = scene["model"], scene["cloud"]
    want = scm.segment_cloud(m, cloud)
    perm = np.random.default_rng(1).permutation(len(cloud))
    maps = {"1024": scene["map"]}
    for name, slots, parts in (("65536", 1 << 16, 1), ("seven", 1024, 7)):    # the same map points: another table, other adds
        maps[name] = new_map(slots)
        for q in np.array_split(scene_map_points()[::-1], parts):
            feed(maps[name], q)
    assert maps["65536"].stats()["slots"] == 1 << 16 and maps["65536"].rehashes == 0 and maps["1024"].stats()["slots"] != 1 << 16
    assert maps["65536"].points().tobytes() == maps["1024"].points().tobytes() == maps["seven"].points().tobytes()
    for name, d in maps.items():
        labels, segs, st = check(d, m, cloud)
        assert labels.tobytes() == want[0].tobytes() and segs.tobytes() == want[1].tobytes(), name
        pl, ps, pst = check(d, m, cloud[perm])
        assert pl.tobytes() == labels[perm].tobytes() and ps.tobytes() == segs.tobytes()
        assert {k: pst[k] for k in scm.STAT_KEYS} == {k: st[k] for k in scm.STAT_KEYS}


# ---- 6: buffers ----------------------------------------------------------------------------------------------------------------------------------
def test_scratch_table_grows_and_is_cleared(scene):
    d, m = scene["map"], scene["model"]
    rng = np.random.default_rng(4)

    def cloud(n):
        cells = rng.integers(-11, 12, (n, 3))
        return cloud_of_cells(cells)

    before = d.segment(connectivity=6)
    small, big, again = cloud(300), cloud(5000), cloud(300)
    for c in (small, big, again, small):
        check(d, m, c, margin=0)
        check(d, m, c, which=scm.ALL, connectivity=6)
    after = d.segment(connectivity=6)     # the two share DmSegment
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    want = sm.segment(m, connectivity=6)
    assert after[0].tobytes() == want[0].tobytes() and after[1].tobytes() == want[1].tobytes()
    check(d, m, small)


# ---- 7: the outputs, the refusals, and the map untouched -------------------------------------------------------------------------------------------
def raw(d, cloud, origin=ORIGIN, cfg=None, rule=None, n_lab=None, n_seg=None, lab_cap=None, seg_cap=None, null=(), fn=None, head=None):
    """loamx_densemap_segment_cloud itself (or a from_* form: fn, head), every output pre-filled with a pattern:
    (rc, n_points, n_segs, stats, labels, segs); n_lab / n_seg None: that output is NULL; null: pointer arguments to pass as NULL"""
    L = loamx.lib()
    lab = None if n_lab is None else np.full(max(n_lab, 1), PAT, np.uint32)
    segs = None if n_seg is None else np.frombuffer(bytes([0xa5]) * (72 * max(n_seg, 1)), sm.SEGMENT).copy()
    nv, ns, st = C.c_uint64(PAT), C.c_uint64(PAT), (C.c_uint64 * 13)(*([PAT] * 13))
    if head is None:
        a = loamx.as_points(cloud)
        cl, o = loamx.cloud_of(a), np.ascontiguousarray(origin, np.float32)
        head = (None if "points" in null else C.byref(cl), None if "origin" in null else o.ctypes.data_as(C.c_void_p))
        fn = L.loamx_densemap_segment_cloud
    rc = fn(None if "h" in null else d.h, *head, None if cfg is None else C.byref(cfg), None if rule is None else C.byref(rule),
            None if lab is None else lab.ctypes.data_as(C.c_void_p), C.c_uint64((n_lab or 0) if lab_cap is None else lab_cap),
            None if "n_points" in null else C.byref(nv),
            None if segs is None else segs.ctypes.data_as(C.c_void_p), C.c_uint64((n_seg or 0) if seg_cap is None else seg_cap),
            None if "n_segs" in null else C.byref(ns), None if "stats" in null else st)
    return rc, nv.value, ns.value, list(st), lab, segs


def exports(d, tmp_path):
    path = str(tmp_path / "m.lxdm")
    d.save(path)
    return open(path, "rb").read(), d.stats()


def test_null_outputs_and_capacity(scene):
    d, m, cloud = scene["map"], scene["model"], scene["cloud"][:3000]
    cfg = loamx.SegmentCloudConfig(margin=0, connectivity=6)
    wl, ws, wst, _ = scm.segment_cloud(m, cloud, margin=0, connectivity=6)
    n, k = len(cloud), len(ws)
    assert k >= 3
    rc, nv, ns, st, lab, segs = raw(d, cloud, cfg=cfg, n_lab=n, n_seg=k)
    assert (rc, nv, ns) == (loamx.OK, n, k) and lab.tobytes() == wl.tobytes() and segs.tobytes() == ws.tobytes()
    assert st[:12] == [wst[key] for key in scm.STAT_KEYS]
    rc, nv, ns, st2, lab, segs = raw(d, cloud, cfg=cfg, n_lab=None, n_seg=k)          # no labels
    assert (rc, nv, ns, st2[:12]) == (loamx.OK, n, k, st[:12]) and segs.tobytes() == ws.tobytes()
    rc, nv, ns, st2, lab, segs = raw(d, cloud, cfg=cfg, n_lab=n, n_seg=None)          # no records
    assert (rc, nv, ns, st2[:12]) == (loamx.OK, n, k, st[:12]) and lab.tobytes() == wl.tobytes()
    rc, nv, ns, st2, lab, segs = raw(d, cloud, cfg=cfg)                               # neither
    assert (rc, nv, ns, st2[:12]) == (loamx.OK, n, k, st[:12])
    assert d.segment_cloud(cloud, margin=0, labels=False)[0] is None
    for kw in (dict(lab_cap=n - 1), dict(seg_cap=k - 1), dict(lab_cap=0, seg_cap=0)):  # one short: only the two counts are written
        rc, nv, ns, st2, lab, segs = raw(d, cloud, cfg=cfg, n_lab=n, n_seg=k, **kw)
        assert (rc, nv, ns) == (loamx.E_CAPACITY, n, k)
        assert np.all(lab == PAT) and segs.tobytes() == bytes([0xa5]) * (72 * k) and st2 == [PAT] * 13
    assert raw(d, cloud, cfg=cfg, n_lab=None, n_seg=None, lab_cap=0, seg_cap=0)[0] == loamx.OK   # a NULL output needs no room
    rc, nv, ns, st2, lab, segs = raw(d, cloud, cfg=None, n_lab=n, n_seg=4096)         # cfg NULL: the defaults
    wl, ws, wst, _ = scm.segment_cloud(m, cloud)
    assert rc == loamx.OK and lab.tobytes() == wl.tobytes() and segs[:ns].tobytes() == ws.tobytes()


def test_refusals_and_the_map_is_untouched(scene, carved, tmp_path):
    d, cloud = scene["map"], scene["cloud"][:500]
    cd = carved["map"]
    before, cbefore = exports(d, tmp_path), exports(cd, tmp_path)
    good, K = loamx.StaticRule(), loamx.SegmentCloudConfig
    cases = [("h is NULL", d, None, None, ("h",)), ("points is NULL", d, None, None, ("points",)), ("origin is NULL", d, None, None, ("origin",)),
             ("n_points is NULL", d, None, None, ("n_points",)), ("n_segs is NULL", d, None, None, ("n_segs",)),
             ("stats is NULL", d, None, None, ("stats",)),
             ("which", d, K(which=3), None, ()), ("margin", d, K(margin=3), None, ()), ("map_min_points", d, K(map_min_points=0), None, ()),
             ("connectivity", d, K(connectivity=7), None, ()), ("min_points", d, K(min_points=0), None, ()),
             ("min_voxels", d, K(min_voxels=0), None, ()), ("lo", d, K(lo=(1, 0, 0), hi=(0, 0, 0)), None, ()),
             ("lo", d, K(lo=(0, -LIM - 1, 0)), None, ()), ("hi", d, K(hi=(0, 0, LIM + 1)), None, ()),
             ("den", cd, None, loamx.StaticRule(3, 1, 0), ()), ("carving", d, None, good, ())]
    L = loamx.lib()
    for word, target, cfg, rule, null in cases:
        rc, nv, ns, st, lab, segs = raw(target, cloud, cfg=cfg, rule=rule, n_lab=500, n_seg=16, null=null)
        assert rc == loamx.E_INVALID, word
        assert word.encode() in L.loamx_last_error(), (word, L.loamx_last_error())
        assert nv == PAT and ns == PAT and st == [PAT] * 13 and np.all(lab == PAT) and segs.tobytes() == bytes([0xa5]) * (72 * 16), word
    nv, st = C.c_uint64(PAT), (C.c_uint64 * 13)()
    assert L.loamx_densemap_segment_cloud_from_map(d.h, None, None, None, None, C.c_uint64(0), C.byref(nv), None, C.c_uint64(0), C.byref(nv),
                                                   st) == loamx.E_INVALID and b"m is NULL" in L.loamx_last_error()
    assert L.loamx_densemap_segment_cloud_from_pipeline(d.h, None, C.c_uint32(0), None, None, None, C.c_uint64(0), C.byref(nv), None, C.c_uint64(0),
                                                        C.byref(nv), st) == loamx.E_INVALID and b"p is NULL" in L.loamx_last_error()
    assert nv.value == PAT
    with pytest.raises(loamx.LoamxError) as e:
        d.segment_cloud(cloud, margin=3)
    assert e.value.code == loamx.E_INVALID and "margin" in str(e.value)
    # every kind of call, refused ones included, and the map's bytes and counters are what they were
    for which in (scm.ALL, scm.NEW, scm.KNOWN):    # (any `which` works without carving when there is no rule)
        check(d, scene["model"], cloud, which=which, margin=2)
        d.segment_cloud(cloud, which=which, labels=False)
        check(cd, carved["model"], cloud, which=which, rule=cm.DEFAULT_RULE)
    assert raw(d, cloud, n_lab=499, n_seg=16)[0] == loamx.E_CAPACITY
    assert exports(d, tmp_path) == before and exports(cd, tmp_path) == cbefore


# ---- 8: the registered cloud of a mapper and of a pipeline, where it lies ---------------------------------------------------------------------------
def _same_as_host(dev, host):
    return dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes() and dev[2] == host[2]


def _strip(st):
    return {k: st[k] for k in scm.STAT_KEYS}


def test_segment_cloud_from_map():
    w = synth.World(half_extent=65.0)
    cmap, smap = w.make_map(60_000)
    poses = synth.trajectory(2)
    sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
    mp.load_cubes(cmap, smap)
    d = loamx.DenseMap(leaf=LEAF, initial_slots=1 << 14)
    rc, labels, segs, st = d.segment_cloud_from(mp)
    assert rc == loamx.SKIPPED and len(labels) == 0 and len(segs) == 0 and not any(st.values())   # the mapper has not processed a sweep
    for t in range(2):
        sw = synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=900 + t, az_steps=900)
        f = sr.process(sw.points.copy(), sw.ring_sizes)
        od.process(f)
        lc, ls = od.last_clouds()
        full = od.transform_to_end(f["full"])
        mp.update_odometry(od.transform_sum)
        _, reg = mp.process(lc, ls, full)
        origin = mp.transform("aft")[3:]
        for cfg in (dict(which=scm.ALL), dict(), dict(which=scm.KNOWN, margin=2, min_voxels=2)):
            rc, labels, segs, st = d.segment_cloud_from(mp, capacity=64, **cfg)    # (too little room at first: the binding asks again)
            hl, hs, hst = d.segment_cloud(reg, origin, **cfg)
            assert rc == loamx.OK and len(labels) == len(reg) > 10000
            assert labels.tobytes() == hl.tobytes() and segs.tobytes() == hs.tobytes() and _strip(st) == _strip(hst)
        assert d.segment_cloud_from(mp, labels=False)[1] is None
        if t == 0:
            assert d.segment_cloud_from(mp)[3]["rejected"] == 0     # an empty map: nothing is near
            assert d.add_from(mp) == loamx.OK                         # the first sweep is the map; the second is tested against it
            assert d.segment_cloud_from(mp)[3]["entered"] == 0      # every point lies in a voxel that holds it
        else:
            st = d.segment_cloud_from(mp)[3]
            assert st["rejected"] > 0 and st["entered"] > 0
    print({k: st[k] for k in loamx.SEGMENT_CLOUD_STATS})


def test_segment_cloud_from_pipeline():
    ns, T = 2, 3
    w = synth.World(half_extent=45.0)
    cmap, smap = w.make_map(60_000)
    sweeps, starts = [[None] * ns for _ in range(T)], []
    for s in range(ns):
        poses = synth.trajectory(T, start=(1.5 * s, 0.0, 2.0 * s))
        starts.append(np.array([0, 0, 0, 1.5 * s, 0, 2.0 * s], np.float32))
        for t in range(T):
            sw = synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=30 * s + t, az_steps=900)
            sweeps[t][s] = (np.ascontiguousarray(sw.points, np.float32), sw.ring_sizes)
    p = loamx.Pipeline(ns)
    p.set_frozen(cmap, smap)
    for s in range(ns):
        p.set_state(s, aft=starts[s])
    p.upload(sweeps)
    dense = [loamx.DenseMap(leaf=LEAF, initial_slots=1 << 14) for _ in range(ns)]
    assert dense[0].segment_cloud_from_pipeline(p, 0)[0] == loamx.SKIPPED     # before any step
    registered = 0
    for t in range(T):
        if p.step(t) != loamx.OK:
            continue
        registered += 1
        for k, d in enumerate(dense):
            reg, origin = p.download_full_res(k, len(sweeps[t][k][0])), p.get(k)[2][3:]
            for cfg in (dict(), dict(which=scm.ALL, connectivity=6)):
                rc, labels, segs, st = d.segment_cloud_from_pipeline(p, k, capacity=128, **cfg)
                hl, hs, hst = d.segment_cloud(reg, origin, **cfg)
                assert rc == loamx.OK and len(labels) == len(reg)
                assert labels.tobytes() == hl.tobytes() and segs.tobytes() == hs.tobytes() and _strip(st) == _strip(hst)
            assert d.add_from_pipeline(p, k) == loamx.OK
    assert registered >= 1
    with pytest.raises(loamx.LoamxError):
        dense[0].segment_cloud_from_pipeline(p, ns)     # a slot beyond the registered streams


# ---- 9: measured, not gated ------------------------------------------------------------------------------------------------------------------------
def terrain(side=1000, leaf=0.125, pillars=2000):
    """the synthetic terrain of scripts/bench_densemap_segment.py: side x side ground voxels, two points each, and pillars on it"""
    rng = np.random.default_rng(1)
    ix, iz = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    height = np.floor(3.0 * np.sin(ix / 40.0) + 2.0 * np.cos(iz / 55.0)).astype(np.int64)
    px, pz = rng.integers(0, side, pillars), rng.integers(0, side, pillars)
    cols = [np.stack([ix.ravel(), height.ravel(), iz.ravel()], axis=1)]
    for k in range(1, 11):
        cols.append(np.stack([px, height[px, pz] + k, pz], axis=1))
    vox = np.concatenate(cols)
    pts = np.zeros((2 * len(vox), 4), np.float32)
    pts[:, :3] = (np.repeat(vox, 2, axis=0) + rng.uniform(0.1, 0.9, (2 * len(vox), 3))) * leaf
    return pts, height


def terrain_and_sweep(leaf=0.125, side=1000):
    """(leaf, the terrain's points, the sweep (131072, 4), its origin): one HDL-64E sweep of the synthetic hall moved to the middle of
    the terrain, the hall's floor one metre up, its ground returns laid on the terrain's own surface"""
    pts, height = terrain(side, leaf)
    w = synth.World(half_extent=60.0)
    poses = synth.trajectory(1)
    sw = synth.make_sweep(w, "HDL-64E", poses[0], poses[1], seed=5)
    cloud = np.ascontiguousarray(sw.points[:, :4], np.float32).copy()
    assert len(cloud) == 131072
    centre = 0.5 * side * leaf
    ground = cloud[:, 1] < w.ground_y + 0.1
    cloud[:, 0] += centre
    cloud[:, 2] += centre
    cloud[:, 1] += 1.0 - w.ground_y
    ci = np.clip(np.floor(cloud[:, [0, 2]] / leaf).astype(np.int64), 0, side - 1)
    cloud[ground, 1] = (height[ci[ground, 0], ci[ground, 1]] + 0.5) * leaf
    return leaf, pts, cloud, (centre, 1.0 - w.ground_y, centre)


def _wall(fn, reps=30, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return "%.2f [%.2f, %.2f] ms" % (np.median(t), min(t), max(t))


def test_measured_on_a_sweep_against_the_terrain():
    """Measured on an MI355X: the figures this prints are recorded in CHANGELOG.md; asserted is only the byte equality with the model
    on a 4,096-point sub-sample of the sweep.  One HDL-64E sweep of the synthetic hall (131,072 points), moved to the middle of the
    million-voxel terrain, its ground returns laid on the terrain's own surface: the ground is known, the hall's pillars, walls and
    ceiling are new.  NEW, margin 1."""
    leaf, pts, cloud, origin = terrain_and_sweep()
    d = loamx.DenseMap(leaf=leaf, initial_slots=1 << 22)
    for k in range(0, len(pts), 1 << 21):
        feed(d, pts[k:k + (1 << 21)])
    # the assertion: a sub-sample against the model
    m = dm.Model(leaf=leaf)
    m.add(pts, ORIGIN)
    sub = cloud[np.random.default_rng(2).choice(len(cloud), 4096, replace=False)]
    labels, segs, st = d.segment_cloud(sub, origin)
    wl, ws, wst, _ = scm.segment_cloud(m, sub, origin)
    assert labels.tobytes() == wl.tobytes() and segs.tobytes() == ws.tobytes() and {k: st[k] for k in scm.STAT_KEYS} == wst
    # the figures
    labels, segs, st = d.segment_cloud(cloud, origin)
    print("segment_cloud, 131072 points against %d voxels, NEW margin 1: %s" % (len(d), st))
    L = loamx.lib()
    a = loamx.as_points(cloud)
    cl, o = loamx.cloud_of(a), np.ascontiguousarray(origin, np.float32)
    lab = np.zeros(len(cloud), np.uint32)
    nv, ns, s13 = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 13)()
    for margin in (1, 2):
        cfg = loamx.SegmentCloudConfig(margin=margin)
        rec = np.zeros(1 << 16, sm.SEGMENT)

        def call(with_labels):
            rc = L.loamx_densemap_segment_cloud(d.h, C.byref(cl), o.ctypes.data_as(C.c_void_p), C.byref(cfg), None,
                                                lab.ctypes.data_as(C.c_void_p) if with_labels else None, C.c_uint64(len(lab)), C.byref(nv),
                                                rec.ctypes.data_as(C.c_void_p), C.c_uint64(len(rec)), C.byref(ns), s13)
            assert rc == loamx.OK
        print("  margin %d: with labels %s, without %s (wall, blocking call); entered %d, components %d" %
              (margin, _wall(lambda: call(True)), _wall(lambda: call(False)), s13[4], s13[7]))
    # the route a host had before: the ray cast's records down, the chosen points into a fresh handle, segment with labels there
    # (the selection on the host between the two is not timed)
    t_cast = _wall(lambda: d.raycast(cloud, origin))
    chosen = cloud[labels != NONE]
    fresh = loamx.DenseMap(leaf=leaf, initial_slots=1 << 18)

    def before():
        fresh.reset()
        fresh.add(chosen, origin)
        fresh.segment(labels=True)
    print("  before: raycast with records %s; add of the %d chosen points to a fresh handle + segment(labels=True) %s (the host's "
          "selection between them not timed)" % (t_cast, len(chosen), _wall(before)))
