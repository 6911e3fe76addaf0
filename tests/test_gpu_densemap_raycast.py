"""GPU: the dense map's ray casts (include/loamx.h, loamx_densemap_raycast and what precedes it) against their model
(tests/densemap_raycast_model.py over the models of the map and of carving).  Leaf 0.5, initial_slots 1024, the box scene of
tests/densemap_align_model.py with 12 mid-air points behind each sweep, carving on: 541 voxels (the table grows), 23 of them dynamic
under the default rule.  Every compared quantity is an integer or the bits of a float: all ten fields of every record and all five
counts equal the model's, and x, y, z of a hit are the bytes of the download record of its key.  No tolerance anywhere."""
import copy
import ctypes as C

import numpy as np
import pytest

import densemap_carve_model as cm
import densemap_raycast_model as rm
from loam_velodyne_amd import loamx, synth

pytestmark = pytest.mark.gpu

LEAF = 0.5
NS = [0, 1, 63, 64, 65, 257, 5000]
CONFIGS = {"plain": dict(), "rule": dict(rule=cm.DEFAULT_RULE), "min5": dict(min_points=5)}


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


def device_cast(d, ends, origin, rule=None, **kw):
    return d.raycast(ends, origin, static=None if rule is None else loamx.StaticRule(*rule), **kw)


def exports(d):
    st = d.stats()
    st.pop("slots")
    return dict(stats=st, points=d.points().tobytes(), misses=d.misses().tobytes(), carve_stats=d.carve_stats())


def explain(got, want):
    """the first record that differs, field by field (for the assertion message)"""
    for i in range(min(len(got), len(want))):
        if got[i].tobytes() != want[i].tobytes():
            return f"ray {i}: got {got[i]}, want {want[i]}"
    return f"lengths {len(got)}, {len(want)}"


@pytest.fixture(scope="module")
def scene():
    S = rm.box_cast_scene()
    S["model"] = feed(cm.CarveModel(leaf=LEAF), S["sweeps"])
    S["map"] = feed(new_map(), S["sweeps"])
    assert len(S["model"]) == len(S["map"]) == 541 and int(S["model"].dynamic_mask().sum()) == 23
    assert S["map"].rehashes >= 1 and S["map"].stats()["slots"] > 1024
    S["download"] = S["map"].points()
    assert S["download"].tobytes() == S["model"].points().tobytes() and S["map"].misses().tobytes() == S["model"].misses().tobytes()
    S["rays"], S["want"] = {}, {}
    return S


def rays_of(S, n):
    if n not in S["rays"]:
        ends = rm.box_rays(n, S["origin"], LEAF)
        S["rays"][n] = (ends, rm.walks_of(ends, S["origin"], LEAF))
    return S["rays"][n]


def want_of(S, n, model=None, tag="scene", **kw):
    """the model's (records, counts) of the n-ray case, computed once per setting"""
    key = (n, tag, tuple(sorted(kw.items())))
    if key not in S["want"]:
        ends, walks = rays_of(S, n)
        S["want"][key] = rm.cast(S["model"] if model is None else model, ends, S["origin"], walks=walks, **kw)
    return S["want"][key]


def check(got, want):
    (rec, counts), (wrec, wcounts) = got, want
    assert rec.dtype == rm.RAY_DTYPE and rm.same_records(rec, wrec), explain(rec, wrec)
    assert counts == wcounts


# ---- 1, 2: exactness against the model, and the coverage that makes it mean something ----------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("n", NS)
def test_cast_equals_the_model(scene, n, cfg):
    kw = CONFIGS[cfg]
    ends, _ = rays_of(scene, n)
    want = want_of(scene, n, **kw)
    got = device_cast(scene["map"], ends, scene["origin"], **kw)
    print(n, cfg, got[1])
    check(got, want)
    rec, counts = got
    assert len(rec) == n and sum(counts[k] for k in rm.COUNT_KEYS[:4]) == n
    # x, y, z of every hit are the bytes of the download record of its key
    hit = rec["status"] >= rm.HIT
    row = np.searchsorted(scene["model"].keys, rec["key"][hit])
    assert np.array_equal(scene["model"].keys[row], rec["key"][hit])
    xyz = np.stack([rec["x"][hit], rec["y"][hit], rec["z"][hit]], axis=1) if hit.any() else np.zeros((0, 3), np.float32)
    assert xyz.tobytes() == np.ascontiguousarray(scene["download"][row, :3]).tobytes()
    assert np.array_equal(rec["n"][hit], scene["download"][row, 3].astype(np.uint32))
    assert not rec["key"][~hit].any() and not rec["range"][~hit].any()
    if n >= 63:
        assert min(counts["miss"], counts["hit"], counts["hit_end"]) >= 3, counts
        assert counts["not_traced"] == 4    # the NaN end, the two ends outside the key range, the ray of two million steps
        if cfg == "rule":
            assert not rm.same_records(rec, want_of(scene, n)[0])    # the rule changes at least one record


# ---- 3: counts only, and the capacity ---------------------------------------------------------------------------------------------
def test_counts_only_and_capacity(scene):
    d = scene["map"]
    for n in (65, 5000):
        ends, _ = rays_of(scene, n)
        for kw in CONFIGS.values():
            none, counts = device_cast(d, ends, scene["origin"], records=False, **kw)
            assert none is None and counts == want_of(scene, n, **kw)[1]
    ends, _ = rays_of(scene, 65)
    before = exports(d)
    buf = np.full(65, 0xAB, np.uint8).repeat(40).view(rm.RAY_DTYPE)
    cl, o, counts = loamx.cloud_of(ends), np.asarray(scene["origin"], np.float32), np.full(5, 77, np.uint64)
    rc = loamx.lib().loamx_densemap_raycast(d.h, C.byref(cl), o.ctypes.data_as(C.c_void_p), None, None, buf.ctypes.data_as(C.c_void_p),
                                            C.c_uint64(64), counts.ctypes.data_as(C.c_void_p))
    assert rc == loamx.E_CAPACITY and b"capacity" in loamx.lib().loamx_last_error()
    assert buf.tobytes() == bytes([0xAB]) * (65 * 40) and counts.tolist() == [77] * 5    # nothing written
    assert exports(d) == before
    # room for exactly the cloud's count is enough, and the records beyond it stay untouched
    rc = loamx.lib().loamx_densemap_raycast(d.h, C.byref(cl), o.ctypes.data_as(C.c_void_p), None, None, buf.ctypes.data_as(C.c_void_p),
                                            C.c_uint64(65), counts.ctypes.data_as(C.c_void_p))
    assert rc == loamx.OK and rm.same_records(buf, want_of(scene, 65)[0])


# ---- 4: independence of the table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["wide", "shuffled", "loaded", "pruned"])
def test_results_do_not_depend_on_the_table(scene, tmp_path, how):
    sweeps, model, tag = scene["sweeps"], None, "scene"
    if how == "wide":
        d = feed(new_map(initial_slots=8192), sweeps)
        assert d.stats()["slots"] >= 8192
    elif how == "shuffled":
        rng = np.random.default_rng(4)
        d = feed(new_map(), [(p[rng.permutation(len(p))], o) for p, o in sweeps])    # (stride 1: every ray of a call is traced)
    elif how == "loaded":
        path = str(tmp_path / "map.lxdm")
        scene["map"].save(path)
        d = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
        d.load(path)
    else:
        d = feed(new_map(), sweeps)
        model, tag = copy.deepcopy(scene["model"]), "pruned"
        assert d.prune() == model.prune() == 23
    ends, _ = rays_of(scene, 257)
    for cfg, kw in CONFIGS.items():
        got = device_cast(d, ends, scene["origin"], **kw)
        check(got, want_of(scene, 257, model, tag, **kw))
        if how != "pruned":
            assert rm.same_records(got[0], device_cast(scene["map"], ends, scene["origin"], **kw)[0])
    if how == "pruned":    # without its dynamic voxels the map answers as the whole map does under the rule (the survivors keep their words)
        check(device_cast(d, ends, scene["origin"]), want_of(scene, 257, rule=cm.DEFAULT_RULE))


# ---- 5: the empty map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("carving", [False, True])
def test_empty_map(scene, carving):
    d = new_map(carving=carving)
    ends, walks = rays_of(scene, 257)
    for skip in (0, 2):
        rec, counts = d.raycast(ends, scene["origin"], skip_steps=skip)
        check((rec, counts), want_of(scene, 257, cm.CarveModel(leaf=LEAF), "empty", skip_steps=skip))
        traced = np.array([c is not None and n <= 4096 for c, n in walks])
        steps = np.array([max(n + 1 - skip, 0) if t else 0 for (c, n), t in zip(walks, traced)], np.uint32)
        assert np.array_equal(rec["status"], np.where(traced, rm.MISS, rm.NOT_TRACED)) and np.array_equal(rec["steps"], steps)
        assert counts == dict(not_traced=int((~traced).sum()), miss=int(traced.sum()), hit=0, hit_end=0, cells=int(steps.sum()))
    assert len(d) == 0 and d.stats()["offered"] == 0


# ---- 6: skip_steps and max_steps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(skip_steps=0), dict(skip_steps=2), dict(skip_steps=100), dict(max_steps=8), dict(max_steps=8, skip_steps=2)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_skip_steps_and_max_steps(scene, kw):
    ends, walks = rays_of(scene, 257)
    for cfg in CONFIGS.values():
        got = device_cast(scene["map"], ends, scene["origin"], **cfg, **kw)
        check(got, want_of(scene, 257, **cfg, **kw))
    rec, counts = got
    if kw.get("skip_steps") == 100:    # beyond every n_steps of the scene: nothing is looked up
        assert counts["cells"] == 0 and counts["hit"] == counts["hit_end"] == 0 and not rec["steps"].any()
    if "max_steps" in kw:
        longer = sum(1 for c, n in walks if c is None or n > 8)
        assert counts["not_traced"] == longer > 4 and sum(1 for c, n in walks if c is not None and n == 8) > 0


# ---- the hand cases of tests/test_densemap_raycast_cpu.py on the device, from the centre of a cell (the ties of the exact diagonal) -----
def test_hand_cases_on_the_device():
    o = (0.25, 0.25, 0.25)

    def pts(*xyz):
        p = np.zeros((len(xyz), 4), np.float32)
        p[:, :3] = xyz
        return p

    ends = pts(o, (1.25, 1.25, 1.25), (-0.25, -0.25, -0.25), (2.25, 0.25, 0.25), (-0.75, 0.25, 0.25), (3.75, 0.25, 0.25),
               (np.nan, 0.25, 0.25), (524288.0, 0.25, 0.25), (0.25, 0.25, -524287.75))
    voxels = pts((0.3, 0.4, 0.1), (0.3, 0.6, 0.1), (0.3, 0.6, 0.6), (0.6, 0.6, 0.1), (1.1, 1.2, 1.3), (-0.3, -0.2, 0.2), (-0.3, -0.3, -0.3),
                 (1.3, 0.3, 0.3), (2.3, 0.3, 0.3), (2.4, 0.2, 0.1), (-0.3, 0.3, 0.2))
    d, m = new_map(), cm.CarveModel(leaf=LEAF)
    for t in (d, m):
        feed(t, [(voxels, o)] + [(pts((3.25, 0.25, 0.25)), o)] * 4)    # four rays through the voxels of cells (2, 0, 0) and (4, 0, 0)
    assert m.dynamic_mask().sum() >= 1
    for kw in (dict(), dict(skip_steps=1), dict(skip_steps=4), dict(skip_steps=5), dict(max_steps=4), dict(max_steps=3), dict(min_points=2),
               dict(min_points=3), dict(rule=cm.DEFAULT_RULE), dict(rule=(1, 0, 1)), dict(rule=cm.DEFAULT_RULE, min_points=2, skip_steps=1)):
        check(device_cast(d, ends, o, **kw), rm.cast(m, ends, o, **kw))
    # the origin's own cell holds a voxel: every ray ends there at once, the zero-length one in its end cell and with range 0
    rec, _ = device_cast(d, ends, o)
    assert rec["status"].tolist()[:3] == [rm.HIT_END, rm.HIT, rm.HIT] and rec["steps"].tolist()[:3] == [0, 0, 0] and rec["range"][0] == 0
    # past it, the two diagonals (every step a tie: x, then y, then z) find (1, 1, 0) and (-1, 0, 0), not the voxels beside the walk
    rec, _ = device_cast(d, ends, o, skip_steps=1)
    assert rec["status"].tolist()[:3] == [rm.MISS, rm.HIT, rm.HIT] and rec["steps"].tolist()[:3] == [0, 2, 1]
    assert rec["key"].tolist()[1:3] == [cm.key_of((1, 1, 0)), cm.key_of((-1, 0, 0))]
    # an origin outside the key range, and one in the last cell inside it
    for origin in ((524288.0, 0.25, 0.25), (0.25, np.nan, 0.25), (524287.75, 0.25, 0.25), (-524287.25, 0.25, 0.25)):
        e = pts((origin[0] - 1.0 if origin[0] > 0 else origin[0] + 1.0, 0.25, 0.25), o)
        check(device_cast(d, e, origin, max_steps=65536), rm.cast(m, e, origin, max_steps=65536))


# ---- 7: the registered cloud of a mapper, where it lies -----------------------------------------------------------------------------
def test_raycast_from_map():
    w = synth.World(half_extent=65.0)
    cmap, smap = w.make_map(60_000)
    poses = synth.trajectory(2)
    sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
    mp.load_cubes(cmap, smap)
    d = loamx.DenseMap(leaf=LEAF, initial_slots=1 << 14)
    rc, rec, counts = d.raycast_from(mp)
    assert rc == loamx.SKIPPED and len(rec) == 0 and not any(counts.values())    # the mapper has not processed a sweep
    for t in range(2):
        sw = synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=900 + t, az_steps=900)
        f = sr.process(sw.points.copy(), sw.ring_sizes)
        od.process(f)
        lc, ls = od.last_clouds()
        full = od.transform_to_end(f["full"])
        mp.update_odometry(od.transform_sum)
        _, reg = mp.process(lc, ls, full)
        origin = mp.transform("aft")[3:]
        if t == 0:
            assert d.add_from(mp) == loamx.OK    # the first sweep is the map; the second is checked against it below
        rc, rec, counts = d.raycast_from(mp, capacity=64)    # (too little room at first: the binding doubles it)
        want, wcounts = d.raycast(reg, origin)
        assert rc == loamx.OK and len(rec) == len(reg) > 10000
        assert rm.same_records(rec, want), explain(rec, want)
        assert counts == wcounts and counts["not_traced"] == 0
        _, _, only = d.raycast_from(mp, records=False, skip_steps=2)
        assert only == d.raycast(reg, origin, skip_steps=2, records=False)[1]
        if t == 0:
            assert counts["miss"] == 0 and counts["hit_end"] > 0    # every ray ends in a voxel that holds its own end point
        else:
            assert counts["hit"] + counts["hit_end"] > 0
    print(counts)


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(scene):
    d, L = scene["map"], loamx.lib()
    ends, _ = rays_of(scene, 65)
    before, want = exports(d), want_of(scene, 65)
    cl, o = loamx.cloud_of(ends), np.asarray(scene["origin"], np.float32)
    op, counts = o.ctypes.data_as(C.c_void_p), np.zeros(5, np.uint64)
    cp = counts.ctypes.data_as(C.c_void_p)
    buf = np.zeros(65, rm.RAY_DTYPE)
    bp = buf.ctypes.data_as(C.c_void_p)
    plain = new_map(carving=False)
    feed(plain, scene["sweeps"][:1])
    rule, bad_rule = loamx.StaticRule(), loamx.StaticRule(den=0)

    def cfg(**kw):
        return C.byref(loamx._cfg(loamx.RaycastConfig, "loamx_densemap_raycast_default_config", **kw))

    cases = [(lambda: L.loamx_densemap_raycast(None, C.byref(cl), op, None, None, bp, C.c_uint64(65), cp), b"h is NULL"),
             (lambda: L.loamx_densemap_raycast(d.h, None, op, None, None, bp, C.c_uint64(65), cp), b"ends is NULL"),
             (lambda: L.loamx_densemap_raycast(d.h, C.byref(cl), None, None, None, bp, C.c_uint64(65), cp), b"origin is NULL"),
             (lambda: L.loamx_densemap_raycast(d.h, C.byref(cl), op, None, None, bp, C.c_uint64(65), None), b"counts is NULL"),
             (lambda: L.loamx_densemap_raycast(d.h, C.byref(cl), op, cfg(max_steps=0), None, bp, C.c_uint64(65), cp), b"max_steps"),
             (lambda: L.loamx_densemap_raycast(d.h, C.byref(cl), op, cfg(max_steps=65537), None, bp, C.c_uint64(65), cp), b"max_steps"),
             (lambda: L.loamx_densemap_raycast(d.h, C.byref(cl), op, cfg(min_points=0), None, bp, C.c_uint64(65), cp), b"min_points"),
             (lambda: L.loamx_densemap_raycast(d.h, C.byref(cl), op, None, C.byref(bad_rule), bp, C.c_uint64(65), cp), b"den"),
             (lambda: L.loamx_densemap_raycast(plain.h, C.byref(cl), op, None, C.byref(rule), bp, C.c_uint64(65), cp), b"carving"),
             (lambda: L.loamx_densemap_raycast_from_map(d.h, None, None, None, bp, C.c_uint64(65), cp), b"m is NULL"),
             (lambda: L.loamx_densemap_raycast_from_pipeline(d.h, None, C.c_uint32(0), None, None, bp, C.c_uint64(65), cp), b"p is NULL")]
    plain_before = plain.points().tobytes()
    for call, word in cases:
        assert call() == loamx.E_INVALID and word in L.loamx_last_error(), word
        assert not buf.tobytes().strip(b"\0") and not counts.any()    # nothing written
    assert L.loamx_densemap_raycast(d.h, C.byref(cl), op, None, None, bp, C.c_uint64(64), cp) == loamx.E_CAPACITY
    assert not buf.tobytes().strip(b"\0") and not counts.any()
    with pytest.raises(loamx.LoamxError) as e:
        d.raycast(ends, scene["origin"], max_steps=65537)
    assert e.value.code == loamx.E_INVALID and "max_steps" in str(e.value)
    # max_steps 65536 and the largest skip_steps are fine; the map and a following cast are what they were
    check(d.raycast(ends, scene["origin"], max_steps=65536), want)
    assert d.raycast(ends, scene["origin"], skip_steps=0xffffffff, records=False)[1]["cells"] == 0
    assert exports(d) == before and plain.points().tobytes() == plain_before
    check(d.raycast(ends, scene["origin"]), want)
    # counts only without carving, and an empty cloud
    assert plain.raycast(ends, scene["origin"], records=False)[1]["hit"] > 0
    rec, counts0 = d.raycast(np.zeros((0, 4), np.float32), scene["origin"])
    assert len(rec) == 0 and not any(counts0.values())
