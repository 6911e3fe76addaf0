"""GPU: views described from the dense map (include/loamx.h, loamx_place_add_views) against their model (tests/place_views_model.py, a
composition of the models of the map, the ray cast and the descriptor) and against the library's own single calls, DenseMap.raycast
-> PlaceDB.add of the hit positions.  Leaf 0.5, the box scene of tests/densemap_raycast_model.py (three sweeps with mid-air points,
carving on) plus hand-placed voxels: a few hundred voxels.  Every compared quantity is an integer or the bits of a float; the chain
test's last step, an alignment, is the one place with a bound, and the bound is the header's."""
import ctypes as C

import numpy as np
import pytest

import densemap_carve_model as cm
import densemap_model as dm
import densemap_raycast_model as rm
import place_model as pm
import place_views_model as vm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

F = np.float32
LEAF = vm.LEAF
PLACE = dict(max_range=8.0, min_range=0.5, height_offset=2.0)    # the floor lies at h <= 0 from most origins; min_range cuts the near hits
FAR_OFFSET = np.array([[6.0e5, 0.0, 0.0]], F)                    # its end lies outside the key range from every origin: NOT_TRACED
# hand-placed voxels, one point each: the one above ABOVE_ORIGIN (a = b = 0), and one 0.28 m beside lattice_origins()[0] in the
# horizontal (nearer than min_range), reached by NEAR_OFFSET from that origin
NEAR_POINT = np.array([[-0.25, -0.75, 0.25, 0.0]], F)
NEAR_OFFSET = np.array([[0.5, -1.0, 0.25]], F)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def new_map(initial_slots=1024, carving=True, moments=False):
    d = loamx.DenseMap(leaf=LEAF, initial_slots=initial_slots)
    if carving:
        d.enable_carving()
    if moments:
        d.enable_moments()
    return d


def feed(target, sweeps):
    for p, o in sweeps:
        r = target.add(p, o)
        assert r == loamx.OK or r is True
    return target


def pair(R=20, S=60, **kw):
    """a device database and its model with the same configuration"""
    cfg = dict(PLACE, **kw)
    model_kw = {k: v for k, v in cfg.items() if k != "initial_entries"}
    return loamx.PlaceDB(n_rings=R, n_sectors=S, exclude_recent=0, **cfg), pm.Model(R=R, S=S, exclude_recent=0, **model_kw)


def entry_bytes(db, i):
    d, k = db.descriptor(i)
    return d.tobytes() + k.tobytes()


def entries(db, first, n):
    return [entry_bytes(db, first + i) for i in range(n)]


def model_bytes(m, i):
    return np.asarray(m.desc[i], F).tobytes() + np.asarray(m.keys[i], F).tobytes()


def rule_of(rule):
    return None if rule is None else loamx.StaticRule(*rule)


@pytest.fixture(scope="module")
def scene():
    S = rm.box_cast_scene()
    sweeps = list(S["sweeps"]) + [(vm.ABOVE_POINT, (10.0, 0.0, 10.0)), (NEAR_POINT, (0.5, 0.5, 0.5))]
    S["sweeps"] = sweeps
    S["model"] = feed(cm.CarveModel(leaf=LEAF), sweeps)
    S["map"] = feed(new_map(), sweeps)
    assert len(S["model"]) == len(S["map"]) == 543 and int(S["model"].dynamic_mask().sum()) >= 10
    assert S["map"].points().tobytes() == S["model"].points().tobytes() and S["map"].misses().tobytes() == S["model"].misses().tobytes()
    assert S["map"].points()[:, :3].tobytes().count(vm.ABOVE_POINT[0, :3].tobytes()) == 1    # on the lattice: exported as placed
    return S


def offsets_of(n_rays):
    """n_rays offsets; from 3 rays on the last two are NEAR_OFFSET and FAR_OFFSET"""
    if n_rays < 3:
        return vm.lidar_offsets(n_rays)
    return np.concatenate([vm.lidar_offsets(n_rays - 2), NEAR_OFFSET, FAR_OFFSET])


def three_way(S, R, Sn, origins, offsets, rule=None, place=None, **cfg):
    """add_views == the model == raycast + add per origin: descriptor and ring-key bytes of every view, and the stats.  Returns the
    stats and the model's records' hit clouds per origin"""
    d, model = S["map"], S["model"]
    kw = dict(place or {})
    db, pmod = pair(R, Sn, **kw)
    single, _ = pair(R, Sn, **kw)
    first, stats = db.add_views(d, origins, offsets, static=rule_of(rule), **cfg)
    mfirst, mstats = vm.add_views(model, pmod, origins, offsets, rule=rule, **cfg)
    tot = dict.fromkeys(rm.COUNT_KEYS, 0)
    clouds = []
    for o in origins:
        rec, counts = d.raycast(vm.ends_of(o, offsets), o, static=rule_of(rule), **cfg)
        clouds.append(vm.hit_cloud(rec))
        assert single.add(clouds[-1], o) == len(clouds) - 1
        for k in rm.COUNT_KEYS:
            tot[k] += counts[k]
    print(R, Sn, len(origins), len(offsets), cfg, stats)
    assert first == mfirst == 0 and len(db) == len(pmod) == len(single) == len(origins)
    assert stats == mstats == dict(entries=len(origins), **tot)
    for i in range(len(origins)):
        got = entry_bytes(db, i)
        assert got == model_bytes(pmod, i), ("model", i)
        assert got == entry_bytes(single, i), ("single calls", i)
    return stats, clouds, db


# ---- (a) three-way equality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R, Sn, n, n_rays", [(20, 60, 2, 600), (64, 128, 1, 257), (1, 4, 2, 255), (8, 12, 1, 256), (20, 60, 1, 1),
                                              (8, 12, 70, 40)])
def test_views_equal_model_and_single_calls(scene, R, Sn, n, n_rays):
    origins = vm.lattice_origins(n)
    stats, clouds, db = three_way(scene, R, Sn, origins, offsets_of(n_rays))
    assert sum(stats[k] for k in rm.COUNT_KEYS[:4]) == n * n_rays
    if n_rays >= 40:
        assert stats["hit"] >= n * n_rays // 2 and stats["not_traced"] == n    # FAR_OFFSET, once per view
        assert sum(1 for i in range(n) if db.descriptor(i)[0].any()) >= (n + 1) // 2    # (an origin inside a voxel sees that voxel alone)


CONFIGS = {"skip0": dict(skip_steps=0), "skip1": dict(skip_steps=1), "min2": dict(min_points=2), "rule": dict(rule=cm.DEFAULT_RULE),
           "steps6": dict(max_steps=6)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_configurations(scene, name):
    """two origins, the second inside an occupied voxel (a wall voxel's exported position), 257 rays"""
    inside = scene["model"].points()[100, :3]
    origins = np.stack([vm.lattice_origins(1)[0], inside]).astype(F)
    stats, clouds, _ = three_way(scene, 8, 12, origins, offsets_of(257), **CONFIGS[name])
    plain = vm.add_views(scene["model"], pm.Model(R=8, S=12, **PLACE), origins, offsets_of(257))[1]
    if name == "skip0":
        assert stats == plain
        # every ray from inside an occupied voxel hits it in cell 0
        own = scene["model"].points()[100, :3].tobytes()
        assert all(c[:3].tobytes() == own for c in clouds[1][:200])
    else:
        assert stats != plain    # the setting changes at least one count
    if name == "steps6":
        assert stats["not_traced"] > 2 and stats["hit"] > 0
    if name == "rule":
        assert stats["cells"] > plain["cells"]    # the transparent mid-air voxels let rays go on


def test_hand_cases(scene):
    """the hits the descriptor drops: exactly above the origin (a = b = 0), h <= 0, nearer than min_range, at or beyond max_range"""
    place = dict(max_range=3.0, min_range=0.5, height_offset=2.0)
    origins = np.stack([vm.lattice_origins(1)[0], vm.ABOVE_ORIGIN]).astype(F)
    offsets = np.concatenate([offsets_of(252), vm.ABOVE_OFFSETS])
    stats, clouds, db = three_way(scene, 8, 12, origins, offsets, place=place)
    kw = dict(R=8, S=12, **place)
    used, ring, sector, h, _ = pm.cells_of(clouds[0], origins[0], **kw)
    d = clouds[0][:, :3] - origins[0]
    r2 = d[:, 2] * d[:, 2] + d[:, 0] * d[:, 0]
    assert (h <= 0).sum() >= 1 and (r2 < F(0.25)).sum() >= 1 and (r2 >= F(9.0)).sum() >= 5 and used.sum() >= 20
    # the ray towards NEAR_POINT hits it, and it is nearer than min_range
    near = clouds[0][:, :3].tobytes().count(NEAR_POINT[0, :3].tobytes())
    assert near >= 1
    # from ABOVE_ORIGIN: one hit, straight above
    assert len(clouds[1]) == 1 and clouds[1][0, :3].tobytes() == vm.ABOVE_POINT[0, :3].tobytes()
    assert not db.descriptor(1)[0].any() and not db.descriptor(1)[1].any() and db.descriptor(0)[0].any()
    # with min_range 0 that hit passes the range rule (r2 = 0 >= 0) and the height rule, and no sector qualifies: a = b = 0
    zero = dict(max_range=3.0, min_range=0.0, height_offset=2.0)
    _, clouds0, db0 = three_way(scene, 8, 12, vm.ABOVE_ORIGIN[None], vm.ABOVE_OFFSETS, place=zero)
    assert len(clouds0[0]) == 1 and clouds0[0][0, 0] == vm.ABOVE_ORIGIN[0] and clouds0[0][0, 2] == vm.ABOVE_ORIGIN[2]
    used0, _, sector0, h0, _ = pm.cells_of(clouds0[0], vm.ABOVE_ORIGIN, R=8, S=12, **zero)
    assert sector0.tolist() == [-1] and h0[0] > 0 and not used0.any()
    assert not db0.descriptor(0)[0].any() and not db0.descriptor(0)[1].any()


# ---- (b) independence -------------------------------------------------------------------------------------------------------------------
def test_independence(scene):
    d = scene["map"]
    origins, offsets = vm.lattice_origins(70), offsets_of(40)
    db, _ = pair(8, 12)
    first, stats = db.add_views(d, origins, offsets)
    want = entries(db, first, 70)
    assert len(set(want)) > 40    # the views differ
    # 70 calls with one origin each
    one, _ = pair(8, 12)
    tot = dict.fromkeys(vm.STAT_KEYS, 0)
    for i in range(70):
        f, st = one.add_views(d, origins[i:i + 1], offsets)
        assert f == i
        for k in vm.STAT_KEYS:
            tot[k] += st[k]
    assert entries(one, 0, 70) == want and tot == stats
    # the origins reversed: the entries reversed
    rev, _ = pair(8, 12)
    f, st = rev.add_views(d, origins[::-1], offsets)
    assert entries(rev, f, 70) == want[::-1] and st == stats
    # the rays permuted
    perm, _ = pair(8, 12)
    f, st = perm.add_views(d, origins, offsets[np.random.default_rng(1).permutation(len(offsets))])
    assert entries(perm, f, 70) == want and st == stats
    # the same map in a table of another size
    other = feed(new_map(initial_slots=1 << 16), scene["sweeps"])
    assert other.stats()["slots"] != d.stats()["slots"] and other.points().tobytes() == d.points().tobytes()
    big, _ = pair(8, 12)
    f, st = big.add_views(other, origins, offsets)
    assert entries(big, f, 70) == want and st == stats
    vox, _ = pair(8, 12)
    f, _ = vox.add_views(d, origins[:3])
    vox2, _ = pair(8, 12)
    f2, _ = vox2.add_views(other, origins[:3])
    assert entries(vox, f, 3) == entries(vox2, f2, 3)


# ---- (c) VOXELS mode ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R, Sn", [(20, 60), (64, 128), (1, 4), (8, 12)])
def test_voxels_mode(scene, R, Sn):
    d, model = scene["map"], scene["model"]
    origins = vm.lattice_origins(5)
    for cfg in (dict(), dict(min_points=2), dict(rule=cm.DEFAULT_RULE), dict(min_points=3, rule=cm.DEFAULT_RULE)):
        rule = cfg.get("rule")
        mp = cfg.get("min_points", 1)
        db, pmod = pair(R, Sn)
        first, stats = db.add_views(d, origins, static=rule_of(rule), min_points=mp)
        mfirst, mstats = vm.add_views(model, pmod, origins, rule=rule, min_points=mp)
        print(R, Sn, cfg, stats)
        assert first == mfirst == 0 and stats == mstats and stats["entries"] == 5 and 0 < stats["not_traced"] <= len(model)
        assert [entry_bytes(db, i) for i in range(5)] == [model_bytes(pmod, i) for i in range(5)]
        if mp == 1:    # the map seen through walls is the download, described
            cloud = d.points() if rule is None else d.points(static=rule_of(rule))
            assert stats["not_traced"] == len(cloud)
            single, _ = pair(R, Sn)
            for o in origins:
                single.add(cloud, o)
            assert entries(single, 0, 5) == entries(db, 0, 5)
    # explicit mode with offsets given is refused (and the other refusals: test_refusals)
    db, _ = pair(R, Sn)
    with pytest.raises(loamx.LoamxError) as e:
        db.add_views(d, origins, offsets_of(4), mode=loamx.PLACE_VIEW_VOXELS)
    assert e.value.code == loamx.E_INVALID and len(db) == 0


# ---- (d) the chain -------------------------------------------------------------------------------------------------------------------------
def test_chain_load_views_query_pose_align(tmp_path):
    """load -> views -> query -> view_pose -> align_many.  The scene and its ranking are fixed by tests/test_place_views_cpu.py (first
    0.0, second 0.4707).  The alignment's bound is the header's: a voxel position is good to about half a leaf, so the final
    translation lies within one leaf of the view's origin."""
    S = vm.chain_scene()
    src = feed(new_map(carving=False, moments=True), S["sweeps"])
    path = str(tmp_path / "prior.lxdm")
    src.save(path)
    d = new_map(carving=False, moments=True)    # a map that arrived by load: no sweeps, no place entries
    d.load(path)
    model = feed(dm.Model(leaf=LEAF), S["sweeps"])
    assert d.points().tobytes() == model.points().tobytes()
    db = loamx.PlaceDB(n_rings=S["place"]["R"], n_sectors=S["place"]["S"], max_range=S["place"]["max_range"], min_range=S["place"]["min_range"],
                       height_offset=S["place"]["height_offset"], exclude_recent=0)
    pmod = pm.Model(**S["place"], exclude_recent=0)
    host = np.random.default_rng(4).uniform(-3, 3, (50, 4)).astype(F)    # an entry from a sweep first: first_id is not 0
    assert db.add(host) == 0 == pmod.add(host)
    first, stats = db.add_views(d, S["origins"], S["offsets"])
    mfirst, mstats = vm.add_views(model, pmod, S["origins"], S["offsets"])
    assert first == mfirst == 1 and stats == mstats and len(db) == 10
    assert entries(db, 0, 10) == [model_bytes(pmod, i) for i in range(10)]
    o = S["origins"][4]
    rec, _ = d.raycast(vm.ends_of(o, S["offsets"]), o)
    hits = vm.hit_cloud(rec)
    q = vm.turned_query(hits, o, S["turn"], S["place"]["S"])
    got, want = db.query(q, (0, 0, 0), exclude_recent=0, n_results=10), pmod.query(q, (0, 0, 0), exclude_recent=0, n_results=10)
    print(got[:3])
    assert [(g[0], g[1]) for g in got] == [(w[0], w[1]) for w in want]
    assert np.asarray([g[2] for g in got], F).tobytes() == np.asarray([w[2] for w in want], F).tobytes()
    assert (got[0][0], got[0][1]) == (first + 4, S["turn"]) and got[1][2] - got[0][2] > 0.4
    P = loamx.view_pose(o, got[0][1], S["place"]["S"])
    assert P.tobytes() == vm.view_pose(o, got[0][1], S["place"]["S"]).tobytes()
    back = q[:, :3].astype(np.float64) @ P[:, :3].T + P[:, 3]
    tol = 4.0 * float(np.spacing(np.float32(np.abs(hits[:, :3]).max())))
    err = float(np.abs(back - hits[:, :3].astype(np.float64)).max())
    print("view_pose error", err, "tolerance", tol)
    assert err <= tol
    assert d.freeze() > 50
    res, best = d.align_many(q, P[None])
    t = np.asarray(res[0]["pose"], np.float64).reshape(3, 4)[:, 3]
    print("align", res[0]["status"], res[0]["iterations"], res[0]["counts"], t, o)
    assert best == 0 and res[0]["status"] == 0
    assert float(np.linalg.norm(t - o.astype(np.float64))) < LEAF


# ---- (e) housekeeping ---------------------------------------------------------------------------------------------------------------------
def test_growth_ids_save_load_capacity(scene, tmp_path):
    d, model = scene["map"], scene["model"]
    origins, offsets = vm.lattice_origins(5), offsets_of(40)
    db, pmod = pair(8, 12, initial_entries=1)
    host = scene["sweeps"][0][0][:500]
    assert db.add(host, (0.1, 0.2, 0.3)) == 0 == pmod.add(host, (0.1, 0.2, 0.3))
    old = entry_bytes(db, 0)
    first, stats = db.add_views(d, origins, offsets)    # room 1 -> 8: more than one doubling, in one step
    assert (first, len(db), db.growths) == (1, 6, 1) and stats["entries"] == 5
    assert vm.add_views(model, pmod, origins, offsets)[0] == 1
    assert entry_bytes(db, 0) == old == model_bytes(pmod, 0)
    assert entries(db, 0, 6) == [model_bytes(pmod, i) for i in range(6)]
    assert db.add(host[:100]) == 6 == first + 5 == pmod.add(host[:100])    # a host add afterwards continues the ids
    first2, _ = db.add_views(d, origins[:2])    # and so does a second call, in the other mode
    assert first2 == 7 == vm.add_views(model, pmod, origins[:2])[0] and len(db) == 9
    assert entries(db, 0, 9) == [model_bytes(pmod, i) for i in range(9)]
    # views are ordinary entries: query_entry, save and load
    q = scene["sweeps"][1][0][:800]
    want = pmod.query(q, (0.0, 0.1, 0.0), n_results=9)
    got = db.query(q, (0.0, 0.1, 0.0), n_results=9)
    assert [(g[0], g[1]) for g in got] == [(w[0], w[1]) for w in want]
    assert np.asarray([g[2:] for g in got], F).tobytes() == np.asarray([w[2:] for w in want], F).tobytes()
    assert [(g[0], g[1]) for g in db.query_entry(5, n_results=3)] == [(w[0], w[1]) for w in pmod.query_entry(5, n_results=3)]
    path = str(tmp_path / "views.lxpl")
    db.save(path)
    fresh, _ = pair(8, 12)
    fresh.load(path)
    assert len(fresh) == 9 and entries(fresh, 0, 9) == entries(db, 0, 9)
    back = fresh.query(q, (0.0, 0.1, 0.0), n_results=9)
    assert [(g[0], g[1]) for g in back] == [(g[0], g[1]) for g in got]
    assert np.asarray([g[2:] for g in back], F).tobytes() == np.asarray([g[2:] for g in got], F).tobytes()
    # max_entries: the call that would pass it is refused, size and bytes unchanged
    cap, _ = pair(8, 12, max_entries=6, initial_entries=2)
    assert cap.add_views(d, origins[:4], offsets)[0] == 0
    before = entries(cap, 0, 4)
    for kw in (dict(offsets=offsets), dict()):
        with pytest.raises(loamx.LoamxError) as e:
            cap.add_views(d, origins[:3], **kw)
        assert e.value.code == loamx.E_CAPACITY
    assert len(cap) == 4 and entries(cap, 0, 4) == before
    assert cap.add_views(d, origins[:2], offsets)[0] == 4 and len(cap) == 6    # exactly up to the cap


def test_empty_map(scene):
    e = new_map()
    origins, offsets = vm.lattice_origins(3), offsets_of(40)
    for kw, want in ((dict(offsets=offsets), dict(entries=3, not_traced=3, miss=117, hit=0, hit_end=0)), (dict(), dict(entries=3, not_traced=0, miss=0, hit=0, hit_end=0, cells=0))):
        db, _ = pair(8, 12)
        first, stats = db.add_views(e, origins, **kw)
        assert first == 0 and len(db) == 3 and {k: stats[k] for k in want} == want
        for i in range(3):
            dsc, key = db.descriptor(i)
            assert not dsc.any() and not key.any()
    assert e.stats()["voxels"] == 0


def test_refusals(scene):
    """every LOAMX_E_INVALID of the list names its argument and leaves the database's size and the map's stats as they were"""
    L = loamx.lib()
    d = scene["map"]
    db, _ = pair(8, 12)
    db.add_views(d, vm.lattice_origins(2), offsets_of(8))
    origins, offsets = vm.lattice_origins(3), np.ascontiguousarray(offsets_of(8))
    size, bytes_before = len(db), entries(db, 0, 2)
    before = (d.stats(), d.carve_stats(), d.points().tobytes())
    plain = new_map(carving=False)
    first, stats = C.c_uint32(77), np.full(6, 77, np.uint64)

    def call(pl=db.h, m=d.h, o=origins, n=3, f=offsets, n_rays=8, cfg=None, rule=None):
        k = None if cfg is None else C.byref(loamx.PlaceViewConfig(*cfg))
        return L.loamx_place_add_views(pl, m, ptr(o), C.c_uint32(n), ptr(f), C.c_uint32(n_rays), k, None if rule is None else C.byref(rule),
                                       C.byref(first), ptr(stats))

    def refused(rc, word):
        msg = L.loamx_last_error()
        assert rc == loamx.E_INVALID and word.encode() in msg, (rc, word, msg)
        assert len(db) == size and first.value == 77 and (stats == 77).all()

    refused(call(pl=None), "pl")
    refused(call(m=None), "dm")
    refused(call(o=None), "origins")
    refused(call(f=None), "offsets")
    refused(call(n=0), "n must")
    refused(call(o=np.zeros((4097, 3), F), n=4097), "LOAMX_PLACE_VIEW_MAX_ORIGINS")
    refused(call(n_rays=0), "n_rays")
    refused(call(f=np.zeros((65537, 3), F), n_rays=65537), "LOAMX_PLACE_VIEW_MAX_RAYS")
    refused(call(cfg=(2, 4096, 0, 1)), "mode")
    refused(call(cfg=(0, 0, 0, 1)), "max_steps")
    refused(call(cfg=(0, 65537, 0, 1)), "max_steps")
    refused(call(cfg=(0, 4096, 0, 0)), "min_points")
    refused(call(cfg=(1, 4096, 0, 0), f=None, n_rays=0), "min_points")
    refused(call(cfg=(1, 4096, 0, 1)), "offsets")
    refused(call(cfg=(1, 4096, 0, 1), f=None, n_rays=8), "n_rays")
    refused(call(rule=loamx.StaticRule(3, 1, 0)), "den")
    refused(call(m=plain.h, rule=loamx.StaticRule(3, 1, 1)), "carving")
    for bad in (np.nan, np.inf, -np.inf):
        o = origins.copy()
        o[2, 1] = bad
        refused(call(o=o), "origins")
        f = offsets.copy()
        f[7, 0] = bad
        refused(call(f=f), "offsets")
    assert entries(db, 0, 2) == bytes_before
    assert (d.stats(), d.carve_stats(), d.points().tobytes()) == before
    assert plain.stats()["offered"] == 0
    # NULL cfg, NULL rule, NULL first_id and NULL stats are allowed
    assert L.loamx_place_add_views(db.h, d.h, ptr(origins), C.c_uint32(3), ptr(offsets), C.c_uint32(8), None, None, None, None) == loamx.OK
    assert len(db) == size + 3


def test_handles_on_two_devices(scene):
    if loamx.device_count() < 2:
        pytest.skip("one device")
    other = loamx.PlaceDB(n_rings=8, n_sectors=12, device=1, **PLACE)
    with pytest.raises(loamx.LoamxError) as e:
        other.add_views(scene["map"], vm.lattice_origins(2), offsets_of(8))
    assert e.value.code == loamx.E_INVALID and "devices" in str(e.value) and len(other) == 0
