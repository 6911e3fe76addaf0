"""One cloud input: what the shared stager (csrc/cloud_stage.hpp, DmCloudStage) and the single body per feature could get wrong.

1. The same cloud by every way in gives the same bytes: ray cast, segment_cloud, the three alignments, add and PlaceDB.add through the
   host form, a mapper (the points a LaserMapping registered, read back and handed to the host form), a pipeline slot and, for the
   alignments, the sweep log; clouds of 0, 1, 64, 65 and 4,097 points (one lane, one wave, one wave and one, one point past sixteen
   256-thread blocks).  A mapper has no empty registered cloud: its 0 case is the mapper that has not processed, which is SKIPPED.
2. Calls interleaved on one handle without a wait between them (the device block of the adds grows under a ray cast while an add may
   be in flight) equal the same calls made alone on fresh handles brought to the same map by waited-for adds; the same for PlaceDB.
3. Two host adds back to back: the second pack does not overwrite the pinned block before the first fetch has read it.
4. The differences between the forms that the unification keeps: SKIPPED before the pose's check, capacity after has_cloud, the
   message styles, pose NULL, the host form's origin check on a full place database, the empty cloud from the host.

The scene: a floor and two walls, 6 m a side, at leaf 0.1 m."""
import ctypes as C

import numpy as np
import pytest

import densemap_model as dm
from loam_velodyne_amd import loamx, synth

pytestmark = pytest.mark.gpu

LEAF = 0.1
SIZES = [0, 1, 64, 65, 4097]
ORIGIN = np.array([0.2, 0.1, -0.3], np.float32)
NEAR = np.array([[1.0, 0.0, 0.002, 0.01], [0.0, 1.0, 0.0, -0.02], [-0.002, 0.0, 1.0, 0.015]])   # a start pose a little off
ALIGN = dict(min_matched=1, max_iterations=6)
SHIFT = np.float32([0.06, -0.04, 0.05])    # what the logged clouds are moved by, off the map


def scene_points(seed, n):
    """n points on the floor y = -1 and the walls x = 3 and z = 3, a centimetre of noise; intensity = the surface"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 3, n)
    u, v, h = rng.uniform(-3.0, 3.0, n), rng.uniform(-3.0, 3.0, n), rng.uniform(-1.0, 1.5, n)
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = np.where(k == 1, 3.0, u)
    p[:, 1] = np.where(k == 0, -1.0, h)
    p[:, 2] = np.where(k == 2, 3.0, v)
    p[:, :3] += rng.normal(0.0, 0.004, (n, 3))
    p[:, 3] = k
    return p


BASE = [(scene_points(s, 40_000), ORIGIN) for s in (1, 2, 3)]


def new_map(extra=(), history=False, frozen=True, wait=True):
    """a handle with the base map (and the clouds of extra on top), every add waited for, the base frozen"""
    d = loamx.DenseMap(leaf=LEAF, initial_slots=1 << 14)
    d.enable_moments()
    if history:
        d.enable_history(initial_points=1 << 12)
    for k, (p, o) in enumerate(list(BASE) + list(extra)):
        assert d.add(p, o) == loamx.OK
        if wait:
            d.stats()
        if frozen and k == len(BASE) - 1:
            assert d.freeze_device() > 1000
    return d


def blob(r):
    """an alignment result (a dict, a list of them, or the ctypes array) as comparable bytes"""
    if isinstance(r, dict):
        return [np.asarray(list(v.values()) if isinstance(v, dict) else v).tobytes() for _, v in sorted(r.items())]
    if isinstance(r, list):
        return [blob(x) for x in r]
    return bytes(r)


def seg_blob(labels, segs, st):
    return labels.tobytes(), segs.tobytes(), {k: v for k, v in st.items() if k != "hooks_lost"}   # (lost hook attempts depend on the schedule)


def exports(d):
    st = d.stats()
    st.pop("slots")
    return st, d.points().tobytes()


@pytest.fixture(scope="module")
def world():
    """the frozen base map, and a mapper chain that registers any prefix of one VLP-16 sweep"""
    w = synth.World(half_extent=65.0)
    cmap, smap = w.make_map(60_000)
    poses = synth.trajectory(1)
    sw = synth.make_sweep(w, "VLP-16", poses[0], poses[1], seed=900, az_steps=900)
    sr, od = loamx.ScanRegistration(), loamx.LaserOdometry()
    f = sr.process(sw.points.copy(), sw.ring_sizes)
    od.process(f)
    lc, ls = od.last_clouds()
    full = od.transform_to_end(f["full"])
    assert len(full) > 4097
    cache = {}

    def registered(n):
        """(a mapper whose registered cloud has n points, those points, their origin); n = 0: a mapper that has not processed"""
        if n not in cache:
            mp = loamx.LaserMapping()
            mp.load_cubes(cmap, smap)
            if n == 0:
                cache[n] = (mp, np.zeros((0, 4), np.float32), np.zeros(3, np.float32))
            else:
                mp.update_odometry(od.transform_sum)
                _, reg = mp.process(lc, ls, full[:n])
                assert len(reg) == n
                cache[n] = (mp, reg, np.float32(mp.transform("aft")[3:]))
        return cache[n]

    return dict(map=new_map(), registered=registered)


# ---- 1: the same cloud, every way in ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_raycast_and_segment_cloud_by_host_and_by_mapper(world, n):
    d = world["map"]
    mp, reg, origin = world["registered"](n)
    rec, counts = d.raycast(reg, origin)
    rc, drec, dcounts = d.raycast_from(mp, capacity=max(n, 1))
    labels, segs, st = d.segment_cloud(reg, origin, which=loamx.CLOUD_ALL)
    src, dlabels, dsegs, dst = d.segment_cloud_from(mp, capacity=max(n, 1), which=loamx.CLOUD_ALL)
    assert rc == src == (loamx.OK if n else loamx.SKIPPED)
    assert len(rec) == len(labels) == n and sum(counts.values()) - counts["cells"] == n and st["offered"] == n
    assert drec.tobytes() == rec.tobytes() and dcounts == counts
    assert seg_blob(dlabels, dsegs, dst) == seg_blob(labels, segs, st)
    if n == 4097:
        assert counts["hit"] > 1000 and st["entered"] > 0    # the rays cross the walls; the sweep's points are not in the map


@pytest.mark.parametrize("n", SIZES)
def test_align_by_host_and_by_mapper(world, n):
    d = world["map"]
    mp, reg, origin = world["registered"](n)
    poses = np.stack([np.eye(3, 4), NEAR])
    want = (d.align(reg, NEAR, origin, **ALIGN), d.align_many(reg, poses, origin, raw=True, **ALIGN), d.align_pyramid(reg, NEAR, origin, **ALIGN))
    rc1, one = d.align_from(mp, NEAR, **ALIGN)
    rc2, many, best = d.align_many_from(mp, poses, raw=True, **ALIGN)
    rc3, pyr = d.align_pyramid_from(mp, NEAR, **ALIGN)
    assert rc1 == rc2 == rc3 == (loamx.OK if n else loamx.SKIPPED)
    if n:
        assert blob(one) == blob(want[0]) and (blob(many), best) == (blob(want[1][0]), want[1][1]) and blob(pyr) == blob(want[2])
        # pose NULL is the identity in the from forms
        assert blob(d.align_from(mp, **ALIGN)[1]) == blob(d.align(reg, np.eye(3, 4), origin, **ALIGN))
    else:
        assert want[0]["status"] == 2 and want[0]["counts"]["matched"] == 0    # the host form runs on an empty cloud: nothing matched


def test_align_by_host_and_by_the_log():
    d = new_map(history=True)
    clouds = []
    for n in SIZES:
        p, o = scene_points(100 + n, n), np.float32([0.1 * n % 1.0, 0.0, 0.5])
        p[:, :3] += SHIFT
        before = d.history_size()[0]
        assert d.add(p, o) == loamx.OK
        assert d.history_size()[0] == before + (1 if n else 0)    # an empty cloud from the host is not a logged call
        if n:
            clouds.append((before, p, o))
    poses = np.stack([np.eye(3, 4), NEAR])
    for call, p, o in clouds:
        assert blob(d.align_from_history(call, NEAR, **ALIGN)) == blob(d.align(p, NEAR, o, **ALIGN))
        assert blob(d.align_from_history(call, **ALIGN)) == blob(d.align(p, np.eye(3, 4), o, **ALIGN))
        got, want = d.align_many_from_history(call, poses, raw=True, **ALIGN), d.align_many(p, poses, o, raw=True, **ALIGN)
        assert (blob(got[0]), got[1]) == (blob(want[0]), want[1])
        assert blob(d.align_pyramid_from_history(call, NEAR, **ALIGN)) == blob(d.align_pyramid(p, NEAR, o, **ALIGN))
    # the 4,097 points find the map: three planes fix the translation, 4 mm of noise over a thousand points a plane and a lever of 3 m
    # under a rotation error of a milliradian stay well below a fifth of the leaf
    res = d.align_from_history(clouds[-1][0], min_matched=200)
    assert res["counts"]["matched"] > 2000 and np.abs(res["pose"][:, 3] + SHIFT).max() < LEAF / 5


@pytest.mark.parametrize("n", SIZES)
def test_add_and_place_add_by_host_and_by_mapper(world, n):
    mp, reg, origin = world["registered"](n)
    a, b = loamx.DenseMap(leaf=LEAF, initial_slots=1024), loamx.DenseMap(leaf=LEAF, initial_slots=1024)
    assert a.add(reg, origin) == loamx.OK and b.add_from(mp) == (loamx.OK if n else loamx.SKIPPED)
    m = dm.Model(leaf=LEAF)
    m.add(reg, origin)
    assert exports(a) == exports(b) and a.points().tobytes() == m.points().tobytes()
    pa, pb = loamx.PlaceDB(), loamx.PlaceDB()
    assert pa.add(reg, origin) == 0 and pb.add_from(mp) == (0 if n else None)
    if n:
        (da, ka), (db, kb) = pa.descriptor(0), pb.descriptor(0)
        assert da.tobytes() == db.tobytes() and ka.tobytes() == kb.tobytes() and da.any()


def test_a_pipeline_slot_equals_the_host_forms(world):
    ns, T = 1, 3
    w = synth.World(half_extent=45.0)
    cmap, smap = w.make_map(60_000)
    poses = synth.trajectory(T)
    sweeps = []
    for t in range(T):
        sw = synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=30 + t, az_steps=900)
        sweeps.append([(np.ascontiguousarray(sw.points, np.float32), sw.ring_sizes)])
    p = loamx.Pipeline(ns)
    p.set_frozen(cmap, smap)
    p.upload(sweeps)
    d = world["map"]
    assert d.raycast_from_pipeline(p, 0)[0] == d.align_from_pipeline(p, 0)[0] == loamx.SKIPPED    # before any step
    t = next(t for t in range(T) if p.step(t) == loamx.OK)
    reg, origin = p.download_full_res(0, len(sweeps[t][0][0])), np.float32(p.get(0)[2][3:])
    assert len(reg) > 4097
    poses2 = np.stack([np.eye(3, 4), NEAR])
    rc, rec, counts = d.raycast_from_pipeline(p, 0, capacity=64)
    hrec, hcounts = d.raycast(reg, origin)
    assert rc == loamx.OK and rec.tobytes() == hrec.tobytes() and counts == hcounts and counts["hit"] > 1000
    rc, labels, segs, st = d.segment_cloud_from_pipeline(p, 0, capacity=64)
    assert rc == loamx.OK and seg_blob(labels, segs, st) == seg_blob(*d.segment_cloud(reg, origin))
    rc, one = d.align_from_pipeline(p, 0, NEAR, **ALIGN)
    assert rc == loamx.OK and blob(one) == blob(d.align(reg, NEAR, origin, **ALIGN))
    rc, many, best = d.align_many_from_pipeline(p, 0, poses2, raw=True, **ALIGN)
    want, wbest = d.align_many(reg, poses2, origin, raw=True, **ALIGN)
    assert rc == loamx.OK and (blob(many), best) == (blob(want), wbest)
    rc, pyr = d.align_pyramid_from_pipeline(p, 0, NEAR, **ALIGN)
    assert rc == loamx.OK and blob(pyr) == blob(d.align_pyramid(reg, NEAR, origin, **ALIGN))
    a, b = loamx.DenseMap(leaf=LEAF, initial_slots=1024), loamx.DenseMap(leaf=LEAF, initial_slots=1024)
    assert a.add(reg, origin) == loamx.OK and b.add_from_pipeline(p, 0) == loamx.OK and exports(a) == exports(b)
    pa, pb = loamx.PlaceDB(), loamx.PlaceDB()
    assert pa.add(reg, origin) == 0 and pb.add_from_pipeline(p, 0) == 0
    assert [x.tobytes() for x in pa.descriptor(0)] == [x.tobytes() for x in pb.descriptor(0)]


# ---- 2: interleaving on one handle -----------------------------------------------------------------------------------------------------
def test_interleaved_calls_on_one_handle():
    c65, c4097, c1 = (scene_points(7, 65), ORIGIN), (scene_points(8, 4097), -ORIGIN), (scene_points(9, 1), ORIGIN)
    ends, probe = scene_points(10, 4097), scene_points(11, 4097)
    probe[:, :3] += np.float32([0.05, 0.03, -0.04])    # (off the surfaces: some of its points are new to the map)
    d = new_map()
    assert d.add(*c65) == loamx.OK
    rays = d.raycast(ends, ORIGIN)                      # (4,097 ends after 65 points: the device block of the adds grows)
    assert d.add(*c4097) == loamx.OK
    segs = d.segment_cloud(probe, ORIGIN, margin=0)    # (NEW: the points whose voxel the map, the 4,097 points included, does not hold)
    res = d.align(probe, NEAR, ORIGIN, **ALIGN)
    assert d.add(*c1) == loamx.OK
    got = exports(d)
    alone = new_map([c65])
    wrays = alone.raycast(ends, ORIGIN)
    assert rays[0].tobytes() == wrays[0].tobytes() and rays[1] == wrays[1] and rays[1]["hit"] + rays[1]["hit_end"] > 1000
    alone = new_map([c65, c4097])
    assert seg_blob(*segs) == seg_blob(*alone.segment_cloud(probe, ORIGIN, margin=0)) and segs[2]["entered"] > 0 and segs[2]["rejected"] > 0
    assert blob(res) == blob(alone.align(probe, NEAR, ORIGIN, **ALIGN)) and res["counts"]["matched"] > 1000
    assert got == exports(new_map([c65, c4097, c1]))
    m = dm.Model(leaf=LEAF)
    for p, o in list(BASE) + [c65, c4097, c1]:
        m.add(p, o)
    assert got[1] == m.points().tobytes()


def test_interleaved_calls_on_one_place_database():
    a, q, b = scene_points(21, 65), scene_points(22, 4097), scene_points(23, 4097)
    db = loamx.PlaceDB(max_range=10.0)
    assert db.add(a, ORIGIN) == 0
    found = db.query(q, ORIGIN, exclude_recent=0)       # (the device block grows behind the add's describe)
    assert db.add(b, -ORIGIN) == 1
    alone = loamx.PlaceDB(max_range=10.0)
    assert alone.add(a, ORIGIN) == 0 and alone.descriptor(0)[0].any()    # (the descriptor waits for the add)
    assert found == alone.query(q, ORIGIN, exclude_recent=0) and len(found) == 1
    assert alone.add(b, -ORIGIN) == 1
    for k in range(2):
        assert [x.tobytes() for x in db.descriptor(k)] == [x.tobytes() for x in alone.descriptor(k)]
    assert db.descriptor(0)[0].tobytes() != db.descriptor(1)[0].tobytes()


# ---- 3: the pinned block is not rewritten early ---------------------------------------------------------------------------------------
def test_two_host_adds_back_to_back():
    first, second = scene_points(31, 4097), scene_points(32, 4097)[::-1].copy()
    d = loamx.DenseMap(leaf=LEAF, initial_slots=1 << 14)
    assert d.add(first, ORIGIN) == loamx.OK and d.add(second, -ORIGIN) == loamx.OK
    m = dm.Model(leaf=LEAF)
    m.add(first, ORIGIN)
    m.add(second, -ORIGIN)
    assert d.points().tobytes() == m.points().tobytes() and len(d) == len(m)
    db, one, two = loamx.PlaceDB(max_range=10.0), loamx.PlaceDB(max_range=10.0), loamx.PlaceDB(max_range=10.0)
    assert db.add(first, ORIGIN) == 0 and db.add(second, ORIGIN) == 1
    assert one.add(first, ORIGIN) == 0 and two.add(second, ORIGIN) == 0
    assert db.descriptor(0)[0].tobytes() == one.descriptor(0)[0].tobytes() and db.descriptor(1)[0].tobytes() == two.descriptor(0)[0].tobytes()


# ---- 4: the differences that stay -------------------------------------------------------------------------------------------------------
def test_preserved_differences(world):
    d, L = world["map"], loamx.lib()
    idle, _, _ = world["registered"](0)                  # a mapper without a registered cloud
    mp, reg, origin = world["registered"](65)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    bad, good = np.full(12, np.nan), np.eye(3, 4).reshape(12).copy()
    one, six, best = loamx.AlignResult(), (loamx.AlignResult * loamx.PYRAMID_MAX_LEVELS)(), C.c_uint32(0)
    cl, o = loamx.cloud_of(reg), np.float32(origin)

    def says(rc, code, word):
        return rc == code and word in L.loamx_last_error()

    # the order of the checks against SKIPPED: the single form looks at the pose last, the pyramid before the cloud, the many form first
    assert L.loamx_densemap_align_from_map(d.h, idle.h, ptr(bad), None, C.byref(one)) == loamx.SKIPPED
    assert says(L.loamx_densemap_align_from_map(d.h, mp.h, ptr(bad), None, C.byref(one)), loamx.E_INVALID, b"the pose must be finite")
    assert says(L.loamx_densemap_align_pyramid_from_map(d.h, idle.h, ptr(bad), None, C.c_uint32(0), six), loamx.E_INVALID, b"the pose must be finite")
    assert says(L.loamx_densemap_align_many_from_map(d.h, idle.h, ptr(bad), C.c_uint32(1), None, six, C.byref(best)), loamx.E_INVALID,
                b"the pose must be finite")
    assert L.loamx_densemap_align_pyramid_from_map(d.h, idle.h, ptr(good), None, C.c_uint32(0), six) == loamx.SKIPPED
    assert L.loamx_densemap_align_many_from_map(d.h, idle.h, ptr(good), C.c_uint32(1), None, six, C.byref(best)) == loamx.SKIPPED
    # "nothing is frozen" comes before SKIPPED
    fresh = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
    assert says(L.loamx_densemap_align_from_map(fresh.h, idle.h, None, None, C.byref(one)), loamx.E_INVALID, b"nothing is frozen")
    # ray cast: capacity after has_cloud
    counts, hit = np.zeros(5, np.uint64), np.zeros(1, loamx.RAY_DTYPE)
    assert L.loamx_densemap_raycast_from_map(d.h, idle.h, None, None, ptr(hit), C.c_uint64(0), ptr(counts)) == loamx.SKIPPED
    assert L.loamx_densemap_raycast_from_map(d.h, mp.h, None, None, ptr(hit), C.c_uint64(0), ptr(counts)) == loamx.E_CAPACITY
    # pose NULL: the identity in the from forms only; the host forms require a pose and take a NULL centre
    assert L.loamx_densemap_align_from_map(d.h, mp.h, None, None, C.byref(one)) == loamx.OK
    assert says(L.loamx_densemap_align(d.h, C.byref(cl), None, ptr(o), None, C.byref(one)), loamx.E_INVALID, b"NULL argument")
    assert L.loamx_densemap_align(d.h, C.byref(cl), ptr(good), None, None, C.byref(one)) == loamx.OK
    assert says(L.loamx_densemap_align_pyramid(d.h, C.byref(cl), None, ptr(o), None, C.c_uint32(0), six), loamx.E_INVALID, b"NULL argument: pose_in")
    assert says(L.loamx_densemap_align_many(d.h, C.byref(cl), None, C.c_uint32(1), ptr(o), None, six, C.byref(best)), loamx.E_INVALID,
                b"NULL argument: poses_in")
    assert L.loamx_densemap_align_many_from_map(d.h, mp.h, None, C.c_uint32(1), None, six, C.byref(best)) == loamx.OK
    # the three message styles
    assert says(L.loamx_densemap_add(d.h, None, ptr(o)), loamx.E_INVALID, b"NULL argument") and b"NULL argument:" not in L.loamx_last_error()
    assert says(L.loamx_densemap_align_from_pipeline(d.h, None, C.c_uint32(0), None, None, C.byref(one)), loamx.E_INVALID, b"NULL argument")
    assert says(L.loamx_densemap_align_many_from_history(None, C.c_uint64(0), None, C.c_uint32(1), None, six, C.byref(best)), loamx.E_INVALID,
                b"NULL argument: h")
    assert says(L.loamx_densemap_raycast(d.h, None, ptr(o), None, None, None, C.c_uint64(0), ptr(counts)), loamx.E_INVALID, b"ends is NULL")
    nv, st = C.c_uint64(0), (C.c_uint64 * 13)()
    assert says(L.loamx_densemap_segment_cloud(d.h, None, ptr(o), None, None, None, C.c_uint64(0), C.byref(nv), None, C.c_uint64(0), C.byref(nv), st),
                loamx.E_INVALID, b"points is NULL")
    # place: the host form refuses a non-finite origin before it finds the database full; messages in the "NULL argument" style
    db, i = loamx.PlaceDB(max_entries=1), C.c_uint32(7)
    assert db.add(reg, origin) == 0
    nan = np.float32([0.0, np.nan, 0.0])
    assert says(L.loamx_place_add(db.h, C.byref(cl), ptr(nan), C.byref(i)), loamx.E_INVALID, b"origin must be finite")
    assert L.loamx_place_add(db.h, C.byref(cl), ptr(o), C.byref(i)) == loamx.E_CAPACITY
    assert L.loamx_place_add_from_map(db.h, mp.h, C.byref(i)) == loamx.E_CAPACITY and L.loamx_place_add_from_map(db.h, idle.h, C.byref(i)) == loamx.SKIPPED
    assert says(L.loamx_place_add(db.h, None, ptr(o), C.byref(i)), loamx.E_INVALID, b"NULL argument") and i.value == 7 and len(db) == 1
    # an empty cloud from the host: add is OK and changes nothing; ray cast and segmentation answer zeros
    empty, before = np.zeros((0, 4), np.float32), exports(d)
    assert d.add(empty, origin) == loamx.OK and exports(d) == before
    assert not any(d.raycast(empty, origin)[1].values()) and not any(d.segment_cloud(empty, origin)[2].values())
