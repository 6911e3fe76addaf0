"""GPU: the dense map's sweep log and its rebuild from corrected poses (include/loamx.h, loamx_densemap_enable_history and what follows
it) against the model of tests/densemap_rebuild_model.py: by definition a rebuilt map is what a fresh handle fed with the corrected sweeps
holds, so the models of the map, of carving, of the moments and of the file are the oracle.  Leaf 0.5, initial_slots 1024 and the scene
of tests/test_gpu_densemap_file.py: the three 4,100-point box sweeps with clutter; one of them carries NaN, inf and -0.0 rows.  Every
compared quantity is an integer word or a byte string.  No tolerance anywhere."""
import numpy as np
import pytest

import densemap_align_model as am
import densemap_file_model as fm
import densemap_rebuild_model as rm
from loam_velodyne_amd import loamx, synth

pytestmark = pytest.mark.gpu

LEAF = 0.5
ALL_FLAGS = [0, 1, 2, 3]
ODD_ROWS = np.float32([[np.nan, 0.0, 0.0, 1.0], [1.0, np.inf, 2.0, 0.0], [-0.0, -0.0, 0.5, -0.0], [-np.inf, np.nan, 1.0, 3.0]])


def new_map(flags, history=True, leaf=LEAF, initial_slots=1024, max_bytes=0, initial_points=1 << 20, **kw):
    d = loamx.DenseMap(leaf=leaf, initial_slots=initial_slots, **kw)
    # (history between the two: it may be enabled in any order with them)
    if flags & 1:
        d.enable_carving(ray_stride=2)
    if history:
        d.enable_history(max_bytes=max_bytes, initial_points=initial_points)
    if flags & 2:
        d.enable_moments()
    return d


def factory(flags):
    return lambda: fm.model_of(flags, LEAF, ray_stride=2)


def feed(target, sweeps):
    for p, o in sweeps:
        assert target.add(p, o) == loamx.OK
    return target


def saved(d, tmp_path, name="map.lxdm"):
    path = str(tmp_path / name)
    d.save(path)
    return open(path, "rb").read()


def state(d, tmp_path):
    """what a refused call must leave alone: the bytes of save, stats, history_size (None without history) and rebuild_stats[0]"""
    try:
        hs = d.history_size()
    except loamx.LoamxError:
        hs = None
    return saved(d, tmp_path, "state.lxdm"), d.stats(), hs, d.rebuild_stats()["rebuilds"]


def clutter(rng, n):
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = rng.uniform(am.BOX_LO + 0.6, am.BOX_HI - 0.6, (n, 3))
    return p


def line(n, first=0, y=0.1):
    """n points, one per voxel, on a line along x from cell `first`"""
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = (first + np.arange(n) + 0.25) * LEAF
    p[:, 1], p[:, 2] = y, 0.2
    return p


def shift_x(cells):
    return rm.rigid([0, 0, 0], [cells * LEAF, 0, 0])


def corrections(rng, n, quarter_at=None):
    """one rigid correction per call: a rotation of up to 0.2 rad about a random axis through a point of the box, a translation of up to
    two leaves; call quarter_at is turned by a quarter turn about +y instead"""
    out = []
    for k in range(n):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        w = np.float64([0.0, np.pi / 2, 0.0]) if k == quarter_at else axis * rng.uniform(0.05, 0.2)
        out.append(rm.rigid(w, rng.uniform(-2 * LEAF, 2 * LEAF, 3), rng.uniform(am.BOX_LO, am.BOX_HI)))
    return np.stack(out)


@pytest.fixture(scope="module")
def scene():
    S = am.box_scene()
    rng = np.random.default_rng(99)
    S["sweeps"] = [(np.concatenate([p, clutter(rng, 100)]), np.float32(o)) for p, o in S["sweeps"]]
    S["sweeps"][1][0][-4:] = ODD_ROWS
    assert [len(p) for p, _ in S["sweeps"]] == [4100] * 3
    S["fourth"] = (np.concatenate([am.box_points(rng, 4000), clutter(rng, 100)]), np.float32((0.2, 0.1, -0.3)))
    crng = np.random.default_rng(5)
    S["C1"] = corrections(crng, 3, quarter_at=1)
    S["C2"] = corrections(crng, 4, quarter_at=2)    # (its first three for the three sweeps)
    S["plain"] = {f: fm.to_bytes(rm.rebuild(factory(f), S["sweeps"])) for f in ALL_FLAGS}
    S["under_C1"] = {f: rm.rebuild(factory(f), S["sweeps"], S["C1"]) for f in ALL_FLAGS}
    return S


# ---- 1. the log ---------------------------------------------------------------------------------------------------------------------
def test_log_holds_the_bytes_that_were_added(scene):
    d = new_map(0, initial_points=5000)    # (grows twice on the way: 5000 -> 10000 -> 20000)
    assert d.history_size() == (0, 0)
    feed(d, scene["sweeps"][:2])
    assert d.add(np.zeros((0, 4), np.float32), (1, 2, 3)) == loamx.OK     # an empty cloud is no call
    feed(d, scene["sweeps"][2:])
    small = new_map(0, max_voxels=100)
    with pytest.raises(loamx.LoamxError) as e:
        small.add(*scene["sweeps"][0])
    assert e.value.code == loamx.E_CAPACITY and small.history_size() == (0, 0)
    assert d.history_size() == (3, 12300)
    for k in (2, 0, 1):
        p, o = d.history(k)
        assert p.tobytes() == scene["sweeps"][k][0].tobytes() and o.tobytes() == scene["sweeps"][k][1].tobytes()
    with pytest.raises(loamx.LoamxError) as e:
        d.history(3)
    assert e.value.code == loamx.E_INVALID
    # the C entry point with too little room: LOAMX_E_CAPACITY, the needed count, no point written
    out = np.full((4099, 4), np.float32(7))
    c, o = loamx.cloud_of(out), np.zeros(3, np.float32)
    import ctypes as C
    assert loamx.lib().loamx_densemap_history_download(d.h, C.c_uint64(0), C.byref(c), o.ctypes.data_as(C.c_void_p)) == loamx.E_CAPACITY
    assert c.count == 4100 and np.all(out == 7)
    d.reset()     # the log is emptied, history stays on
    assert d.history_size() == (0, 0)
    feed(d, scene["sweeps"][1:2])
    assert d.history_size() == (1, 4100) and d.history(0)[0].tobytes() == scene["sweeps"][1][0].tobytes()


def test_log_of_a_pipeline_slot():
    ns, T = 2, 4
    w = synth.World(half_extent=45.0)
    cm, sm = w.make_map(60_000)
    sweeps, starts = [[None] * ns for _ in range(T)], []
    for s in range(ns):
        poses = synth.trajectory(T, start=(1.5 * s, 0.0, 2.0 * s))
        starts.append(np.array([0, 0, 0, 1.5 * s, 0, 2.0 * s], np.float32))
        for t in range(T):
            sw = synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=30 * s + t, az_steps=900)
            sweeps[t][s] = (np.ascontiguousarray(sw.points, np.float32), sw.ring_sizes)
    p = loamx.Pipeline(ns)
    p.set_frozen(cm, sm)
    for s in range(ns):
        p.set_state(s, aft=starts[s])
    p.upload(sweeps)
    dense = [new_map(0, leaf=0.1, initial_slots=1 << 16, initial_points=30000) for _ in range(ns)]
    want = [[] for _ in range(ns)]
    for t in range(T):
        if p.step(t) == loamx.OK:
            for k in range(ns):
                assert dense[k].add_from_pipeline(p, k) == loamx.OK
                want[k].append((p.download_full_res(k, len(sweeps[t][k][0])), np.float32(p.get(k)[2][3:])))
        else:
            assert dense[0].add_from_pipeline(p, 0) == loamx.SKIPPED     # not logged
    assert len(want[0]) >= 2
    for k in range(ns):
        assert dense[k].history_size() == (len(want[k]), sum(len(c) for c, _ in want[k]))
        for j, (cloud, origin) in enumerate(want[k]):
            got, o = dense[k].history(j)
            assert got.tobytes() == np.ascontiguousarray(cloud[:, :4], np.float32).tobytes() and o.tobytes() == origin.tobytes()
        # and the log rebuilds the map it came from
        before = dense[k].points().tobytes()
        dense[k].rebuild()
        assert dense[k].points().tobytes() == before


# ---- 2. identity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_identity_rebuild_changes_nothing(scene, tmp_path, flags):
    d = feed(new_map(flags), scene["sweeps"])
    raw = saved(d, tmp_path)
    assert raw == scene["plain"][flags]

    def view():
        st = d.stats()
        st.pop("slots")
        return st, d.carve_stats() if flags & 1 else None

    before = view()
    d.rebuild(None)
    assert saved(d, tmp_path) == raw and view() == before
    # matrices that round to the identity, -0.0 entries among them, take the same path
    eye = np.tile(np.float64(rm.IDENTITY) * (1.0 + 2.0 ** -40), (3, 1, 1))
    eye[eye == 0.0] = -0.0
    d.rebuild(eye)
    assert saved(d, tmp_path) == raw and view() == before and d.rebuild_stats()["rebuilds"] == 2 and d.history_size() == (3, 12300)


# ---- 3. corrections -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_rebuild_under_corrections_equals_the_model(scene, tmp_path, flags):
    d = feed(new_map(flags), scene["sweeps"])
    voxels_before = d.stats()["voxels"]
    d.rebuild(scene["C1"])
    got = saved(d, tmp_path)
    model = scene["under_C1"][flags]
    assert got == fm.to_bytes(model) and got != scene["plain"][flags]
    # a fresh handle fed with the host-corrected sweeps (the library's own helper does the correcting)
    fresh = new_map(flags, history=False)
    for (p, o), c in zip(scene["sweeps"], scene["C1"]):
        fresh.add(loamx.correct(c, p), loamx.correct(c, o.reshape(1, 3))[0])
    assert saved(fresh, tmp_path, "fresh.lxdm") == got
    st, fs = d.stats(), fresh.stats()
    # the smallest power of two of slots >= initial_slots, >= 2 x the voxels before and >= 2 x the voxels after
    assert st.pop("slots") == rm.attempts(1024, voxels_before, len(model))[-1] and fs.pop("slots") >= 2 * len(model)
    assert st == fs and st["voxels"] == len(model) and st["dropped_range"] + st["dropped_key"] == 3
    if flags & 1:
        assert d.carve_stats() == fresh.carve_stats() and d.misses().tobytes() == fresh.misses().tobytes()
    if flags & 2:
        assert d.surfels().tobytes() == fresh.surfels().tobytes() and d.freeze() == fresh.freeze() > 100
    # the log is unchanged
    for k in range(3):
        assert d.history(k)[0].tobytes() == scene["sweeps"][k][0].tobytes()


# ---- 4. from the originals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 3])
def test_a_second_rebuild_starts_from_the_originals(scene, tmp_path, flags):
    d = feed(new_map(flags), scene["sweeps"])
    d.rebuild(scene["C1"])
    d.rebuild(scene["C2"][:3])
    e = feed(new_map(flags), scene["sweeps"])
    e.rebuild(scene["C2"][:3])
    twice = saved(d, tmp_path)
    assert twice == saved(e, tmp_path, "once.lxdm") and twice != fm.to_bytes(scene["under_C1"][flags])
    d.rebuild(None)
    assert saved(d, tmp_path) == scene["plain"][flags]


# ---- 5. adds go on ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 3])
def test_adds_go_on_after_a_rebuild(scene, tmp_path, flags):
    d = feed(new_map(flags), scene["sweeps"])
    d.rebuild(scene["C1"])
    feed(d, [scene["fourth"]])
    model = rm.rebuild(factory(flags), scene["sweeps"], scene["C1"])
    model.add(*scene["fourth"])
    assert saved(d, tmp_path) == fm.to_bytes(model)
    assert d.history_size() == (4, 16400) and d.history(3)[0].tobytes() == scene["fourth"][0].tobytes()     # logged as given
    d.rebuild(scene["C2"])
    assert saved(d, tmp_path) == fm.to_bytes(rm.rebuild(factory(flags), scene["sweeps"] + [scene["fourth"]], scene["C2"]))


# ---- 6. launch shape and table size -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,launches", [(0, 1), (2, 1), (1, 6), (3, 6)])
def test_launches(scene, flags, launches):
    d = feed(new_map(flags), scene["sweeps"])

    def grown_by(call):
        a = d.rebuild_stats()
        call()
        b = d.rebuild_stats()
        return tuple(b[k] - a[k] for k in ("rebuilds", "tables_tried", "launches", "points_replayed"))

    # three calls: one launch with carving off, an insert and a carve launch per call with carving on; the table of the map as it
    # stands holds the same map again
    assert grown_by(lambda: d.rebuild(None)) == (1, 1, launches, 12300)
    # under C1 the map has more voxels: every table tried costs the same launches, and the tables tried are the model's
    tries = len(rm.attempts(1024, d.stats()["voxels"], len(scene["under_C1"][flags])))
    assert grown_by(lambda: d.rebuild(scene["C1"])) == (1, tries, tries * launches, tries * 12300)


def spread_line(d):
    """three calls of 400 points on the same 400 voxels (the occupancy read after each: exact), and the corrections that pull them apart"""
    for _ in range(3):
        assert d.add(line(400), (0, 0, 0)) == loamx.OK
        assert d.stats()["voxels"] == 400
    return np.stack([shift_x(0), shift_x(400), shift_x(800)])


def test_table_growth(tmp_path):
    d = new_map(0)
    C = spread_line(d)
    a = d.rebuild_stats()
    d.rebuild(C)
    b = d.rebuild_stats()
    st = d.stats()
    assert st["voxels"] == 1200 and st["slots"] == 4096 and st["offered"] == st["added"] == 1200
    assert b["tables_tried"] - a["tables_tried"] == 3 == len(rm.attempts(1024, 400, 1200)) and b["launches"] - a["launches"] == 3
    model = rm.rebuild(factory(0), [(line(400), np.zeros(3, np.float32))] * 3, C)
    assert saved(d, tmp_path) == fm.to_bytes(model) and len(model) == 1200
    # and back: from the voxels the map has now, 1,200 -> 4096 slots at once
    d.rebuild(None)
    c = d.rebuild_stats()
    assert c["tables_tried"] - b["tables_tried"] == 1 and d.stats()["voxels"] == 400 and d.stats()["slots"] == 4096


# ---- 7. refusals leave the handle alone ---------------------------------------------------------------------------------------------
def refused(call, code=loamx.E_INVALID, says=None):
    with pytest.raises(loamx.LoamxError) as e:
        call()
    assert e.value.code == code
    if says:
        assert says in str(e.value)


def test_refusals_leave_the_handle_alone(scene, tmp_path):
    plain = feed(new_map(0, history=False), scene["sweeps"])
    before = state(plain, tmp_path)
    refused(lambda: plain.rebuild(scene["C1"]), says="history")
    refused(lambda: plain.history_size(), says="history")
    refused(lambda: plain.enable_history(), says="empty")     # the map holds points
    assert state(plain, tmp_path) == before

    d = feed(new_map(0), scene["sweeps"])
    before = state(d, tmp_path)
    refused(lambda: d.rebuild(scene["C1"][:2]), says="n_calls")
    refused(lambda: d.rebuild(scene["C2"]), says="n_calls")
    import ctypes as C
    assert loamx.lib().loamx_densemap_rebuild(d.h, None, C.c_uint64(2)) == loamx.E_INVALID     # with NULL too
    bad = scene["C1"].copy()
    bad[2, 1, 3] = np.nan
    refused(lambda: d.rebuild(bad), says="corrections")
    path = str(tmp_path / "other.lxdm")
    plain.save(path)
    refused(lambda: d.merge_file(path), says="log")
    refused(lambda: d.merge(plain), says="log")
    empty = new_map(0)
    refused(lambda: empty.load(path), says="log")
    assert empty.stats()["voxels"] == 0 and empty.history_size() == (0, 0)
    assert state(d, tmp_path) == before
    # the merge from a handle with history is fine
    plain.merge(d)
    assert plain.stats()["offered"] == 2 * 12300


def test_capacity_refusals_leave_the_handle_alone(scene, tmp_path):
    d = new_map(0, max_voxels=1000)
    C = spread_line(d)
    before = state(d, tmp_path)
    refused(lambda: d.rebuild(C), code=loamx.E_CAPACITY)      # 1,200 voxels
    assert state(d, tmp_path) == before and d.stats()["voxels"] == 400
    d.rebuild(C[[0, 1, 1]])                                   # 800 fit
    assert d.stats()["voxels"] == 800

    e = new_map(0, max_bytes=16 * (2 * 4100 - 1))             # one point short of the second sweep
    feed(e, scene["sweeps"][:1])
    before = state(e, tmp_path)
    refused(lambda: e.add(*scene["sweeps"][1]), code=loamx.E_CAPACITY)
    assert state(e, tmp_path) == before and e.history_size() == (1, 4100)
    assert e.add(scene["sweeps"][1][0][:-1], scene["sweeps"][1][1]) == loamx.OK      # exactly the cap
    assert e.history_size() == (2, 8199)


# ---- 8. the snapshot ----------------------------------------------------------------------------------------------------------------
def test_snapshot_is_not_touched(scene):
    d = feed(new_map(2), scene["sweeps"])
    n = d.freeze()
    rtc = am.rtc_of(scene["start"][:, :3], scene["start"][:, 3])
    s1, c1 = d.align_step(scene["cloud"], rtc, 1)
    d.rebuild(scene["C1"])
    s2, c2 = d.align_step(scene["cloud"], rtc, 1)
    assert s1.tobytes() == s2.tobytes() and c1.tobytes() == c2.tobytes() and c1[am.MATCHED] > 1000
    assert d.frozen_size == n > 300
