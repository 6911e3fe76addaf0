"""GPU: snapshots built on the device (include/loamx.h: loamx_densemap_freeze_device, loamx_densemap_freeze_pyramid_device,
loamx_densemap_freeze_history, loamx_densemap_download_frozen) and the alignment of a logged sweep where it lies
(loamx_densemap_align_*_from_history).

Everything here is a byte comparison.  freeze_device and freeze_pyramid_device against freeze and freeze_pyramid on the same handle,
through download_frozen: the same keys and the same six f32 per entry (k_dm_surfels runs the host's arithmetic, operation for
operation, and every operation is correctly rounded on either side).  freeze_history against its definition: the snapshot a fresh
handle holds after the window's corrected sweeps (tests/densemap_rebuild_model.py gives the corrected points) and freeze().  The
from_history forms against the host-fed forms on history(call) with its origin as the centre, struct for struct.

The end-to-end case closes a loop in the hall of the place tests (tests/place_model.py, revisit_case) from the log alone.  Its bars
are the ones tests/test_gpu_densemap_align_many.py holds the best hypothesis of a pose grid to at the same leaf, 0.01 rad and
leaf / 10, applied to the relative pose of the two keyframes."""
import ctypes as C

import numpy as np
import pytest

import densemap_align_model as am
import densemap_freeze_cases as fc
import densemap_model as dm
import densemap_moments_model as mm
import densemap_rebuild_model as rm
import place_model as pm
from loam_velodyne_amd import loamx, synth

pytestmark = pytest.mark.gpu

LEAF = 0.5


def new_map(carving=False, history=False, moments=True, leaf=LEAF, initial_slots=1024):
    d = loamx.DenseMap(leaf=leaf, initial_slots=initial_slots)
    if carving:
        d.enable_carving()
    if history:
        d.enable_history(initial_points=1 << 12)
    if moments:
        d.enable_moments()
    return d


def feed(d, sweeps):
    for p, o in sweeps:
        assert d.add(p, o) == loamx.OK
    return d


def entries(d, level=0):
    k, r = d.download_frozen(level)
    assert k.dtype == np.uint64 and r.dtype == np.float32 and r.shape == (len(k), 6)
    assert np.all(k[1:] > k[:-1])   # ascending, unique
    return k.tobytes(), r.tobytes(), len(k)


def same_on_both_sides(d, **freeze):
    """freeze, then freeze_device with the same arguments on the same handle: the same entries.  Returns (keys, records) of them"""
    n_host = d.freeze(**freeze)
    host = entries(d)
    keys, recs = d.download_frozen()
    n_dev = d.freeze_device(**freeze)
    dev = entries(d)
    assert n_host == n_dev == host[2] == dev[2] == d.frozen_size and d.frozen_levels == 1
    assert host[0] == dev[0], "keys differ"
    assert host[1] == dev[1], "records differ"
    return keys, recs


@pytest.fixture(scope="module")
def box():
    S = am.box_scene()
    S["map"] = feed(new_map(), S["sweeps"])
    return S


# ---- 1. freeze_device against freeze ------------------------------------------------------------------------------------------------
def test_box_and_plane(box):
    keys, recs = same_on_both_sides(box["map"])
    assert 400 < len(keys) <= 512
    # download_frozen itself: the surfels that have a normal, under the model's keys
    m = dm.Model(leaf=LEAF)
    for p, o in box["sweeps"]:
        m.add(p, o)
    want_keys, want_recs = am.frozen_of(m.keys, box["map"].surfels())
    assert keys.tobytes() == want_keys.tobytes() and recs.tobytes() == want_recs.tobytes()
    # other settings
    for kw in (dict(min_points=3), dict(min_points=12, min_planar_ratio=0.2), dict(min_planar_ratio=0.0)):
        same_on_both_sides(box["map"], **kw)
    d = feed(new_map(), [(am.lattice_plane(), am.PLANE_ORIGIN)])
    keys, recs = same_on_both_sides(d)
    assert len(keys) == 256 and np.all(recs[:, 3:] == np.float32([0, 0, 1]))


def test_with_a_rule_and_carving(box):
    rng = np.random.default_rng(8)
    d = new_map(carving=True)
    clutter = np.zeros((600, 4), np.float32)
    clutter[:, :3] = rng.uniform(-0.7, 0.7, (600, 3))      # blobs in mid-air: the later sweeps' rays cross them
    d.add(np.concatenate([box["sweeps"][0][0], clutter]), box["sweeps"][0][1])
    feed(d, box["sweeps"][1:])
    feed(d, [(am.box_points(rng, 4000), o) for o in ((1.0, 0.5, -0.5), (-1.0, -0.5, 0.5))])
    every, _ = same_on_both_sides(d, min_points=3)
    rule = loamx.StaticRule()
    same_on_both_sides(d, min_points=3, static=rule)
    static, _ = same_on_both_sides(d, min_points=3, static=loamx.StaticRule(min_misses=1, num=0, den=1))   # dynamic: crossed once
    assert 0 < len(static) < len(every)     # the rule drops voxels that have a surfel
    # the rule without carving is refused by either form
    for call in (box["map"].freeze, box["map"].freeze_device):
        with pytest.raises(loamx.LoamxError) as e:
            call(static=rule)
        assert e.value.code == loamx.E_INVALID and "carving" in str(e.value)


def test_a_grown_table_the_empty_map_and_a_map_without_surfels():
    d = new_map()
    assert d.freeze_device() == 0 and d.frozen_levels == 1 and entries(d)[2] == 0      # the empty map
    same_on_both_sides(d)
    rng = np.random.default_rng(3)
    p = np.zeros((30000, 4), np.float32)
    p[:, :3] = rng.uniform(-5.0, 5.0, (30000, 3))
    p[:, 1] = np.round(p[:, 1] / 4.0) * 4.0 + rng.normal(0.0, 0.01, 30000)             # sheets across y: most voxels are planar
    for k in range(3):
        d.add(p[10000 * k:10000 * (k + 1)], (0.0, 1.0, 0.0))
    assert d.rehashes >= 1 and d.stats()["slots"] >= 1 << 14                           # doubled on the way
    keys, _ = same_on_both_sides(d, min_points=3)
    assert len(keys) > 600                                                             # the snapshot's table is larger than 1024 slots too
    # one point per voxel: no voxel has a surfel
    d = new_map()
    line = np.zeros((700, 4), np.float32)
    line[:, 0] = (np.arange(700) + 0.25) * LEAF
    d.add(line, (0.0, 0.0, 1.0))
    assert len(d) == 700 and d.freeze_device(min_points=3) == 0 and entries(d)[2] == 0
    sums, counts = d.align_step(line[:100], am.rtc_of(), 1)
    assert counts[am.UNMATCHED] == 100 and not sums.any()
    same_on_both_sides(d, min_points=3)
    # moments off: refused as freeze is
    with pytest.raises(loamx.LoamxError) as e:
        new_map(moments=False).freeze_device()
    assert e.value.code == loamx.E_INVALID and "moments" in str(e.value)


def test_the_designed_voxels():
    cases = fc.point_cases()
    d, m = new_map(), mm.MomentsModel(leaf=LEAF)
    for c in cases:
        assert d.add(c["points"], c["origin"]) == loamx.OK
        m.add(c["points"], c["origin"])
    # the device holds the words the cases were designed as
    assert len(d) == len(cases) == len(m.keys)
    assert d.moments().tobytes() == m.moments().tobytes()
    by_key = {int(dm.keys_of(c["points"][:1], c["origin"], LEAF)[0][0]): c for c in cases}
    for key, vals, mom in zip(m.keys.tolist(), m.vals.tolist(), m.moments().tolist()):
        assert by_key[key]["vals"] == vals and by_key[key]["mom"] == mom
    seen = set()
    for cfg in sorted({(c["min_points"], c["min_planar_ratio"]) for c in cases}, key=str):
        keys, recs = same_on_both_sides(d, min_points=cfg[0], min_planar_ratio=cfg[1])
        # ... and the entries are the host's surfel of those words
        for key, rec in zip(keys.tolist(), recs):
            c = by_key[key]
            s = loamx.surfel_of(LEAF, c["idx"], c["vals"], c["mom"], min_points=cfg[0], min_planar_ratio=cfg[1])
            assert rec.tobytes() == s[[0, 1, 2, 4, 5, 6]].tobytes(), c["name"]
            if (c["min_points"], c["min_planar_ratio"]) == cfg:      # (under the settings the case was designed for)
                seen.add(c["name"])
    assert {"65536 points near the far corner", "symmetric about the origin, V = 0", "a cross, the two smallest equal, V = 0",
            "coplanar on axis 0, origin in the plane", "tilted plane, low side"} <= seen
    assert "collinear" not in seen and "one point" not in seen


def test_the_128_bit_voxel():
    """2^24 - 1 points on three corners of one voxel, the 128-bit path of tests/test_densemap_moments_cpu.py fed as points: n * Mxx is
    about 2^86.  One block of 2^20 points per corner, added in slices"""
    n = (1 << 24) - 1
    k = [n // 3 + 5, n // 3 - 1000, n - 2 * (n // 3) + 995]
    idx, Q = (3, -2, 1), fc.Q
    origin = fc.origin_of(idx, (-3 << 20, 4 << 20, -5 << 20))
    corners = [fc.points_of(idx, [q]) for q in ([Q, 0, 0], [0, Q, 0], [0, 0, Q])]
    d = new_map()
    V = [0, 0, 0]
    for kc, corner in zip(k, corners):
        block = np.repeat(corner, 1 << 20, axis=0)
        left = kc
        while left:
            m = min(left, 1 << 20)
            assert d.add(block[:m], origin) == loamx.OK
            left -= m
        w = mm.terms_of(corner, origin, LEAF)[1][0, 6:].astype(np.int64)
        V = [V[a] + kc * int(w[a]) for a in range(3)]
    vals = [n] + [x * Q for x in k]
    mom = [x * Q * Q for x in k] + [0, 0, 0] + [v % (1 << 64) for v in V]
    assert len(d) == 1 and d.moments().tolist() == [mom] and n * mom[0] > 1 << 84
    keys, recs = same_on_both_sides(d)
    s = loamx.surfel_of(LEAF, idx, vals, mom)
    assert len(keys) == 1 and recs[0].tobytes() == s[[0, 1, 2, 4, 5, 6]].tobytes()
    assert np.abs(np.abs(recs[0, 3:]) - 1.0 / np.sqrt(3.0)).max() < 1e-6       # the plane x + y + z = Q, exactly


def test_word_sets_loaded_from_a_file(tmp_path):
    """the word sets of the CPU test that no point set of ours sums to — the scatter integers whose conversion is a tie, just above
    2^53 and 2^64, both directions, both signs — and its 4,000 random voxels, put on the device as words through a map file"""
    import densemap_file_model as fm
    leaf = 0.1
    cases = fc.word_cases() + fc.random_cases(4000, seed=31)
    by_key = {}
    for k, c in enumerate(cases):
        idx = c["idx"] if c["name"] == "random" else (k - 3, 2 * k, 5 - k)      # (the designed ones share an index: apart)
        by_key[int(dm_key(idx))] = dict(c, idx=idx)
    assert len(by_key) == len(cases)
    keys = sorted(by_key)
    vals = np.array([[int(v) % (1 << 64) for v in by_key[k]["vals"]] for k in keys], np.uint64)
    mom = np.array([[int(v) % (1 << 64) for v in by_key[k]["mom"]] for k in keys], np.uint64)
    path = str(tmp_path / "words.lxdm")
    fm.write(path, dict(flags=fm.MOMENTS, leaf=np.float32(leaf), keys=np.array(keys, np.uint64), vals=vals, miss=None, mom=mom,
                        stats=(int(vals[:, 0].sum()), 0, 0), carve_stats=(0,) * 6, carve=(0.0, 0, 0, 0)))
    d = new_map(leaf=leaf)
    d.load(path)
    assert len(d) == len(cases) and d.moments().tobytes() == mom.tobytes()
    for cfg in ((None, None), (3, 0.0), (7, 0.2)):
        got_keys, recs = same_on_both_sides(d, min_points=cfg[0], min_planar_ratio=cfg[1])
        assert 1000 < len(got_keys) <= len(cases)
        for key, rec in zip(got_keys.tolist(), recs):
            c = by_key[key]
            s = loamx.surfel_of(leaf, c["idx"], c["vals"], c["mom"], min_points=cfg[0], min_planar_ratio=cfg[1])
            assert rec.tobytes() == s[[0, 1, 2, 4, 5, 6]].tobytes(), (c["name"], c["vals"], c["mom"])
        if cfg == (3, 0.0):
            assert sum(1 for key in got_keys.tolist() if by_key[key]["name"].startswith("ties")) == 4


def dm_key(idx):
    return sum((int(i) + (1 << 20)) << (21 * a) for a, i in enumerate(idx))


@pytest.mark.parametrize("n", [1, 65, 5000])
def test_a_step_reads_the_same_words_from_either_snapshot(box, n):
    d = box["map"]
    rng = np.random.default_rng(70 + n)
    cloud = am.box_points(rng, n, sigma=0.05)
    cloud[::7, :3] += 0.7                                   # some off the walls
    P = box["start"]
    cloud[:, :3] = (cloud[:, :3].astype(np.float64) - P[:, 3]) @ P[:, :3]
    rtc = am.rtc_of(P[:, :3], P[:, 3])
    words = []
    for freeze in (d.freeze, d.freeze_device):
        freeze()
        words.append([d.align_step(cloud, rtc, nb) for nb in (0, 1)])
    for (s0, c0), (s1, c1) in zip(*words):
        assert s0.tobytes() == s1.tobytes() and c0.tobytes() == c1.tobytes()
    assert n < 65 or words[0][1][1][am.MATCHED] > n // 4


# ---- 2. freeze_pyramid_device against freeze_pyramid --------------------------------------------------------------------------------
@pytest.mark.parametrize("max_curvature", [0.0, 0.02])
def test_pyramid_levels(box, max_curvature):
    d = box["map"]
    n_host = d.freeze_pyramid(levels=4, max_curvature=max_curvature)
    host = [entries(d, l) for l in range(4)]
    d.freeze()     # (the coarse levels go: what follows builds them anew)
    assert d.frozen_levels == 1
    n_dev = d.freeze_pyramid_device(levels=4, max_curvature=max_curvature)
    dev = [entries(d, l) for l in range(4)]
    assert n_host == n_dev == [h[2] for h in host] and d.frozen_levels == 4
    for l in range(4):
        assert host[l][0] == dev[l][0] and host[l][1] == dev[l][1], l
    assert n_dev[1] > 20
    if max_curvature:
        assert sum(n_dev[1:]) < sum(d.freeze_pyramid_device(levels=4)[1:])     # the limit drops coarse voxels
    assert d.freeze_pyramid_device(levels=1) == n_dev[:1] and d.frozen_levels == 1
    with pytest.raises(loamx.LoamxError):
        d.download_frozen(1)
    with pytest.raises(loamx.LoamxError) as e:
        d.freeze_pyramid_device(levels=loamx.PYRAMID_MAX_LEVELS + 1)
    assert e.value.code == loamx.E_INVALID and "levels" in str(e.value)


def test_pyramid_with_a_rule():
    S = am.box_scene()
    rng = np.random.default_rng(8)
    d = new_map(carving=True)
    clutter = np.zeros((600, 4), np.float32)
    clutter[:, :3] = rng.uniform(-0.7, 0.7, (600, 3))
    d.add(np.concatenate([S["sweeps"][0][0], clutter]), S["sweeps"][0][1])
    feed(d, S["sweeps"][1:])
    rule = loamx.StaticRule()
    n_host = d.freeze_pyramid(levels=3, min_points=3, static=rule)
    host = [entries(d, l) for l in range(3)]
    assert d.freeze_pyramid_device(levels=3, min_points=3, static=rule) == n_host
    assert [entries(d, l) for l in range(3)] == host


# ---- 3. freeze_history --------------------------------------------------------------------------------------------------------------
def saved(d, tmp_path):
    path = str(tmp_path / "live.lxdm")
    d.save(path)
    return open(path, "rb").read()


@pytest.fixture(scope="module")
def logged():
    """six sweeps of the box from six origins, the third with odd rows, in a map with history, moments and carving"""
    rng = np.random.default_rng(41)
    origins = [(0.4, -0.3, 0.1), (-1.2, 0.8, -0.4), (1.5, 0.6, 0.3), (0.2, 0.1, -0.3), (-0.5, -1.0, 0.6), (2.0, -1.5, 0.0)]
    sweeps = [(am.box_points(rng, 1500 + 200 * k), np.float32(o)) for k, o in enumerate(origins)]
    sweeps[2][0][-3:] = np.float32([[np.nan, 0.0, 0.0, 1.0], [1.0, np.inf, 2.0, 0.0], [-0.0, -0.0, 0.5, -0.0]])
    d = feed(new_map(carving=True, history=True), sweeps)
    assert d.history_size() == (6, sum(len(p) for p, _ in sweeps))
    crng = np.random.default_rng(5)
    general = np.stack([rm.rigid(crng.normal(size=3) * 0.1, crng.uniform(-1, 1, 3), crng.uniform(am.BOX_LO, am.BOX_HI)) for _ in range(6)])
    quarter = general.copy()
    quarter[1] = rm.rigid([0.0, np.pi / 2, 0.0], [0.25, -1.0, 3.0])
    quarter[4] = rm.rigid([0.0, 0.0, -np.pi / 2], [0.0, 0.0, 0.0])
    return dict(map=d, sweeps=sweeps, corrections=dict(identity=None, general=general, quarter=quarter))


def by_definition(sweeps, corrections, **freeze):
    """the entries a fresh handle with moments holds after the corrected sweeps and freeze()"""
    d = new_map()
    for p, o in rm.corrected_sweeps(sweeps, corrections):
        assert d.add(p, o) == loamx.OK
    d.freeze(**freeze)
    return entries(d)


@pytest.mark.parametrize("which", ["identity", "general", "quarter"])
@pytest.mark.parametrize("first,n", [(0, 1), (5, 1), (2, 3), (0, 6)])
def test_freeze_history_is_the_fresh_handle(logged, tmp_path, first, n, which):
    d, C_all = logged["map"], logged["corrections"][which]
    Cw = None if C_all is None else C_all[first:first + n]
    before = saved(d, tmp_path), d.stats(), d.carve_stats(), d.history_size(), d.rebuild_stats()
    got_n = d.freeze_history(first, n, Cw, min_points=4)
    got = entries(d)
    assert got_n == got[2] == d.frozen_size and d.frozen_levels == 1
    want = by_definition(logged["sweeps"][first:first + n], Cw, min_points=4)
    assert got[2] == want[2] > 50
    assert got[0] == want[0] and got[1] == want[1]
    # the live map, its statistics, its log and its carve words are untouched
    assert (saved(d, tmp_path), d.stats(), d.carve_stats(), d.history_size(), d.rebuild_stats()) == before
    if (first, n) == (2, 3):
        # corrections as 4x4, and an identity given as numbers, are the same calls
        if Cw is not None:
            C44 = np.concatenate([Cw, np.broadcast_to(np.float64([[[0, 0, 0, 1]]]), (n, 1, 4))], axis=1)
            assert d.freeze_history(first, n, C44, min_points=4) == got_n and entries(d) == got
        else:
            assert d.freeze_history(first, n, np.stack([np.eye(3, 4)] * n), min_points=4) == got_n and entries(d) == got


def test_freeze_history_differs_from_the_whole_map_and_grows_its_table(logged):
    d = logged["map"]
    whole = d.freeze_device(min_points=4)
    assert d.freeze_history(1, 2, min_points=4) < whole
    # a window with far more voxels than the live map holds: the scratch table starts small and doubles on the "too small" word.  (A
    # correction only has to be finite: this one stretches a dense sheet of 3 x 3 m to 60 x 60 m)
    rng = np.random.default_rng(12)
    sheet = np.zeros((40000, 4), np.float32)
    sheet[:, [0, 2]] = rng.uniform(-1.5, 1.5, (40000, 2))
    sheet[:, 1] = 0.1 + rng.normal(0.0, 0.01, 40000)
    g = new_map(history=True)
    g.add(sheet, (0.0, 1.0, 0.0))
    assert len(g) < 200
    stretch = np.float64([[[20, 0, 0, 0], [0, 1, 0, 0], [0, 0, 20, 0]]])
    n = g.freeze_history(0, 1, stretch, min_points=3)
    assert n > 1000 and entries(g) == by_definition([(sheet, (0.0, 1.0, 0.0))], stretch, min_points=3)
    stats = g.rebuild_stats()
    assert stats["rebuilds"] == 0 and stats["tables_tried"] == 0 and len(g) < 200      # the rebuild's statistics and the map stay


def test_freeze_history_refusals_keep_the_old_snapshot(logged):
    d = logged["map"]
    d.freeze_history(0, 2, min_points=4)
    old = entries(d)

    def refused(call, says, code=loamx.E_INVALID):
        with pytest.raises(loamx.LoamxError) as e:
            call()
        assert e.value.code == code and says in str(e.value), str(e.value)
        assert entries(d) == old and d.frozen_levels == 1

    refused(lambda: d.freeze_history(0, 0), "n_calls")
    refused(lambda: d.freeze_history(6, 1), "beyond the log")
    refused(lambda: d.freeze_history(4, 3), "beyond the log")
    refused(lambda: d.freeze_history(2 ** 64 - 1, 2), "beyond the log")
    bad = np.stack([np.eye(3, 4)] * 2)
    bad[1, 2, 3] = np.nan
    refused(lambda: d.freeze_history(0, 2, bad), "not finite")
    bad[1, 2, 3] = np.inf
    refused(lambda: d.freeze_history(3, 2, bad), "call 1 of the window")
    refused(lambda: d.freeze_history(0, 1, min_points=2), "min_points")
    for other, says in ((new_map(history=False), "history"), (new_map(history=True, moments=False), "moments")):
        with pytest.raises(loamx.LoamxError) as e:
            other.freeze_history(0, 1)
        assert e.value.code == loamx.E_INVALID and says in str(e.value)
        assert other.frozen_levels == 0


# ---- 4. the from_history forms ------------------------------------------------------------------------------------------------------
def raw_align(d, cloud, pose, centre, **cfg):
    a = loamx.as_points(cloud)
    c = loamx.cloud_of(a)
    p = np.ascontiguousarray(pose, np.float64).reshape(12)
    ctr = np.ascontiguousarray(centre, np.float32)
    k, out = loamx.AlignConfig(**cfg), loamx.AlignResult()
    assert loamx.lib().loamx_densemap_align(d.h, C.byref(c), p.ctypes.data_as(C.c_void_p), ctr.ctypes.data_as(C.c_void_p), C.byref(k),
                                            C.byref(out)) == loamx.OK
    return out


def raw_align_from_history(d, call, pose, **cfg):
    p = None if pose is None else np.ascontiguousarray(pose, np.float64).reshape(12)
    k, out = loamx.AlignConfig(**cfg), loamx.AlignResult()
    assert loamx.lib().loamx_densemap_align_from_history(d.h, C.c_uint64(call), None if p is None else p.ctypes.data_as(C.c_void_p), C.byref(k),
                                                         C.byref(out)) == loamx.OK
    return out


SIZES = [1, 63, 64, 65, 5000]


@pytest.fixture(scope="module")
def revisits():
    """the box map frozen, and five more logged sweeps of 1, 63, 64, 65 and 5000 points, each a little off the map"""
    S = am.box_scene()
    d = feed(new_map(history=True), S["sweeps"])
    d.freeze_device()
    rng = np.random.default_rng(77)
    offs = []
    for k, n in enumerate(SIZES):
        off = rm.rigid(rng.normal(size=3) * 0.03, rng.uniform(-0.15, 0.15, 3))
        p = am.box_points(rng, n)
        p[:, :3] = (p[:, :3].astype(np.float64) - off[:, 3]) @ off[:, :3]      # off^-1: the alignment should answer `off`
        assert d.add(p, rng.uniform(-1.0, 1.0, 3).astype(np.float32)) == loamx.OK
        offs.append(off)
    assert d.history_size()[0] == 3 + len(SIZES)
    return dict(map=d, offs=offs, starts=[am.box_scene(case=k)["start"] for k in range(3)])


@pytest.mark.parametrize("k", range(len(SIZES)))
def test_align_from_history_equals_the_host_fed_form(revisits, k):
    d, call = revisits["map"], 3 + k
    cloud, origin = d.history(call)
    assert len(cloud) == SIZES[k]
    near = rm.rigid([0.01, -0.02, 0.015], [0.05, -0.04, 0.03])
    for pose, cfg in ((np.eye(3, 4), {}), (near, {}), (near, dict(neighbourhood=0, max_residual=0.3, min_matched=1, max_iterations=5))):
        got, want = raw_align_from_history(d, call, pose, **cfg), raw_align(d, cloud, pose, origin, **cfg)
        assert bytes(got) == bytes(want), (got.as_dict(), want.as_dict())
    # pose NULL: the identity
    assert bytes(raw_align_from_history(d, call, None)) == bytes(raw_align(d, cloud, np.eye(3, 4), origin))
    assert d.align_from_history(call)["pose"].tobytes() == np.float64(raw_align(d, cloud, np.eye(3, 4), origin).pose[:]).tobytes()
    if SIZES[k] == 5000:
        res = d.align_from_history(call, min_matched=200)
        rot, trans = am.pose_error(res["pose"], revisits["offs"][k])
        assert res["status"] == 0 and rot <= 0.01 and trans <= LEAF / 10


@pytest.mark.parametrize("n_poses", [1, 2, 65])
@pytest.mark.parametrize("k", [0, 2, 3, 4])
def test_align_many_from_history_equals_the_host_fed_form(revisits, k, n_poses):
    d, call = revisits["map"], 3 + k
    cloud, origin = d.history(call)
    rng = np.random.default_rng(n_poses)
    poses = np.stack([rm.rigid(rng.normal(size=3) * 0.02, rng.uniform(-0.2, 0.2, 3)) for _ in range(n_poses)])
    if n_poses > 1:
        poses[1, 1, 3] += 50.0      # one that matches nothing and ends at once
    cfg = dict(min_matched=min(50, max(SIZES[k] // 2, 1)), max_iterations=8)
    got, best = d.align_many_from_history(call, poses, raw=True, **cfg)
    want, want_best = d.align_many(cloud, poses, origin, raw=True, **cfg)
    assert bytes(got) == bytes(want) and best == want_best
    if n_poses == 1:
        one, b1 = d.align_many_from_history(call, None, raw=True, **cfg)      # poses None: the identity alone
        ident, b2 = d.align_many(cloud, np.eye(3, 4)[None], origin, raw=True, **cfg)
        assert bytes(one) == bytes(ident) and b1 == b2


def test_align_pyramid_from_history_equals_the_host_fed_form(revisits):
    d = revisits["map"]
    assert d.freeze_pyramid_device(levels=3) and d.frozen_levels == 3
    try:
        for k in (1, 3, 4):
            cloud, origin = d.history(3 + k)
            pose = rm.rigid([0.02, 0.05, -0.03], [0.4, -0.3, 0.2])
            for first in (2, 1, None):
                got = d.align_pyramid_from_history(3 + k, pose, first_level=first, min_matched=1)
                want = d.align_pyramid(cloud, pose, origin, first_level=first, min_matched=1)
                assert len(got) == len(want) == (3 if first is None else first + 1)
                for g, w in zip(got, want):
                    assert g["pose"].tobytes() == w["pose"].tobytes() and g["counts"] == w["counts"]
                    assert (g["iterations"], g["status"], g["degenerate_dims"], g["rms"]) == (w["iterations"], w["status"], w["degenerate_dims"], w["rms"])
        # a selected coarse level is what the single forms read
        d.select_level(1)
        cloud, origin = d.history(7)
        assert bytes(raw_align_from_history(d, 7, None)) == bytes(raw_align(d, cloud, np.eye(3, 4), origin))
    finally:
        d.freeze_device()


def test_from_history_refusals(revisits):
    d, L = revisits["map"], loamx.lib()
    for call, says in ((lambda: d.align_from_history(8), "beyond the log"), (lambda: d.align_many_from_history(99, None), "beyond the log"),
                       (lambda: d.align_pyramid_from_history(8), "beyond the log"), (lambda: d.align_pyramid_from_history(3, first_level=1), "first_level"),
                       (lambda: d.align_from_history(3, np.full((3, 4), np.nan)), "finite"),
                       (lambda: d.align_from_history(3, max_iterations=0), "max_iterations"),
                       (lambda: new_map().align_from_history(0), "history")):
        with pytest.raises(loamx.LoamxError) as e:
            call()
        assert e.value.code == loamx.E_INVALID and says in str(e.value), str(e.value)
    h = feed(new_map(history=True), [(am.box_points(np.random.default_rng(1), 100), (0.0, 0.0, 0.0))])
    with pytest.raises(loamx.LoamxError) as e:
        h.align_from_history(0)
    assert e.value.code == loamx.E_INVALID and "nothing is frozen" in str(e.value)
    out, b, k = (loamx.AlignResult * 2)(), C.c_uint32(7), loamx.AlignConfig()
    assert L.loamx_densemap_align_many_from_history(d.h, C.c_uint64(3), None, C.c_uint32(2), C.byref(k), out, C.byref(b)) == loamx.E_INVALID
    assert "poses_in" in L.loamx_last_error().decode() and b.value == 7 and bytes(out) == bytes(C.sizeof(out))


# ---- 5. a loop closed from the log alone --------------------------------------------------------------------------------------------
def pose34(p6):
    return np.concatenate([synth.rot_zxy(p6[0], p6[1], p6[2]), np.asarray(p6[3:6], np.float64).reshape(3, 1)], axis=1)


def compose(A, B):
    """A o B for 3x4 poses"""
    return np.concatenate([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3]).reshape(3, 1)], axis=1)


def inverse(A):
    return np.concatenate([A[:, :3].T, (-A[:, :3].T @ A[:, 3]).reshape(3, 1)], axis=1)


def in_map(P, cloud):
    out = cloud.copy()
    out[:, :3] = (cloud[:, :3].astype(np.float64) @ P[:, :3].T + P[:, 3]).astype(np.float32)
    return out


def test_a_revisit_verified_from_the_log_alone():
    """Sweeps 0 .. 13 of the hall are registered at their true poses and logged.  The revisit of sweep 10 (a quarter turn and half a
    metre off) arrives as sweep i = 14 with a drifted pose, and is logged with it.  The place database names j; the window
    j - 2 .. j + 2 of the log is frozen, sweep i is aligned where it lies from the seeds of pose_grid, and the relative pose of the two
    keyframes that goes into the pose graph comes out at the truth."""
    sweeps, queries = pm.revisit_case()
    k_rev, dyaw, off = pm.REVISITS[0]
    truth6 = synth.trajectory(40, step=2.5, yaw_step_deg=1.0)
    P = [pose34(truth6[k]) for k in range(14)]
    q6 = truth6[k_rev].copy()
    q6[1] += np.deg2rad(dyaw)
    q6[3] += off
    q6[5] -= off
    P_true = pose34(q6)
    drift = rm.rigid([0.004, 0.03, -0.003], [0.35, 0.05, -0.3], centre=P_true[:, 3])
    P_i = compose(drift, P_true)                 # what the odometry believes
    d = new_map(history=True, initial_slots=1 << 16)
    db = loamx.PlaceDB(exclude_recent=3)
    for k in range(14):
        assert d.add(in_map(P[k], sweeps[k]), P[k][:, 3].astype(np.float32)) == loamx.OK
        db.add(sweeps[k])
    i = 14
    assert d.add(in_map(P_i, queries[0][2]), P_i[:, 3].astype(np.float32)) == loamx.OK
    assert db.add(queries[0][2]) == i
    j, shift = db.query_entry(i, n_results=1)[0][:2]
    assert abs(j - k_rev) <= 1
    w = 2                                        # below exclude_recent: the window cannot contain sweep i
    n = d.freeze_history(j - w, 2 * w + 1)
    assert n > 1000
    o_i = d.history(i)[1]
    hint, step = db.yaw_hint(shift), 2 * np.pi / 60
    seeds = loamx.pose_grid(compose(P[j], inverse(P_i)), centre=o_i, yaws=hint + step * np.arange(-2, 3) / 2,
                            offsets=[(dx, 0.0, dz) for dx in (-1.0, 0.0, 1.0) for dz in (-1.0, 0.0, 1.0)])
    res, best = d.align_many_from_history(i, seeds, max_iterations=30)
    assert best is not None
    # out[best].pose is map <- map about sweep i's origin: the corrected pose of sweep i, and the edge j -> i of the pose graph
    z = loamx.posegraph_between(P[j], compose(res[best]["pose"], P_i)).reshape(3, 4)
    z_true = loamx.posegraph_between(P[j], P_true).reshape(3, 4)
    rot, trans = am.pose_error(z, z_true)
    print(f"loop {j} -> {i}: start {best} of {len(seeds)}, {rot:.2e} rad, {trans:.2e} m, rms {res[best]['rms']:.4f}, counts {res[best]['counts']}")
    assert rot <= 0.01 and trans <= LEAF / 10
    # the drift was real: the logged pose is outside the bars
    rot0, trans0 = am.pose_error(loamx.posegraph_between(P[j], P_i).reshape(3, 4), z_true)
    assert rot0 > 0.01 and trans0 > LEAF / 10
