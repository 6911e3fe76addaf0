"""GPU: the dense map's free-space carving (loamx_densemap_enable_carving ...) against its model (tests/densemap_carve_model.py), byte for
byte — the exported records, the miss counts, the map's and the carving's statistics: host-fed calls of every partial wave / block size,
occupied-wins inside a call, a mover in front of a wall (the filtered export and prune), growth with misses on board, the stride / step
/ range limits, the in-wave combine on and off, the registered clouds of a mapper and of a pipeline, and carving off."""
import ctypes as C

import numpy as np
import pytest

import densemap_carve_model as cm
import densemap_model as dm
from loam_velodyne_amd import loamx, synth

pytestmark = pytest.mark.gpu

LEAF = 0.5


def _pair(carve=None, **kw):
    """a device map and its model, carving enabled with the same settings"""
    carve = carve or {}
    kw.setdefault("leaf", LEAF)
    kw.setdefault("initial_slots", 1024)
    d = loamx.DenseMap(**kw)
    d.enable_carving(**carve)
    mk = {k: v for k, v in kw.items() if k != "initial_slots"}
    m = cm.CarveModel(carve_max_range=carve.get("max_range", 0.0), **{k: v for k, v in carve.items() if k != "max_range"}, **mk)
    return d, m


def _check(d, m, rule=None):
    st, want = d.stats(), m.stats()
    for k, v in want.items():
        assert st[k] == v, (k, st[k], v)
    assert d.carve_stats() == m.carve_stats()
    assert d.points().tobytes() == m.points().tobytes()
    assert d.points("sensor").tobytes() == m.points("sensor").tobytes()
    got = d.misses()
    assert got.dtype == np.uint32 and got.tobytes() == m.misses().tobytes()
    if rule is not None:
        assert d.points(static=loamx.StaticRule(*rule)).tobytes() == m.points(static=rule).tobytes()


def _mixed_cloud(rng, n, origin):
    """random rays around origin with the special cases mixed in (as far as n has room for them)"""
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = np.asarray(origin, np.float32) + rng.uniform(-12, 12, (n, 3)).astype(np.float32)
    o = np.asarray(origin, np.float32)
    special = [o + np.float32([0.01, 0.02, -0.01]),          # in the origin's own cell: no steps
               o + np.float32([0.5, 0.0, 0.0]),              # one step: shorter than the margin
               o + np.float32([6.0, 0.0, 0.0]),              # axis-aligned
               o + np.float32([0.0, 0.0, -7.0]),             # axis-aligned, negative-going
               o + np.float32([-5.0, -4.0, -3.0]),           # negative-going on every axis
               o + np.float32([40.0, 0.0, 0.0]),             # outside the range filter (max_range 30)
               o + np.float32([0.1, 0.05, 0.0]),             # inside min_range 0.3
               np.float32([6.0e5, 0.0, 0.0]),                # outside the key range (and the range filter)
               np.float32([np.nan, 0.0, 0.0])]
    where = rng.permutation(n)[:len(special)]
    for w, s in zip(where, special):
        p[w, :3] = s
    return p


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_host_adds_equal_the_model(n):
    rng = np.random.default_rng(100 + n)
    d, m = _pair(min_range=0.3, max_range=30.0)
    origins = [(-3.3, -1.2, -2.6), (-2.9, -1.1, -2.0), (1.2, 0.4, 0.3)]
    for o in origins:
        p = _mixed_cloud(rng, n, o)
        assert d.add(p, o) == loamx.OK
        assert m.add(p, o)
        _check(d, m, cm.DEFAULT_RULE)
    if n >= 257:
        cs = m.carve_stats()
        assert cs["traced"] > 0 and cs["misses"] > 0 and cs["cells_visited"] > cs["traced"]
        assert m.stats()["dropped_range"] > 0
    d.reset()   # carving stays on, both words cleared
    m2 = cm.CarveModel(leaf=LEAF, min_range=0.3, max_range=30.0)
    p = _mixed_cloud(rng, n, origins[0])
    d.add(p, origins[0])
    m2.add(p, origins[0])
    _check(d, m2)


def _ray_points(cells_x, y=0.25, z=0.25):
    return np.array([[0.25 + LEAF * c, y, z, 0] for c in cells_x], np.float32)


def test_occupied_wins():
    o = (0.25, 0.25, 0.25)
    near, far = _ray_points([2, 3, 5]), _ray_points([9, 12, 12])
    both = np.concatenate([near, far])
    d, m = _pair()
    d.add(both, o)
    m.add(both, o)
    _check(d, m)
    assert int(d.misses().sum()) == 0 and d.carve_stats()["misses"] == 0   # the far rays cross the near cells, hit by the same call
    d, m = _pair()
    for part in (near, far):
        d.add(part, o)
        m.add(part, o)
    _check(d, m)
    # cells 2, 3, 5 are crossed by the three far rays; cell 9, crossed by the two rays to cell 12, was hit by their own call
    assert d.misses().tolist() == [3, 3, 3, 0, 0]
    # the order of the points within a call does not matter
    d2, _ = _pair()
    d2.add(near[::-1], o)
    d2.add(far[::-1], o)
    assert d2.misses().tobytes() == d.misses().tobytes() and d2.carve_stats() == d.carve_stats()


def mover_scene(seed=7):
    """(wall, cluster, origin): a wall at x ~ 10 m seen from the origin, and a small cluster at x ~ 5 m in front of it; with the
    cluster there, the wall points behind it are not seen"""
    rng = np.random.default_rng(seed)
    o = np.float32([0.2, 0.3, 0.25])
    ys, zs = np.meshgrid(np.arange(-3.0, 3.0, 0.25), np.arange(-1.0, 2.0, 0.25))
    wall = np.zeros((ys.size, 4), np.float32)
    wall[:, 0] = 10.2 + rng.uniform(0, 0.1, ys.size)
    wall[:, 1] = ys.ravel() + rng.uniform(0, 0.05, ys.size)
    wall[:, 2] = zs.ravel() + rng.uniform(0, 0.05, ys.size)
    cy, cz = np.meshgrid(np.arange(-0.4, 0.6, 0.5), np.arange(0.1, 1.1, 0.5))
    cluster = np.zeros((cy.size, 4), np.float32)
    cluster[:, 0] = 5.2
    cluster[:, 1] = cy.ravel()
    cluster[:, 2] = cz.ravel()
    # the wall points whose ray passes the cluster's box at x = 5.2 are shadowed while it stands there
    t = (5.2 - o[0]) / (wall[:, 0] - o[0])
    hy, hz = o[1] + t * (wall[:, 1] - o[1]), o[2] + t * (wall[:, 2] - o[2])
    shadowed = (hy > -0.65) & (hy < 0.35) & (hz > -0.15) & (hz < 0.85)
    return wall, cluster, shadowed, o


def mover_calls():
    wall, cluster, shadowed, o = mover_scene()
    with_mover = np.concatenate([wall[~shadowed], cluster])
    return [with_mover] * 2 + [wall] * 5, wall, cluster, o


def test_a_mover_is_dropped_and_the_wall_kept():
    calls, wall, cluster, o = mover_calls()
    d, m = _pair()
    for p in calls:
        d.add(p, o)
        m.add(p, o)
    _check(d, m, cm.DEFAULT_RULE)
    # the model alone: exactly the cluster's voxels are dynamic, every wall voxel stays
    wall_keys = set(dm.keys_of(wall, o, LEAF)[0].tolist())
    cluster_keys = set(dm.keys_of(cluster, o, LEAF)[0].tolist())
    assert len(cluster_keys) == 4 and not wall_keys & cluster_keys
    assert set(m.keys[m.dynamic_mask()].tolist()) == cluster_keys
    rule = loamx.StaticRule()
    static = d.points(static=rule)
    assert len(static) == len(d) - len(cluster_keys) == len(wall_keys)
    assert static.tobytes() == m.points(static=cm.DEFAULT_RULE).tobytes()
    assert d.prune(rule) == len(cluster_keys) == m.prune()
    assert d.points().tobytes() == static.tobytes()
    _check(d, m, cm.DEFAULT_RULE)
    assert d.prune(rule) == 0
    # the map goes on as before
    for p in (calls[0], calls[-1]):
        d.add(p, o)
        m.add(p, o)
        _check(d, m, cm.DEFAULT_RULE)


def test_growth_with_misses_on_board():
    rng = np.random.default_rng(21)
    o = (0.1, 0.2, 0.3)
    d, m = _pair()
    calls = [np.concatenate([rng.uniform(-9, 9, (220, 3)), np.zeros((220, 1))], axis=1).astype(np.float32) for _ in range(4)]
    for p in calls[:2]:
        d.add(p, o)
        m.add(p, o)
    assert d.rehashes == 0 and 0 < len(m) <= 512
    before = d.misses()
    assert before.tobytes() == m.misses().tobytes() and int(before.sum()) > 0
    keys_before = m.keys.copy()
    for p in calls[2:]:
        d.add(p, o)
        m.add(p, o)
    assert len(m) > 512 and d.rehashes >= 1
    _check(d, m, cm.DEFAULT_RULE)
    # the misses of the voxels from before the rehash travelled with them (and only grew)
    after = d.misses()[np.isin(m.keys, keys_before)]
    assert np.all(after >= before)
    # a rehash alone changes nothing: the same calls into a table that never grows
    big = loamx.DenseMap(leaf=LEAF, initial_slots=1 << 14)
    big.enable_carving()
    for p in calls:
        big.add(p, o)
    assert big.rehashes == 0
    assert big.misses().tobytes() == d.misses().tobytes() and big.points().tobytes() == d.points().tobytes()


def test_limits_show_in_their_own_statistics():
    o = (0.25, 0.25, 0.25)
    pts = _ray_points(range(1, 11))
    d, m = _pair(dict(ray_stride=3))
    d.add(pts, o)
    m.add(pts, o)
    _check(d, m)
    assert d.carve_stats()["traced"] == 4 and d.carve_stats()["skipped_stride"] == 6
    # n_steps == max_steps is traced, max_steps + 1 is not
    d, m = _pair(dict(max_steps=7))
    p = _ray_points([7, 8])
    d.add(p, o)
    m.add(p, o)
    _check(d, m)
    cs = d.carve_stats()
    assert (cs["traced"], cs["skipped_steps"], cs["cells_visited"]) == (1, 1, 6)
    # max_range on the boundary square: d2 == max_range^2 is traced, the next f32 above is not
    far = np.array([[0.25 + 4.0, 0.25, 0.25, 0], [0.25, 0.25, 0.25 + np.nextafter(np.float32(4.0), np.float32(5.0)), 0]], np.float32)
    d, m = _pair(dict(max_range=4.0))
    d.add(far, o)
    m.add(far, o)
    _check(d, m)
    cs = d.carve_stats()
    assert (cs["traced"], cs["skipped_range"]) == (1, 1)
    # an origin outside the key range: its points are added, no ray is traced
    d, m = _pair()
    oo = (0.6e6, 0.0, 0.0)
    d.add(pts, oo)
    m.add(pts, oo)
    _check(d, m)
    assert d.carve_stats()["skipped_steps"] == 10 and d.stats()["added"] == 10
    # a stride larger than a block's worth of rays, over more than one block
    rng = np.random.default_rng(3)
    p = np.concatenate([rng.uniform(-8, 8, (700, 3)), np.zeros((700, 1))], axis=1).astype(np.float32)
    d, m = _pair(dict(ray_stride=2))
    for _ in range(2):
        d.add(p, o)
        m.add(p, o)
    _check(d, m)


def test_combine_on_and_off():
    calls, _, _, o = mover_calls()
    a, m = _pair()
    b, _ = _pair()
    b.set_combine(False)
    for p in calls[:4]:
        a.add(p, o)
        b.add(p, o)
        m.add(p, o)
    _check(a, m)
    _check(b, m)


def test_from_mapper():
    n = 3
    w = synth.World(half_extent=65.0)
    cmap, smap = w.make_map(60_000)
    poses = synth.trajectory(n)
    sweeps = [synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=900 + t, az_steps=900) for t in range(n)]
    sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
    mp.load_cubes(cmap, smap)
    d, m = _pair(dict(ray_stride=8, max_range=40.0), initial_slots=1 << 14)
    for sw in sweeps:
        f = sr.process(sw.points.copy(), sw.ring_sizes)
        od.process(f)
        lc, ls = od.last_clouds()
        full = od.transform_to_end(f["full"])
        mp.update_odometry(od.transform_sum)
        rc, reg = mp.process(lc, ls, full)
        assert d.add_from(mp) == loamx.OK
        m.add(reg, mp.transform("aft")[3:])
    assert m.carve_stats()["traced"] > 1000 and m.carve_stats()["misses"] > 0
    _check(d, m, cm.DEFAULT_RULE)


def test_from_pipeline():
    ns, T = 2, 4
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
    pairs = [_pair(dict(ray_stride=8, max_range=40.0), initial_slots=1 << 14) for _ in range(ns)]
    registered = 0
    for t in range(T):
        if p.step(t) == loamx.OK:
            for k, (d, m) in enumerate(pairs):
                assert d.add_from_pipeline(p, k) == loamx.OK
                m.add(p.download_full_res(k, len(sweeps[t][k][0])), p.get(k)[2][3:])
            registered += 1
    assert registered >= 2
    for d, m in pairs:
        assert m.carve_stats()["traced"] > 500
        _check(d, m, cm.DEFAULT_RULE)


def test_carving_off():
    L = loamx.lib()
    o = (0.25, 0.25, 0.25)
    d = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
    plain = dm.Model(leaf=LEAF)
    p = _ray_points(range(1, 11))
    d.add(p, o)
    plain.add(p, o)
    for call in (d.carve_stats, d.misses, d.prune, lambda: d.points(static=loamx.StaticRule())):
        with pytest.raises(loamx.LoamxError) as e:
            call()
        assert e.value.code == loamx.E_INVALID and "carving is not enabled" in str(e.value)
    with pytest.raises(loamx.LoamxError):
        d.save_pcd("unused.pcd", static=loamx.StaticRule())
    # enabling on a map that is not empty is refused, and nothing changes
    before = (d.stats(), d.points().tobytes())
    with pytest.raises(loamx.LoamxError) as e:
        d.enable_carving()
    assert e.value.code == loamx.E_INVALID
    assert (d.stats(), d.points().tobytes()) == before
    with pytest.raises(loamx.LoamxError):
        d.carve_stats()   # still off
    d.add(p, o)
    plain.add(p, o)
    assert d.points().tobytes() == plain.points().tobytes()
    # after a reset the map is empty again: allowed, and the map carves from here on
    d.reset()
    d.enable_carving()
    m = cm.CarveModel(leaf=LEAF)
    for _ in range(2):
        d.add(p, o)
        m.add(p, o)
    _check(d, m)
    # bad settings and a bad rule
    e2 = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
    for bad in (dict(ray_stride=0), dict(max_steps=0), dict(max_steps=65537), dict(max_range=-1.0)):
        with pytest.raises(loamx.LoamxError):
            e2.enable_carving(**bad)
    e2.enable_carving(max_steps=65536)
    with pytest.raises(loamx.LoamxError):
        e2.prune(loamx.StaticRule(den=0))
    # the capacity answer of download_misses
    n = C.c_uint64(0)
    assert L.loamx_densemap_download_misses(d.h, None, C.c_uint64(0), C.byref(n)) == loamx.E_CAPACITY
    assert n.value == len(m)


def test_save_pcd_static(tmp_path):
    calls, _, _, o = mover_calls()
    d, m = _pair()
    for p in calls:
        d.add(p, o)
    rule = loamx.StaticRule()
    for axes in ("loam", "sensor"):
        path = str(tmp_path / f"static_{axes}.pcd")
        d.save_pcd(path, axes=axes, static=rule)
        hdr, body = dm.read_pcd(path)
        assert int(hdr["POINTS"]) == len(d) - 4
        assert body.tobytes() == d.points(axes, static=rule).tobytes()
