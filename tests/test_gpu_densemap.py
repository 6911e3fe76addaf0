"""GPU: the dense global map (loamx_densemap_*) against its numpy model (tests/densemap_model.py), byte for byte — host-fed clouds, the
order of the points and of the calls, growth of the table and the capacity rule, the registered clouds of a LaserMapping chain (host
messages and linked) and of a Pipeline, the PCD export — and the mapper's / pipeline's own results unchanged by a dense map attached."""
import numpy as np
import pytest

import densemap_model as dm
from loam_velodyne_amd import loamx, synth

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(d, m):
    st = d.stats()
    want = m.stats()
    for k, v in want.items():
        assert st[k] == v, (k, st[k], v)
    assert len(d) == len(m)
    assert _same(d.points(), m.points())
    assert _same(d.points("sensor"), m.points("sensor"))


def _away_from(points, origin, radii, margin=1e-2):
    """the points whose distance to origin is not within margin of any of radii (the range filter's boundaries)"""
    r = np.sqrt(((points[:, :3].astype(np.float64) - np.asarray(origin, np.float64)) ** 2).sum(1))
    keep = np.ones(len(points), bool)
    for x in radii:
        if x > 0:
            keep &= np.abs(r - x) > margin
    return points[keep]


def _host_clouds(n_sweeps=4, seed=0):
    w = synth.World(half_extent=45.0)
    poses = synth.trajectory(n_sweeps, start=(0.5, 0.0, 1.0))
    out = []
    for t in range(n_sweeps):
        sw = synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=seed + t, az_steps=900)
        p = np.ascontiguousarray(sw.points, np.float32).copy()
        origin = np.asarray(poses[t + 1][3:6], np.float32)
        p[:, :3] += origin   # (a map-frame cloud around a moving sensor)
        out.append((p, origin))
    return out


@pytest.mark.parametrize("rng", [(0.0, 0.0), (2.0, 30.0)])
def test_host_adds_equal_the_model(rng):
    mn, mx = rng
    clouds = [(_away_from(p, o, (mn, mx)), o) for p, o in _host_clouds()]
    d = loamx.DenseMap(leaf=0.1, min_range=mn, max_range=mx)
    m = dm.Model(leaf=0.1, min_range=mn, max_range=mx)
    for p, o in clouds:
        assert d.add(p, o) == loamx.OK
        assert m.add(p, o)
        _check(d, m)
    st = d.stats()
    assert st["voxels"] > 1000 and st["added"] > 0
    if mx > 0:
        assert st["dropped_range"] > 0
    else:
        assert st["dropped_range"] == 0
    # PCL layout in, another leaf
    d2, m2 = loamx.DenseMap(leaf=0.25), dm.Model(leaf=0.25)
    for p, o in clouds[:2]:
        d2.add(loamx.to_pcl_layout(p), o)
        m2.add(p, o)
    _check(d2, m2)
    d.reset()
    assert len(d) == 0 and d.stats()["offered"] == 0 and d.points().shape == (0, 4)


def test_order_and_call_boundaries_do_not_matter():
    clouds = _host_clouds(3, seed=40)
    a = loamx.DenseMap(leaf=0.1)
    b = loamx.DenseMap(leaf=0.1)
    c = loamx.DenseMap(leaf=0.1)
    rng = np.random.default_rng(5)
    for p, o in clouds:
        a.add(p, o)
        c.add(p, o)
        q = p[rng.permutation(len(p))]
        cut = sorted(rng.choice(np.arange(1, len(q)), 3, replace=False))
        for part in np.split(q, cut):
            b.add(part, o)
    pa, pb, pc = a.points(), b.points(), c.points()
    assert pa.tobytes() == pb.tobytes() == pc.tobytes()
    sa, sb = a.stats(), b.stats()
    assert sa["voxels"] == sb["voxels"] and sa["added"] == sb["added"]
    # the in-wave combine of equal keys is an optimisation only
    e = loamx.DenseMap(leaf=0.1)
    e.set_combine(False)
    for p, o in clouds:
        e.add(p, o)
    assert e.points().tobytes() == pa.tobytes()


def test_growth_capacity_and_key_range():
    rng = np.random.default_rng(11)
    leaf = 0.1
    calls = [rng.uniform(-200, 200, (3000, 4)).astype(np.float32) for _ in range(5)]   # (nearly every point a voxel of its own)
    # points beyond the key range (|i| >= 2^20 at leaf 0.1: |x| >= 104857.6 m) in the second call
    calls[1][:7, 0] = np.float32(2.0e5)
    calls[1][7:10, 2] = np.float32(-1.2e5)
    d = loamx.DenseMap(leaf=leaf, initial_slots=1 << 10)
    m = dm.Model(leaf=leaf)
    for p in calls:
        d.add(p, (0, 0, 0))
        m.add(p, (0, 0, 0))
    assert d.rehashes >= 3, d.rehashes
    assert d.stats()["slots"] >= 2 * len(m)
    assert m.stats()["dropped_key"] == 10
    _check(d, m)
    # the capacity rule: the first add with voxels_now + points > max_voxels is refused and changes nothing
    cap = 7000
    d = loamx.DenseMap(leaf=leaf, initial_slots=1 << 10, max_voxels=cap)
    m = dm.Model(leaf=leaf, max_voxels=cap)
    refused = None
    for k, p in enumerate(calls):
        if m.would_refuse(len(p)):
            refused = k
            before = (d.stats(), d.points())
            with pytest.raises(loamx.LoamxError) as e:
                d.add(p, (0, 0, 0))
            assert e.value.code == loamx.E_CAPACITY
            assert not m.add(p, (0, 0, 0))
            assert d.stats() == before[0] and d.points().tobytes() == before[1].tobytes()
            break
        assert d.add(p, (0, 0, 0)) == loamx.OK
        assert m.add(p, (0, 0, 0))
    assert refused == 2, refused   # (3000 + 2990 voxels, then 5990 + 3000 > 7000)
    _check(d, m)
    d.add(calls[0][:100], (0, 0, 0))   # a smaller add still fits
    m.add(calls[0][:100], (0, 0, 0))
    _check(d, m)


def _mapper_chain(n, seed=900):
    w = synth.World(half_extent=65.0)
    cm, sm = w.make_map(60_000)
    poses = synth.trajectory(n)
    sweeps = [synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=seed + t) for t in range(n)]
    return cm, sm, sweeps


def test_from_mapper_host_messages_and_linked():
    n = 8
    cm, sm, sweeps = _mapper_chain(n)

    def host_chain(dense):
        sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
        mp.load_cubes(cm, sm)
        model, out = dm.Model(leaf=0.1), []
        for sw in sweeps:
            f = sr.process(sw.points.copy(), sw.ring_sizes)
            od.process(f)
            lc, ls = od.last_clouds()
            full = od.transform_to_end(f["full"])
            mp.update_odometry(od.transform_sum)
            rc, reg = mp.process(lc, ls, full)
            if dense is not None:
                assert dense.add_from(mp) == loamx.OK
                model.add(reg, mp.transform("aft")[3:])
            out.append((rc, [mp.transform(w) for w in ("aft", "bef", "tobe", "sum")], reg))
        # no registered cloud asked for: nothing to add
        if dense is not None:
            f = sr.process(sweeps[0].points.copy(), sweeps[0].ring_sizes)
            od.process(f)
            lc, ls = od.last_clouds()
            mp.update_odometry(od.transform_sum)
            mp.process(lc, ls)
            assert dense.add_from(mp) == loamx.SKIPPED
        return model, out

    d = loamx.DenseMap(leaf=0.1)
    model, with_dense = host_chain(d)
    _, without = host_chain(None)
    for (rca, ta, rega), (rcb, tb, regb) in zip(with_dense, without):
        assert rca == rcb and all(np.array_equal(x, y) for x, y in zip(ta, tb)) and _same(rega, regb)
    assert len(model) > 1000
    _check(d, model)

    # the linked chain: the registered cloud never leaves the device before the add
    sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
    mp.load_cubes(cm, sm)
    landing = np.zeros((max(len(s.points) for s in sweeps), 4), np.float32)
    dl = loamx.DenseMap(leaf=0.1, min_range=1.0)
    ml = dm.Model(leaf=0.1, min_range=1.0)
    dn = loamx.DenseMap(leaf=0.1)   # fed without a landing area for the registered cloud
    for t, sw in enumerate(sweeps):
        sr.process_linked(sw.points.copy(), sw.ring_sizes)
        od.process_linked(sr)
        rc, reg = mp.process_linked(od, landing)
        assert dl.add_from(mp) == loamx.OK
        assert dn.add_from(mp) == loamx.OK
        ml.add(reg, mp.transform("aft")[3:])   # (f32 on both sides, the same operations: exact at the boundary too)
        assert all(np.array_equal(a, b) for a, b in zip([mp.transform(w) for w in ("aft", "bef", "tobe", "sum")], with_dense[t][1]))
    _check(dl, ml)
    assert dn.points().tobytes() == d.points().tobytes()   # (the linked chain registers the same clouds)


def test_from_pipeline():
    ns, T = 4, 5
    w = synth.World(half_extent=45.0)
    cm, sm = w.make_map(60_000)
    sweeps, starts = [[None] * ns for _ in range(T)], []
    for s in range(ns):
        poses = synth.trajectory(T, start=(1.5 * s, 0.0, 2.0 * s))
        starts.append(np.array([0, 0, 0, 1.5 * s, 0, 2.0 * s], np.float32))
        for t in range(T):
            sw = synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=30 * s + t, az_steps=900)
            sweeps[t][s] = (np.ascontiguousarray(sw.points, np.float32), sw.ring_sizes)

    def run(dense):
        p = loamx.Pipeline(ns)
        p.set_frozen(cm, sm)
        for s in range(ns):
            p.set_state(s, aft=starts[s])
        p.upload(sweeps)
        models = [dm.Model(leaf=0.1) for _ in range(ns)]
        out, registered = [], 0
        for t in range(T):
            rc = p.step(t)
            if dense is not None:
                if rc == loamx.OK:
                    for k in range(ns):
                        assert dense[k].add_from_pipeline(p, k) == loamx.OK
                        models[k].add(p.download_full_res(k, len(sweeps[t][k][0])), p.get(k)[2][3:])
                    registered += 1
                else:
                    assert dense[0].add_from_pipeline(p, 0) == loamx.SKIPPED
            out.append((rc, [p.get(s) for s in range(ns)]))
        return models, out, registered

    dense = [loamx.DenseMap(leaf=0.1) for _ in range(ns)]
    models, a, registered = run(dense)
    _, b, _ = run(None)
    assert registered >= 2
    for (rca, ga), (rcb, gb) in zip(a, b):
        assert rca == rcb
        for (tra, tsa, afa, sta), (trb, tsb, afb, stb) in zip(ga, gb):
            assert np.array_equal(tra, trb) and np.array_equal(tsa, tsb) and np.array_equal(afa, afb) and sta == stb
    for k in range(ns):
        assert len(models[k]) > 1000
        _check(dense[k], models[k])


def test_save_pcd_equals_points(tmp_path):
    d = loamx.DenseMap(leaf=0.2)
    for p, o in _host_clouds(2, seed=70):
        d.add(p, o)
    for axes in ("loam", "sensor"):
        path = str(tmp_path / f"map_{axes}.pcd")
        d.save_pcd(path, axes=axes)
        hdr, body = dm.read_pcd(path)
        assert hdr["FIELDS"] == "x y z intensity" and hdr["DATA"] == "binary" and int(hdr["POINTS"]) == len(d)
        assert body.tobytes() == d.points(axes).tobytes()
