"""GPU: the place-recognition database (loamx_place_*) against its numpy model (tests/place_model.py), byte for byte — descriptors and ring
keys of host clouds, queries (exhaustive and with the ring-key pre-selection) on the revisit cases tests/test_place_cpu.py solves with
the model alone, growth / capacity / reset / save and load, the registered clouds of a LaserMapping chain (host messages and linked) and
of a Pipeline, adds from several sources into one database — and the mapper's / pipeline's own results unchanged by a database attached."""
import numpy as np
import pytest

import place_model as pm
from test_place_cpu import HAND, HAND_CLOUD
from loam_velodyne_amd import loamx, synth

pytestmark = pytest.mark.gpu
F = np.float32


def _bits(x):
    return np.asarray(x, F).tobytes()


def _same_entry(db, i, D, k):
    d, key = db.descriptor(i)
    assert d.shape == D.shape
    bad = np.nonzero(d.view(np.uint32) != np.asarray(D, F).view(np.uint32))
    assert d.tobytes() == np.asarray(D, F).tobytes(), (i, len(bad[0]), list(zip(*bad))[:4], d[bad][:4], D[bad][:4])
    assert key.tobytes() == np.asarray(k, F).tobytes(), (i, key, k)


def _same_matches(got, want):
    assert [(g[0], g[1]) for g in got] == [(w[0], w[1]) for w in want], (got, want)
    assert _bits([g[2] for g in got]) == _bits([w[2] for w in want]), (got, want)
    assert _bits([g[3] for g in got]) == _bits([w[3] for w in want]), (got, want)


def _sweep(sensor, az, seed=0, pose=None):
    w = synth.World(half_extent=45.0)
    pose = np.zeros(6) if pose is None else np.asarray(pose, np.float64)
    return np.ascontiguousarray(synth.make_sweep(w, sensor, pose, pose, seed=seed, az_steps=az).points, F)


def _pair(**cfg):
    """a device database and its model with the same configuration"""
    names = dict(n_rings="R", n_sectors="S")
    return loamx.PlaceDB(**cfg), pm.Model(**{names.get(k, k): v for k, v in cfg.items() if k != "initial_entries"})


@pytest.mark.parametrize("cfg", [dict(), dict(min_range=3.0, max_range=30.0), dict(n_rings=32, n_sectors=64), dict(n_rings=8, n_sectors=12),
                                 dict(n_rings=64, n_sectors=128, max_range=50.0, height_offset=2.5), dict(n_rings=1, n_sectors=5)])
def test_descriptors_of_host_clouds(cfg):
    db, m = _pair(**cfg)
    vlp, hdl = _sweep("VLP-16", 900, seed=1), _sweep("HDL-64E", 1024, seed=2)
    rng = np.random.default_rng(4)
    origin = np.array([1.25, -0.3, -2.5], F)
    moved = hdl.copy()
    moved[:, :3] += origin
    cases = [(vlp, (0, 0, 0)), (hdl, (0, 0, 0)), (loamx.to_pcl_layout(vlp), (0, 0, 0)), (moved, origin),
             (np.zeros((0, 4), F), (0, 0, 0)), (vlp[rng.permutation(len(vlp))], (0, 0, 0)), (vlp[:1], (0, 0, 0)), (hdl[:1025], (0.5, 0, 0))]
    for i, (p, o) in enumerate(cases):
        assert db.add(p, o) == i == m.add(p, o)
    assert len(db) == len(cases)
    for i in range(len(cases)):
        _same_entry(db, i, m.desc[i], m.keys[i])
    assert not db.descriptor(4)[0].any() and not db.descriptor(4)[1].any()     # the empty cloud: an all-zero entry
    assert db.descriptor(5)[0].tobytes() == db.descriptor(0)[0].tobytes()      # the same cloud shuffled: the same bytes
    assert db.descriptor(2)[0].tobytes() == db.descriptor(0)[0].tobytes()      # PCL-layout records
    assert (db.descriptor(1)[0] > 0).sum() > min(100, m.R * m.S // 4)


def test_hand_cloud_and_boundaries():
    db = loamx.PlaceDB(n_rings=HAND["R"], n_sectors=HAND["S"], max_range=HAND["max_range"], height_offset=HAND["height_offset"])
    db.add(HAND_CLOUD)
    want = np.zeros((4, 8), F)
    want[0, 0], want[0, 2], want[1, 0], want[2, 4], want[2, 7], want[3, 0] = 2, 3, 6, 2, 1, 5
    _same_entry(db, 0, want, pm.ring_key(want))
    with pytest.raises(loamx.LoamxError) as e:
        db.add(HAND_CLOUD, (np.nan, 0, 0))
    assert e.value.code == loamx.E_INVALID and len(db) == 1
    with pytest.raises(loamx.LoamxError):
        db.descriptor(1)
    with pytest.raises(loamx.LoamxError):
        db.query(HAND_CLOUD, n_results=loamx.PLACE_MAX_RESULTS + 1)


@pytest.fixture(scope="module")
def revisit():
    return pm.revisit_case()


@pytest.mark.parametrize("K", [0, 10])
def test_revisit_queries(revisit, K):
    sweeps, queries = revisit
    db, m = _pair(n_candidates=K, exclude_recent=12)
    ex = pm.Model(n_candidates=0, exclude_recent=12)
    for p in sweeps:
        assert db.add(p) == m.add(p)
        ex.add(p)
    for i in (0, 17, 39):
        _same_entry(db, i, m.desc[i], m.keys[i])
    for k, dyaw, q in queries:
        got = db.query(q, n_results=5)
        want = m.query(q, n_results=5)
        print(f"revisit K={K} k={k} dyaw={dyaw}: device {got[:2]}")
        assert len(got) == 5
        _same_matches(got, want)
        if K:    # the pre-selected search is the exhaustive one restricted to the model's candidate set
            _, rk = m.describe(q)
            ids, _ = m.candidates(rk, len(m), 0)
            assert len(ids) == K
            _same_matches(got, ex.query(q, n_results=5, only=ids))
        # the expectations of tests/test_place_cpu.py hold on the device
        want_shift = int(round(dyaw / 360.0 * 60)) % 60
        assert got[0][0] == k and min((got[0][1] - want_shift) % 60, (want_shift - got[0][1]) % 60) <= 1
        assert got[1][2] - got[0][2] >= 0.05
        assert abs(db.yaw_hint(got[0][1]) - np.deg2rad(dyaw % 360.0)) <= 2 * np.pi / 60 + 1e-6
        # exclude_recent of a query that is not stored: the ids below 40 - 20
        _same_matches(db.query(q, exclude_recent=20, n_results=3), m.query(q, exclude_recent=20, n_results=3))
    # stored entries: the configuration's exclude_recent (12)
    for q in (39, 20, 13, 12, 5):
        got = db.query_entry(q, n_results=4)
        _same_matches(got, m.query_entry(q, n_results=4))
        assert all(g[0] + 12 < q for g in got) and len(got) == min(4, max(q - 12, 0))
    assert len(db.query_entry(39, n_results=64)) == (27 if K == 0 else 10)


def test_growth_capacity_reset_save_load(tmp_path):
    rng = np.random.default_rng(21)

    def cloud():
        n = int(rng.integers(5, 60))
        return np.concatenate([rng.uniform(-70, 70, (n, 1)), rng.uniform(-1.5, 8, (n, 1)), rng.uniform(-70, 70, (n, 1)), np.zeros((n, 1))], 1).astype(F)

    db, m = _pair(exclude_recent=0, initial_entries=1024)
    dk, mk = _pair(exclude_recent=0, n_candidates=50, initial_entries=1024)
    probe = [cloud() for _ in range(2)]

    def check(n_results=6):
        for q in probe:
            _same_matches(db.query(q, n_results=n_results), m.query(q, n_results=n_results))
            _same_matches(dk.query(q, n_results=n_results), mk.query(q, n_results=n_results))
        _same_matches(db.query_entry(len(m) - 1, n_results=3), m.query_entry(len(m) - 1, n_results=3))

    for target in (1000, 1500, 2100):     # 1024 -> 2048 -> 4096: a power-of-two boundary is crossed before the second and the third check
        while len(m) < target:
            c = cloud()
            assert db.add(c) == m.add(c)
            assert dk.add(c) == mk.add(c)
        check()
    assert db.growths == 2 and dk.growths == 2 and len(db) == 2100
    for i in (0, 1023, 1024, 2047, 2048, 2099):
        _same_entry(db, i, m.desc[i], m.keys[i])

    # save / load into a fresh handle: identical answers
    path = str(tmp_path / "places.lxpl")
    db.save(path)
    fresh = loamx.PlaceDB(exclude_recent=0, initial_entries=64)
    fresh.load(path)
    assert len(fresh) == len(db)
    for q in probe:
        a, b = db.query(q, n_results=8), fresh.query(q, n_results=8)
        _same_matches(a, b)
    for i in (0, 1700, 2099):
        assert fresh.descriptor(i)[0].tobytes() == db.descriptor(i)[0].tobytes() and fresh.descriptor(i)[1].tobytes() == db.descriptor(i)[1].tobytes()
    other = loamx.PlaceDB(n_rings=10)
    with pytest.raises(loamx.LoamxError) as e:
        other.load(path)
    assert e.value.code == loamx.E_INVALID and len(other) == 0
    with pytest.raises(loamx.LoamxError):
        fresh.load(str(tmp_path / "missing.lxpl"))
    assert len(fresh) == len(db)
    # the loaded handle goes on like the saved one
    c = cloud()
    assert fresh.add(c) == db.add(c) == m.add(c)
    _same_matches(fresh.query_entry(2100, n_results=5), m.query_entry(2100, n_results=5))

    # reset
    db.reset()
    assert len(db) == 0 and db.query(probe[0]) == []
    m.reset()
    assert db.add(probe[1]) == 0 == m.add(probe[1])
    _same_matches(db.query(probe[1], n_results=5), m.query(probe[1], n_results=5))

    # max_entries: the add that would pass it is refused and changes nothing
    cap, mc = _pair(exclude_recent=0, max_entries=3)
    for i in range(3):
        assert cap.add(probe[i % 2]) == i == mc.add(probe[i % 2])
    before = cap.query(probe[0], n_results=5)
    with pytest.raises(loamx.LoamxError) as e:
        cap.add(probe[0])
    assert e.value.code == loamx.E_CAPACITY and mc.add(probe[0]) is None
    assert len(cap) == 3
    _same_matches(cap.query(probe[0], n_results=5), before)
    _same_matches(before, mc.query(probe[0], n_results=5))


def _mapper_chain(n, seed=900):
    w = synth.World(half_extent=65.0)
    cm, sm = w.make_map(60_000)
    poses = synth.trajectory(n)
    sweeps = [synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=seed + t) for t in range(n)]
    return cm, sm, sweeps


def test_from_mapper_host_messages_and_linked():
    n = 8
    cm, sm, sweeps = _mapper_chain(n)

    def host_chain(db):
        sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
        mp.load_cubes(cm, sm)
        model, out = pm.Model(exclude_recent=2), []
        # no registered cloud asked for: nothing to add, no entry
        if db is not None:
            f = sr.process(sweeps[0].points.copy(), sweeps[0].ring_sizes)
            od.process(f)
            lc, ls = od.last_clouds()
            mp.update_odometry(od.transform_sum)
            mp.process(lc, ls)
            assert db.add_from(mp) is None and len(db) == 0
            sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
            mp.load_cubes(cm, sm)
        for sw in sweeps:
            f = sr.process(sw.points.copy(), sw.ring_sizes)
            od.process(f)
            lc, ls = od.last_clouds()
            full = od.transform_to_end(f["full"])
            mp.update_odometry(od.transform_sum)
            rc, reg = mp.process(lc, ls, full)
            if db is not None:
                assert db.add_from(mp) == model.add(reg, mp.transform("aft")[3:])
            out.append((rc, [mp.transform(w) for w in ("aft", "bef", "tobe", "sum")], reg))
        return model, out

    db = loamx.PlaceDB(exclude_recent=2)
    model, with_db = host_chain(db)
    _, without = host_chain(None)
    for (rca, ta, rega), (rcb, tb, regb) in zip(with_db, without):
        assert rca == rcb and all(np.array_equal(x, y) for x, y in zip(ta, tb)) and rega.tobytes() == regb.tobytes()
    assert len(db) == n
    for i in range(n):
        _same_entry(db, i, model.desc[i], model.keys[i])
        assert (model.desc[i] > 0).sum() > 50
    _same_matches(db.query_entry(n - 1, n_results=5), model.query_entry(n - 1, n_results=5))

    # the linked chain: the registered cloud never leaves the device before the add
    sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
    mp.load_cubes(cm, sm)
    landing = np.zeros((max(len(s.points) for s in sweeps), 4), F)
    dl, ml = _pair(exclude_recent=2, min_range=1.0)
    dn = loamx.PlaceDB(exclude_recent=2)   # fed without a landing area for the registered cloud
    for t, sw in enumerate(sweeps):
        sr.process_linked(sw.points.copy(), sw.ring_sizes)
        od.process_linked(sr)
        rc, reg = mp.process_linked(od, landing)
        assert dl.add_from(mp) == t == ml.add(reg, mp.transform("aft")[3:])
        assert dn.add_from(mp) == t
        assert all(np.array_equal(a, b) for a, b in zip([mp.transform(w) for w in ("aft", "bef", "tobe", "sum")], with_db[t][1]))
    for i in range(n):
        _same_entry(dl, i, ml.desc[i], ml.keys[i])
        assert dn.descriptor(i)[0].tobytes() == db.descriptor(i)[0].tobytes()   # (the linked chain registers the same clouds)
    _same_matches(dl.query_entry(n - 1, n_results=5), ml.query_entry(n - 1, n_results=5))


def _pipeline_case(ns, T):
    w = synth.World(half_extent=45.0)
    cm, sm = w.make_map(60_000)
    sweeps, starts = [[None] * ns for _ in range(T)], []
    for s in range(ns):
        poses = synth.trajectory(T, start=(1.5 * s, 0.0, 2.0 * s))
        starts.append(np.array([0, 0, 0, 1.5 * s, 0, 2.0 * s], F))
        for t in range(T):
            sw = synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=30 * s + t, az_steps=900)
            sweeps[t][s] = (np.ascontiguousarray(sw.points, F), sw.ring_sizes)
    return cm, sm, sweeps, starts


def test_from_pipeline():
    ns, T = 2, 5
    cm, sm, sweeps, starts = _pipeline_case(ns, T)

    def run(dbs):
        p = loamx.Pipeline(ns)
        p.set_frozen(cm, sm)
        for s in range(ns):
            p.set_state(s, aft=starts[s])
        p.upload(sweeps)
        models = [pm.Model(exclude_recent=0) for _ in range(ns)]
        out, registered = [], 0
        for t in range(T):
            rc = p.step(t)
            if dbs is not None:
                if rc == loamx.OK:
                    for k in range(ns):
                        want = models[k].add(p.download_full_res(k, len(sweeps[t][k][0])), p.get(k)[2][3:])
                        assert dbs[k].add_from_pipeline(p, k) == want
                    registered += 1
                else:
                    assert dbs[0].add_from_pipeline(p, 0) is None and len(dbs[0]) == 0
            out.append((rc, [p.get(s) for s in range(ns)], [p.download_full_res(k, len(sweeps[t][k][0])) for k in range(ns)] if rc == loamx.OK else None))
        return models, out, registered

    dbs = [loamx.PlaceDB(exclude_recent=0) for _ in range(ns)]
    models, a, registered = run(dbs)
    _, b, _ = run(None)
    assert registered >= 2
    for (rca, ga, fa), (rcb, gb, fb) in zip(a, b):
        assert rca == rcb
        for (tra, tsa, afa, sta), (trb, tsb, afb, stb) in zip(ga, gb):
            assert np.array_equal(tra, trb) and np.array_equal(tsa, tsb) and np.array_equal(afa, afb) and sta == stb
        assert (fa is None) == (fb is None)
        if fa is not None:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(fa, fb))
    for k in range(ns):
        assert len(dbs[k]) == registered
        for i in range(registered):
            _same_entry(dbs[k], i, models[k].desc[i], models[k].keys[i])
        last = len(models[k]) - 1
        _same_matches(dbs[k].query_entry(last, n_results=3), models[k].query_entry(last, n_results=3))


def test_adds_from_several_sources_into_one_database():
    """one database fed from a mapper's stream, a pipeline's stream and the host in turn, queried at once: the adds are ordered by events"""
    n = 4
    cm, sm, msweeps = _mapper_chain(n, seed=950)
    ns, T = 2, 4
    pcm, psm, sweeps, starts = _pipeline_case(ns, T)
    db, m = _pair(exclude_recent=0)
    sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
    mp.load_cubes(cm, sm)
    landing = np.zeros((max(len(s.points) for s in msweeps), 4), F)
    p = loamx.Pipeline(ns)
    p.set_frozen(pcm, psm)
    for s in range(ns):
        p.set_state(s, aft=starts[s])
    p.upload(sweeps)
    host = _sweep("VLP-16", 900, seed=77)
    for t in range(n):
        sr.process_linked(msweeps[t].points.copy(), msweeps[t].ring_sizes)
        od.process_linked(sr)
        rc, reg = mp.process_linked(od, landing)
        rcp = p.step(t)
        got = [db.add_from(mp)]
        want = [m.add(reg, mp.transform("aft")[3:])]
        if rcp == loamx.OK:
            for k in range(ns):
                got.append(db.add_from_pipeline(p, k))
                want.append(m.add(p.download_full_res(k, len(sweeps[t][k][0])), p.get(k)[2][3:]))
        got.append(db.add(host, (0.1 * t, 0, 0)))
        want.append(m.add(host, (0.1 * t, 0, 0)))
        assert got == want
        _same_matches(db.query_entry(len(m) - 1, n_results=4), m.query_entry(len(m) - 1, n_results=4))
    assert len(db) == len(m) > 2 * n
    for i in range(len(m)):
        _same_entry(db, i, m.desc[i], m.keys[i])
    _same_matches(db.query(host, (0.05, 0, 0), n_results=6), m.query(host, (0.05, 0, 0), n_results=6))
