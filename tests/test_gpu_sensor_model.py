"""GPU: raw-sweep ingestion with a sensor model (loamx_sensor_model, include/loamx.h): ring from bounds / a table / a ring field,
relTime from the azimuth / a time field.  Every comparison is bit for bit unless it says otherwise."""
import numpy as np
import pytest

import oracle_py as op
from loam_velodyne_amd import loamx, synth
from sensor_model_np import _np_bin_time_field

pytestmark = pytest.mark.gpu

FEATS = ("sharp", "less_sharp", "flat", "less_flat")
# VLP-32C-like laser elevations (dense near 0 deg, sparse toward -25 / +15): not evenly spaced
VLP32C = np.array([-25.0, -15.639, -11.31, -8.843, -7.254, -6.148, -5.333, -4.667, -4.0, -3.667, -3.333, -3.0, -2.667, -2.333, -2.0,
                   -1.667, -1.333, -1.0, -0.667, -0.333, 0.0, 0.333, 0.667, 1.0, 1.333, 1.667, 2.333, 3.333, 4.667, 7.0, 10.333, 15.0])


def _same(a, b, keys=("full", "ring_sizes") + FEATS):
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def _as_velodyne(raw):
    """(n, 3) float32 -> stride-32 PointXYZIRT-style records holding the same x, y, z (ring 0, time 0)"""
    rec = np.zeros(len(raw), synth.RECORD_LAYOUTS["velodyne"])
    rec["x"], rec["y"], rec["z"] = raw[:, 0], raw[:, 1], raw[:, 2]
    return rec


def _velodyne_field_ring(n_rings, time=None):
    return loamx.SensorModel.from_dtype(synth.RECORD_LAYOUTS["velodyne"], ring="ring", time=time, n_rings=n_rings)


@pytest.mark.parametrize("sensor,az,bad", [("VLP-16", 1800, 0), ("VLP-16", 900, 7), ("HDL-32", 512, 16), ("HDL-64E", 2048, 64)])
def test_bounds_azimuth_equals_process_raw(small_world, sensor, az, bad):
    sw = synth.make_sweep(small_world, sensor, np.zeros(6), np.array([0.002, 0.01, 0.0, 0.3, 0.0, 0.9]), seed=az, az_steps=az)
    raw = synth.to_raw(sw, bad_every=bad)
    if bad:
        R = synth.SENSORS[sensor][0]
        raw = np.roll(raw.reshape(az, R, 3), az // 3, axis=0).reshape(-1, 3)
    g = loamx.ScanRegistration().process_raw(raw, sensor)
    s = loamx.ScanRegistration().process_sensor(_as_velodyne(raw), loamx.SensorModel.from_mapper(sensor))
    _same(g, s)


@pytest.mark.parametrize("sensor,az,bad", [("VLP-16", 900, 7), ("HDL-32", 512, 16), ("HDL-64E", 1024, 64)])
def test_field_ring_azimuth_equals_process_raw(small_world, sensor, az, bad):
    sw = synth.make_sweep(small_world, sensor, np.zeros(6), np.array([0.002, 0.01, 0.0, 0.3, 0.0, 0.9]), seed=az + 1, az_steps=az)
    raw = synth.to_raw(sw, bad_every=bad)
    rec = synth.to_records(sw, "velodyne", bad_every=bad)
    R = synth.SENSORS[sensor][0]
    assert np.all(rec["ring"][np.arange(bad // 2, az - 1, bad) * R + 2] == R)   # the planted out-of-field returns carry an invalid ring
    g = loamx.ScanRegistration().process_raw(raw, sensor)
    s = loamx.ScanRegistration().process_sensor(rec, _velodyne_field_ring(R))
    _same(g, s)
    # a return the angle mapper drops (45 deg up) but whose ring field is valid: kept in ring 5
    extra = rec.copy()
    k = len(extra) // 2
    extra["x"][k], extra["y"][k], extra["z"][k], extra["ring"][k] = 10.0, 0.0, 10.0, 5
    s2 = loamx.ScanRegistration().process_sensor(extra, _velodyne_field_ring(R))
    r2 = loamx.ScanRegistration().process_raw(np.stack([extra["x"], extra["y"], extra["z"]], 1), sensor)
    assert s2["ring_sizes"][5] == r2["ring_sizes"][5] + 1 and s2["ring_sizes"].sum() == r2["ring_sizes"].sum() + 1
    lo = s2["ring_sizes"][:5].sum()
    ring5 = s2["full"][lo:lo + s2["ring_sizes"][5]]
    hit = (ring5[:, 0] == 0.0) & (ring5[:, 1] == 10.0) & (ring5[:, 2] == 10.0)   # LOAM frame: (y, z, x)
    assert hit.sum() == 1 and np.floor(ring5[hit, 3][0]) == 5


def test_table_on_uneven_lasers(orc, small_world):
    sw = synth.make_sweep(small_world, "HDL-32", np.zeros(6), np.array([0.0, 0.01, 0.0, 0.2, 0.0, 0.6]), seed=3, az_steps=1024,
                          elevations_deg=VLP32C)
    rec = synth.to_records(sw, "velodyne", bad_every=13)
    table = loamx.SensorModel().set_table(VLP32C, 0.1)
    t = loamx.ScanRegistration().process_sensor(rec, table)
    f = loamx.ScanRegistration().process_sensor(rec, _velodyne_field_ring(32))
    _same(t, f)
    assert t["ring_sizes"].sum() == len(rec) - 3 * len(range(13 // 2, 1024 - 1, 13))   # every return but the planted ones
    # the linear mapper over the same field of view puts these returns in other rings: the limitation the table removes
    b = loamx.ScanRegistration().process_sensor(rec, loamx.SensorModel.from_mapper(mapper=(-25.0, 15.0, 32)))
    assert not np.array_equal(b["ring_sizes"], t["ring_sizes"])
    # a return 4 deg away from every table entry (-20 deg lies between -25 and -15.639) is dropped; nothing else moves
    planted = np.insert(rec, len(rec) // 2, rec[len(rec) // 2])
    k = len(rec) // 2
    planted["x"][k], planted["y"][k], planted["z"][k] = 10.0, 0.0, 10.0 * np.tan(np.deg2rad(-20.0))
    _same(loamx.ScanRegistration().process_sensor(planted, table), t)
    # features: the oracle's ScanRegistration on the binned cloud
    of = op.ScanRegistration(orc).process(t["full"], t["ring_sizes"])
    for k in FEATS:
        assert t[k].shape == of[k].shape and np.array_equal(t[k][:, :3], of[k][:, :3]), k


@pytest.mark.parametrize("layout,time,scale", [("velodyne", "time", 1.0), ("ouster", "t", 1e-9), ("hesai", "timestamp", 1.0)])
def test_time_field_any_order(orc, small_world, layout, time, scale):
    sw = synth.make_sweep(small_world, "VLP-16", np.zeros(6), np.array([0.0, 0.02, 0.0, 0.3, 0.0, 0.8]), seed=8, az_steps=1200)
    model = loamx.SensorModel.from_dtype(synth.RECORD_LAYOUTS[layout], ring="ring", time=time, time_scale=scale, n_rings=16)
    runs = []
    for ring_major in (False, True):
        rec = synth.to_records(sw, layout, bad_every=29, ring_major=ring_major)
        g = loamx.ScanRegistration().process_sensor(rec, model)
        full, rs = _np_bin_time_field(rec, time, scale, 16)
        assert np.array_equal(g["ring_sizes"], rs)
        assert g["full"].shape == full.shape and np.array_equal(g["full"], full), ring_major
        p = loamx.ScanRegistration().process(full, rs)
        of = op.ScanRegistration(orc).process(full, rs)
        for k in FEATS:
            assert np.array_equal(g[k], p[k]), k
            assert g[k].shape == of[k].shape and np.array_equal(g[k][:, :3], of[k][:, :3]), k
        runs.append(g)
    _same(runs[0], runs[1])
    assert runs[0]["full"][:, 3].max() % 1.0 > 0.09     # relTime spans the sweep


def test_field_ring_with_imu_equals_process_raw(small_world):
    """mirrors tests/test_gpu_ingest.py::test_imu_deskew_matches_oracle: IMU messages between the sweeps, the 200-deep history wraps"""
    g, s = loamx.ScanRegistration(), loamx.ScanRegistration()
    model = _velodyne_field_ring(16)
    t_imu, k_imu = 0.0, 0
    for k in range(4):
        t_scan = 0.1 * (k + 1)
        while t_imu < t_scan + 0.12:
            roll, pitch, yaw = 0.02 * np.sin(3 * t_imu), 0.015 * np.cos(2 * t_imu), 0.4 * t_imu + (6.2 if k_imu % 97 == 50 else 0.0)
            acc = (0.8 * np.sin(5 * t_imu), 0.1, -0.5 * np.cos(4 * t_imu))
            g.update_imu(t_imu, roll, pitch, yaw, acc)
            s.update_imu(t_imu, roll, pitch, yaw, acc)
            t_imu += 0.00077
            k_imu += 1
        sw = synth.make_sweep(small_world, "VLP-16", np.zeros(6), np.array([0.0, 0.04, 0.0, 0.1, 0.0, 0.5]), seed=30 + k, az_steps=700)
        g.set_time(t_scan)
        s.set_time(t_scan)
        a = g.process_raw(synth.to_raw(sw, bad_every=33), "VLP-16")
        b = s.process_sensor(synth.to_records(sw, "velodyne", bad_every=33), model)
        _same(a, b)
        assert np.array_equal(g.imu_trans(), s.imu_trans()), k
        if k >= 1:
            assert np.abs(s.imu_trans()).max() > 1e-3


def _pipeline_run(small_world, T, ns, layout):
    recs, starts = [[None] * ns for _ in range(T)], []
    for s in range(ns):
        poses = synth.trajectory(T, start=(1.5 * s, 0.0, 2.0 * s))
        starts.append(np.array([0, 0, 0, 1.5 * s, 0, 2.0 * s], np.float32))
        for t in range(T):
            sw = synth.make_sweep(small_world, "VLP-16", poses[t], poses[t + 1], seed=70 * s + t, az_steps=600)
            recs[t][s] = synth.to_records(sw, layout, bad_every=41 + s)
    return recs, starts


def _stream_steps(p, T, stage):
    out = []
    for t in range(3):
        stage(t)
    for t in range(T):
        r = p.step(t)
        if t + 3 < T:
            stage(t + 3)
        out.append((r, [p.get(s) for s in range(p.n_streams)]))
    return out


def _same_runs(ra, rb):
    for (a, ga), (b, gb) in zip(ra, rb):
        assert a == b
        for x, y in zip(ga, gb):
            for i in range(3):
                assert np.array_equal(x[i], y[i])
            assert x[3] == y[3]


@pytest.mark.parametrize("layout,time,scale", [("ouster", "t", 1e-9), ("velodyne", None, 1.0)])
def test_pipeline_stage_step_sensor(small_world, layout, time, scale):
    """4 streams x 6 steps: stage_step_sensor == stage_step fed the process_sensor binnings (mirrors
    tests/test_gpu_pipeline.py::test_raw_sweeps_into_the_pipeline_equal_binned_rings)"""
    T, ns = 6, 4
    recs, starts = _pipeline_run(small_world, T, ns, layout)
    cm, sm = small_world.make_map(60000)
    model = loamx.SensorModel.from_dtype(synth.RECORD_LAYOUTS[layout], ring="ring", time=time, time_scale=scale, n_rings=16)

    def make():
        p = loamx.Pipeline(ns)
        p.set_frozen(cm, sm)
        for s in range(ns):
            p.set_state(s, aft=starts[s])
        return p
    sr = loamx.ScanRegistration()
    binned = []
    for t in range(T):
        row = []
        for s in range(ns):
            g = sr.process_sensor(recs[t][s], model)
            row.append((g["full"], g["ring_sizes"]))
        binned.append(row)
    a, b = make(), make()
    ra = _stream_steps(a, T, lambda t: a.stage_step(t, binned[t]))
    rb = _stream_steps(b, T, lambda t: b.stage_step_sensor(t, recs[t], model))
    _same_runs(ra, rb)


def test_pipeline_bounds_model_equals_stage_step_raw(small_world):
    T, ns = 6, 4
    recs, starts = _pipeline_run(small_world, T, ns, "velodyne")
    raws = [[np.stack([r["x"], r["y"], r["z"]], 1) for r in row] for row in recs]
    cm, sm = small_world.make_map(60000)

    def make():
        p = loamx.Pipeline(ns)
        p.set_frozen(cm, sm)
        for s in range(ns):
            p.set_state(s, aft=starts[s])
        return p
    model = loamx.SensorModel.from_mapper("VLP-16")
    a, b = make(), make()
    ra = _stream_steps(a, T, lambda t: a.stage_step_raw(t, raws[t], "VLP-16"))
    rb = _stream_steps(b, T, lambda t: b.stage_step_sensor(t, recs[t], model))
    _same_runs(ra, rb)


def test_invalid_model_leaves_handle_usable(small_world):
    sw = synth.make_sweep(small_world, "VLP-16", np.zeros(6), np.zeros(6), seed=12, az_steps=600)
    rec = synth.to_records(sw, "ouster", bad_every=19)
    good = loamx.SensorModel.from_dtype(rec.dtype, ring="ring", time="t", time_scale=1e-9, n_rings=16)
    bad = loamx.SensorModel.from_dtype(rec.dtype, ring="ring", time="t", time_scale=1e-9, n_rings=16)
    bad.time_offset = 22                                   # misaligned u32
    h = loamx.ScanRegistration()
    with pytest.raises(loamx.LoamxError):
        h.process_sensor(rec, bad)
    bad2 = loamx.SensorModel().set_table([0.0, -1.0], 0.5)  # not increasing
    with pytest.raises(loamx.LoamxError):
        h.process_sensor(rec, bad2)
    _same(h.process_sensor(rec, good), loamx.ScanRegistration().process_sensor(rec, good))
    p = loamx.Pipeline(1)
    with pytest.raises(loamx.LoamxError):
        p.stage_step_sensor(0, [rec], bad)
