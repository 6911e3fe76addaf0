"""GPU: pins of the raw-sweep ingestion kernels (csrc/ingest.hip) at the shapes where the stable split can go wrong, and of the
ring / time source combinations no other test runs.  Every comparison is bit for bit, except against the oracle's binning, where
tests/test_gpu_ingest.py's rule holds: xyz, ring and order exact, intensity = ring + relTime within 2 ulp of the stored value."""
import numpy as np
import pytest

import oracle_py as op
from loam_velodyne_amd import loamx, synth
from sensor_model_np import _np_bin_time_field

pytestmark = pytest.mark.gpu

FEATS = ("sharp", "less_sharp", "flat", "less_flat")
# x, y, z, a one-byte ring (256 rings fit) and the time in seconds
REC = np.dtype({"names": ["x", "y", "z", "ring", "time"], "formats": ["f4", "f4", "f4", "u1", "f4"], "offsets": [0, 4, 8, 12, 16],
                "itemsize": 20})
# 1 point; one short of / exactly / one past a wave; the same around a workgroup of 256; a last workgroup that holds one point
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 513)


def _same(a, b, keys=("full", "ring_sizes") + FEATS):
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def _like_oracle(g, o_pts, o_rs):
    """tests/test_gpu_ingest.py::test_binning_matches_oracle's comparison"""
    assert np.array_equal(g["ring_sizes"], o_rs)
    assert g["full"].shape == o_pts.shape
    assert np.array_equal(g["full"][:, :3], o_pts[:, :3])
    assert np.array_equal(np.floor(g["full"][:, 3] + 1e-4), np.floor(o_pts[:, 3] + 1e-4))
    assert np.all(np.abs(g["full"][:, 3] - o_pts[:, 3]) <= 2 * np.spacing(np.maximum(np.abs(o_pts[:, 3]), np.float32(1.0))))


def _angles(lo, hi, nr):
    """the elevation (degrees) the linear mapper (lo, hi, nr) puts in the middle of every ring"""
    return lo + np.arange(nr) * (hi - lo) / (nr - 1)


def _records(ids, lo, hi, nr, span=0.98, room=False):
    """len(ids) returns at advancing azimuth over `span` of a revolution (away from the +-pi seam), ranges 3 .. 9 m (room: the walls
    of a square room 5 m from the sensor, flat stretches and four corners), point i at the elevation of ring ids[i] of the mapper
    (lo, hi, nr): bounds, the table _angles(lo, hi, nr) and the ring field give the same ring.  The time field runs to 0.11 s, so
    its last tenth meets the clamp at scan_period."""
    n = len(ids)
    i = np.arange(n)
    ori = -2.8 + 2 * np.pi * span * i / n
    el = np.deg2rad(_angles(lo, hi, nr)[ids])
    rng = 5.0 / np.maximum(np.abs(np.cos(ori)), np.abs(np.sin(ori))) if room else 6.0 + 3.0 * np.sin(0.37 * i)
    rec = np.zeros(n, REC)
    rec["x"], rec["y"], rec["z"] = rng * np.cos(ori) * np.cos(el), -rng * np.sin(ori) * np.cos(el), rng * np.sin(el)
    rec["ring"] = ids
    rec["time"] = 0.11 * i / n
    return rec


def _xyz(rec):
    return np.stack([rec["x"], rec["y"], rec["z"]], 1)


def _models(lo, hi, nr):
    return {"bounds": loamx.SensorModel.from_mapper(mapper=(lo, hi, nr)),
            "field": loamx.SensorModel.from_dtype(REC, ring="ring", n_rings=nr),
            "table": loamx.SensorModel().set_table(_angles(lo, hi, nr), 0.05),
            "field_time": loamx.SensorModel.from_dtype(REC, ring="ring", time="time", n_rings=nr)}


def _one_ring(n):
    return _records(np.full(n, 3), -15.0, 15.0, 16), (-15.0, 15.0, 16)


def _distinct_rings(n):
    """64 different rings in every wave: the rank loop runs once per lane"""
    return _records(np.arange(n) % 256, -25.5, 25.5, 256), (-25.5, 25.5, 256)


def _some_rings_empty(n):
    rec = _records(np.array([1, 4, 4, 11, 5, 1, 1])[np.arange(n) % 7], -15.0, 15.0, 16)
    rec["x"][5:n - 1:5] = np.nan   # (never the first / last return: they define startOri / endOri)
    return rec, (-15.0, 15.0, 16)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("content", [_one_ring, _distinct_rings, _some_rings_empty])
def test_split_edge_shapes(orc, content, n):
    rec, mapper = content(n)
    models = _models(*mapper)
    h = loamx.ScanRegistration()
    b = h.process_sensor(rec, models["bounds"])
    _like_oracle(b, *op.multiscan_bin(orc, _xyz(rec), mapper))
    assert b["ring_sizes"].sum() == len(b["full"]) == np.isfinite(rec["x"]).sum()
    _same(h.process_raw(_xyz(rec), mapper=mapper), b)
    _same(h.process_sensor(rec, models["field"]), b)
    _same(h.process_sensor(rec, models["table"]), b)
    ft = h.process_sensor(rec, models["field_time"])
    full, rs = _np_bin_time_field(rec, "time", 1.0, mapper[2])
    assert np.array_equal(ft["ring_sizes"], rs) and np.array_equal(rs, b["ring_sizes"])
    assert ft["full"].shape == full.shape and np.array_equal(ft["full"], full)
    assert np.array_equal(ft["full"][:, :3], b["full"][:, :3])   # the same split; only relTime has another source


@pytest.mark.parametrize("n", LENGTHS)
def test_split_every_point_rejected(orc, n):
    """NaN, zero range, 45 deg above a field of view that ends at 15 (ring field: 16 of 16 rings), and for the time field a ring
    that is valid with a time that is not finite"""
    rec = _records(np.full(n, 3), -15.0, 15.0, 16)
    kind = np.arange(n) % 4
    rec["x"][kind == 0] = np.nan
    for k in "xyz":
        rec[k][kind == 1] = 0.0
    up = kind >= 2
    rec["x"][up], rec["y"][up], rec["z"][up], rec["ring"][up] = 5.0, 1.0, np.float32(np.hypot(5.0, 1.0)), 16
    models = _models(-15.0, 15.0, 16)
    h = loamx.ScanRegistration()
    o_pts, o_rs = op.multiscan_bin(orc, _xyz(rec), (-15.0, 15.0, 16))
    assert len(o_pts) == 0 and not o_rs.any()
    runs = [h.process_raw(_xyz(rec), mapper=(-15.0, 15.0, 16))] + [h.process_sensor(rec, models[k]) for k in ("bounds", "field", "table")]
    late = rec.copy()
    late["ring"][kind == 3] = 3
    late["time"][kind == 3] = np.where(np.arange((kind == 3).sum()) % 2, np.nan, np.inf)
    runs.append(h.process_sensor(late, models["field_time"]))
    for g in runs:
        assert g["full"].shape == (0, 4) and g["ring_sizes"].shape == (16,) and not g["ring_sizes"].any()
        for k in FEATS:
            assert len(g[k]) == 0, k


def test_bounds_and_table_with_time_field(small_world):
    """the two classify instantiations no other test runs: ring from bounds / a table, relTime from the time field.  synth.to_records'
    ring field agrees with both (the planted out-of-field returns carry an invalid ring), so RING_FROM_FIELD is the expected value."""
    dt = synth.RECORD_LAYOUTS["velodyne"]
    sw = synth.make_sweep(small_world, "VLP-16", np.zeros(6), np.array([0.002, 0.01, 0.0, 0.3, 0.0, 0.9]), seed=5, az_steps=300)
    rec = synth.to_records(sw, "velodyne", bad_every=7)
    f = loamx.ScanRegistration().process_sensor(rec, loamx.SensorModel.from_dtype(dt, ring="ring", time="time", n_rings=16))
    b = loamx.ScanRegistration().process_sensor(rec, loamx.SensorModel.from_dtype(dt, ring=None, mapper="VLP-16", time="time"))
    _same(b, f)
    assert f["ring_sizes"].sum() == len(rec) - 3 * len(range(7 // 2, 300 - 1, 7)) and f["full"][:, 3].max() % 1.0 > 0.09
    elev = np.array([-25.0, -15.639, -11.31, -8.843, -7.254, -6.148, -5.333, -4.667, -4.0, -3.667, -3.333, -3.0, -2.667, -2.333, -2.0,
                     -1.667, -1.333, -1.0, -0.667, -0.333, 0.0, 0.333, 0.667, 1.0, 1.333, 1.667, 2.333, 3.333, 4.667, 7.0, 10.333, 15.0])
    sw = synth.make_sweep(small_world, "HDL-32", np.zeros(6), np.array([0.0, 0.01, 0.0, 0.2, 0.0, 0.6]), seed=6, az_steps=200,
                          elevations_deg=elev)
    rec = synth.to_records(sw, "velodyne", bad_every=13)
    f = loamx.ScanRegistration().process_sensor(rec, loamx.SensorModel.from_dtype(dt, ring="ring", time="time", n_rings=32))
    t = loamx.ScanRegistration().process_sensor(rec, loamx.SensorModel.from_dtype(dt, ring=None, table=elev, max_error_deg=0.1, time="time"))
    _same(t, f)
    assert f["ring_sizes"].sum() == len(rec) - 3 * len(range(13 // 2, 200 - 1, 13))


def _pin3_records():
    return _records(np.zeros(600, np.int64), -15.0, 15.0, 16, room=True)


def _imu_until(handles, t_imu, k_imu, t_end):
    """tests/test_gpu_ingest.py::test_imu_deskew_matches_oracle's IMU messages (0.77 ms apart, a planted 6.2 rad yaw wrap)"""
    while t_imu < t_end:
        roll, pitch, yaw = 0.02 * np.sin(3 * t_imu), 0.015 * np.cos(2 * t_imu), 0.4 * t_imu + (6.2 if k_imu % 97 == 50 else 0.0)
        for h in handles:
            h.update_imu(t_imu, roll, pitch, yaw, (0.8 * np.sin(5 * t_imu), 0.1, -0.5 * np.cos(4 * t_imu)))
        t_imu += 0.00077
        k_imu += 1
    return t_imu, k_imu


def test_time_field_with_imu_equals_azimuth():
    """The IMU de-skew with relTime from the time field, against the azimuth path (which tests/test_gpu_ingest.py pins to the oracle): a
    one-ring sweep whose time field holds, bit for bit, the relTime its azimuths give.  For ring 0 the stored intensity is 0 + relTime,
    and one ring makes the split the identity, so a run without IMU data returns every point's relTime in firing order."""
    rec = _pin3_records()
    n = len(rec)
    az = loamx.SensorModel.from_dtype(REC, ring="ring", n_rings=1)
    fld = loamx.SensorModel.from_dtype(REC, ring="ring", time="time", time_scale=1.0, n_rings=1)
    plain = loamx.ScanRegistration().process_sensor(rec, az)
    assert len(plain["full"]) == n and np.array_equal(plain["full"][:, :3], _xyz(rec)[:, [1, 2, 0]])
    rel = plain["full"][:, 3].copy()
    # conditions on the input: t_ref = 0 makes the time field's subtraction exact, and its clamp at scan_period does not bite
    assert rel.min() == 0.0 and rel.max() <= np.float32(0.1) and rel.max() > 0.09
    rec["time"] = rel
    a, f = loamx.ScanRegistration(), loamx.ScanRegistration()
    t_imu, k_imu = 0.0, 0
    for k in range(3):
        t_scan = 0.1 * (k + 1)
        t_imu, k_imu = _imu_until((a, f), t_imu, k_imu, t_scan + 0.12)
        a.set_time(t_scan)
        f.set_time(t_scan)
        ga, gf = a.process_sensor(rec, az), f.process_sensor(rec, fld)
        _same(ga, gf)
        assert len(ga["full"]) == n and not np.array_equal(ga["full"][:, :3], plain["full"][:, :3])   # the points were de-skewed
        assert len(ga["sharp"]) and len(ga["flat"])
        assert np.array_equal(a.imu_trans(), f.imu_trans()), k
        if k >= 1:
            assert np.abs(f.imu_trans()).max() > 1e-3   # the IMU path is really active


def test_ring_sources_agree_with_time_field_and_imu(small_world):
    """the same IMU history and time field through the three ring sources (they agree on synth.to_records' sweeps)"""
    dt = synth.RECORD_LAYOUTS["velodyne"]
    models = [loamx.SensorModel.from_dtype(dt, ring="ring", time="time", n_rings=16),
              loamx.SensorModel.from_dtype(dt, ring=None, mapper="VLP-16", time="time"),
              loamx.SensorModel.from_dtype(dt, ring=None, table=_angles(-15.0, 15.0, 16), max_error_deg=0.1, time="time")]
    hs = [loamx.ScanRegistration() for _ in models]
    t_imu, k_imu = 0.0, 0
    for k in range(3):
        t_scan = 0.1 * (k + 1)
        t_imu, k_imu = _imu_until(hs, t_imu, k_imu, t_scan + 0.12)
        sw = synth.make_sweep(small_world, "VLP-16", np.zeros(6), np.array([0.0, 0.04, 0.0, 0.1, 0.0, 0.5]), seed=40 + k, az_steps=300)
        rec = synth.to_records(sw, "velodyne", bad_every=33)
        runs = []
        for h, m in zip(hs, models):
            h.set_time(t_scan)
            runs.append(h.process_sensor(rec, m))
        for g, h in zip(runs[1:], hs[1:]):
            _same(g, runs[0])
            assert np.array_equal(h.imu_trans(), hs[0].imu_trans()), k
        assert runs[0]["ring_sizes"].sum() == len(rec) - 3 * len(range(33 // 2, 300 - 1, 33))
        if k >= 1:
            assert np.abs(hs[0].imu_trans()).max() > 1e-3
