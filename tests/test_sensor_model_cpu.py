"""CPU: the sensor-model C-ABI (loamx_sensor_model, include/loamx.h) — declared and exported, laid out as a C compiler lays it out,
validated on the host without a device; and the synthetic driver records (synth.to_records) the GPU tests feed it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from loam_velodyne_amd import loamx, synth

NEW_SYMBOLS = ("loamx_sensor_model_from_mapper", "loamx_sensor_model_check", "loamx_scanreg_process_sensor",
               "loamx_pipeline_stage_step_sensor")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays


def test_struct_layout_matches_c(tmp_path):
    probe = tmp_path / "probe.c"
    fields = [f for f, _ in loamx.SensorModel._fields_]
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     '  printf("%zu\\n", sizeof(loamx_sensor_model));\n' +
                     "".join(f'  printf("%zu\\n", offsetof(loamx_sensor_model, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(loamx.SensorModel)
    assert got[1:] == [getattr(loamx.SensorModel, f).offset for f in fields]


@pytest.mark.parametrize("sensor", ["VLP-16", "HDL-32", "HDL-64E"])
def test_from_mapper_round_trips(sensor):
    mp = loamx._mapper(sensor, None)
    m = loamx.SensorModel.from_mapper(sensor)
    assert (m.n_scan_rings, m.ring_source, m.time_source) == (mp.n_scan_rings, loamx.RING_FROM_BOUNDS, loamx.TIME_FROM_AZIMUTH)
    assert (m.lower_bound_deg, m.upper_bound_deg) == (mp.lower_bound_deg, mp.upper_bound_deg)
    m.check(12)


def _velodyne_model(**kw):
    m = loamx.SensorModel.from_dtype(synth.RECORD_LAYOUTS["velodyne"], ring="ring", time="time", n_rings=32)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_check_accepts_valid_models():
    _velodyne_model().check(32)
    loamx.SensorModel.from_dtype(synth.RECORD_LAYOUTS["ouster"], ring="ring", time="t", time_scale=1e-9, n_rings=128).check(48)
    loamx.SensorModel.from_dtype(synth.RECORD_LAYOUTS["hesai"], ring="ring", time="timestamp", n_rings=256).check(32)
    loamx.SensorModel().set_table([-25.0, -1.0, 0.0, 0.5, 15.0], 0.5).check(12)
    loamx.SensorModel.from_dtype(synth.RECORD_LAYOUTS["velodyne"], ring=None, table=np.linspace(-10, 10, 4), max_error_deg=1.0).check(32)
    m = loamx.SensorModel.from_dtype(np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("r", "u1"), ("pad", "u1", 3)]), ring="r", n_rings=1)
    m.check(16)


def _invalid_models():
    nan = float("nan")
    yield "unknown ring source", _velodyne_model(ring_source=3), 32
    yield "unknown time source", _velodyne_model(time_source=2), 32
    yield "ring type F32", _velodyne_model(ring_type=loamx.FIELD_F32), 32
    yield "ring type 0", _velodyne_model(ring_type=0), 32
    yield "time type U16", _velodyne_model(time_type=loamx.FIELD_U16), 32
    yield "time type 9", _velodyne_model(time_type=9), 32
    yield "ring field outside stride", _velodyne_model(ring_offset=32), 32
    yield "time field outside stride", _velodyne_model(time_offset=28), 28
    yield "misaligned ring", _velodyne_model(ring_offset=21), 32
    yield "misaligned f64 time", _velodyne_model(time_type=loamx.FIELD_F64, time_offset=20), 32
    yield "time_scale 0", _velodyne_model(time_scale=0.0), 32
    yield "time_scale < 0", _velodyne_model(time_scale=-1e-9), 32
    yield "time_scale nan", _velodyne_model(time_scale=nan), 32
    yield "time_scale inf", _velodyne_model(time_scale=float("inf")), 32
    yield "0 rings", _velodyne_model(n_scan_rings=0), 32
    yield "257 rings", _velodyne_model(n_scan_rings=257), 32
    yield "stride 30", _velodyne_model(), 30
    yield "stride 8", loamx.SensorModel.from_mapper("VLP-16"), 8
    b = loamx.SensorModel.from_mapper("VLP-16"); b.n_scan_rings = 1
    yield "bounds with 1 ring", b, 12
    b = loamx.SensorModel.from_mapper("VLP-16"); b.upper_bound_deg = b.lower_bound_deg
    yield "bounds upper == lower", b, 12
    t = loamx.SensorModel().set_table([-1.0, 0.0, 1.0], 0.5); t.ring_angles_deg = None
    yield "NULL table", t, 12
    yield "table not increasing", loamx.SensorModel().set_table([-1.0, 0.0, 0.0, 1.0], 0.5), 12
    yield "table decreasing", loamx.SensorModel().set_table([1.0, 0.0], 0.5), 12
    yield "table nan", loamx.SensorModel().set_table([-1.0, nan, 1.0], 0.5), 12
    yield "table inf", loamx.SensorModel().set_table([-1.0, 0.0, float("inf")], 0.5), 12
    yield "max error 0", loamx.SensorModel().set_table([-1.0, 1.0], 0.0), 12
    yield "max error < 0", loamx.SensorModel().set_table([-1.0, 1.0], -0.5), 12
    yield "max error nan", loamx.SensorModel().set_table([-1.0, 1.0], nan), 12
    yield "table 0 rings", loamx.SensorModel().set_table([], 0.5), 12


@pytest.mark.parametrize("case", list(_invalid_models()), ids=lambda c: c[0])
def test_check_rejects_invalid_models(case):
    _, m, stride = case
    with pytest.raises(loamx.LoamxError) as e:
        m.check(stride)
    assert e.value.code == loamx.E_INVALID
    assert loamx.lib().loamx_last_error()   # with a message


def test_make_sweep_without_elevations_is_unchanged():
    """elevations_deg omitted: the even spacing of the preset, byte for byte (np.linspace, as before the argument existed)"""
    w = synth.World(half_extent=30.0)
    a = synth.make_sweep(w, "VLP-16", np.zeros(6), np.array([0, 0.01, 0, 0.2, 0, 0.5]), seed=4, az_steps=90)
    b = synth.make_sweep(w, "VLP-16", np.zeros(6), np.array([0, 0.01, 0, 0.2, 0, 0.5]), seed=4, az_steps=90,
                         elevations_deg=np.linspace(-15.0, 15.0, 16))
    assert a.points.tobytes() == b.points.tobytes() and np.array_equal(a.ring_sizes, b.ring_sizes)
    c = synth.make_sweep(w, "VLP-16", np.zeros(6), np.zeros(6), seed=4, az_steps=90, elevations_deg=[-20.0, -3.0, 0.0, 1.0, 9.0])
    assert len(c.ring_sizes) == 5 and c.points.shape == (5 * 90, 4)


@pytest.mark.parametrize("layout,ring,time,scale", [("velodyne", "ring", "time", 1.0), ("ouster", "ring", "t", 1e-9),
                                                    ("hesai", "ring", "timestamp", 1.0)])
def test_records_put_fields_where_the_model_reads_them(layout, ring, time, scale):
    w = synth.World(half_extent=30.0)
    sw = synth.make_sweep(w, "VLP-16", np.zeros(6), np.zeros(6), seed=5, az_steps=60)
    rec = synth.to_records(sw, layout, bad_every=7)
    m = loamx.SensorModel.from_dtype(rec.dtype, ring=ring, time=time, time_scale=scale, n_rings=16)
    m.check(rec.dtype.itemsize)
    raw = rec.view(np.uint8).reshape(len(rec), rec.dtype.itemsize)
    fmt = {loamx.FIELD_U16: "<u2", loamx.FIELD_U32: "<u4", loamx.FIELD_F32: "<f4", loamx.FIELD_F64: "<f8"}
    rv = raw[:, m.ring_offset:m.ring_offset + 2].copy().view(fmt[m.ring_type]).ravel()
    tv = raw[:, m.time_offset:m.time_offset + np.dtype(fmt[m.time_type]).itemsize].copy().view(fmt[m.time_type]).ravel()
    A, R = 60, 16
    ring_major = layout == "ouster"
    laser = np.tile(np.arange(R), A) if not ring_major else np.repeat(np.arange(R), A)
    step = np.repeat(np.arange(A), R) if not ring_major else np.tile(np.arange(A), R)
    planted = (step % 7 == 3) & (step < A - 1) & (laser == 2)
    assert np.array_equal(rv[~planted], laser[~planted]) and np.all(rv[planted] == R)
    rel = (tv.astype(np.float64) - (1.7e9 if layout == "hesai" else 0.0)) * scale
    assert np.allclose(rel, 0.1 * step / A, atol=1e-6)
    xyz = raw[:, :12].copy().view("<f4").reshape(-1, 3)
    firing = synth.to_raw(sw, bad_every=7).reshape(A, R, 3)
    want = firing.transpose(1, 0, 2).reshape(-1, 3) if ring_major else firing.reshape(-1, 3)
    assert np.array_equal(xyz, want, equal_nan=True)
