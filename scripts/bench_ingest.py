"""Raw-sweep ingestion: wall time of loamx_scanreg_process_raw on HDL-64E revolutions (with and
without IMU data) next to the oracle's CPU loop.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel times."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle_py as op
from loam_velodyne_amd import loamx, synth

orc = op.Oracle(fast=True) if "fast" in op.Oracle.__init__.__code__.co_varnames else op.Oracle()
w = synth.World()
sw = synth.make_sweep(w, "HDL-64E", np.zeros(6), np.array([0, 0.01, 0, 0.2, 0, 1.0]), seed=1)
raw = synth.to_raw(sw, bad_every=64)
n = len(raw)
for imu in (() if os.environ.get("BENCH_INGEST_MODE") else (False, True)):   # (a per-mode profile run skips these)
    g, o = loamx.ScanRegistration(), op.ScanRegistration(orc)
    if imu:
        for j in range(200):
            t = 0.001 * j
            for h in (g, o):
                h.update_imu(t, 0.01 * np.sin(t), 0.02 * np.cos(t), 0.3 * t, (0.2, 0.0, -0.1))
    g.set_time(0.1); g.process_raw(raw, "HDL-64E"); o.process_raw(raw, 0.1, "HDL-64E")     # warm-up / first sweep
    t0 = time.perf_counter()
    for k in range(10):
        g.set_time(0.2 + 0.1 * k)
        g.process_raw(raw, "HDL-64E")
    tg = (time.perf_counter() - t0) / 10
    t0 = time.perf_counter()
    for k in range(3):
        op.multiscan_bin(orc, raw, "HDL-64E") if not imu else o.process_raw(raw, 0.2 + 0.1 * k, "HDL-64E")
    to = (time.perf_counter() - t0) / 3
    print("imu=%d  points %d  GPU call (H2D + ingestion + features + D2H) %.2f ms   oracle %s %.2f ms" %
          (imu, n, tg * 1e3, "bin+features" if imu else "bin only", to * 1e3))

# sensor models (loamx_scanreg_process_sensor) on the same HDL-64E revolution, 131,072 points as PointXYZIRT-style records (stride 32)
# or ring-major Ouster-style records (stride 48).  Binning kernels: k_raw_unpack / k_sensor_unpack, k_raw_init,
# k_raw_classify<ring, time>, (k_sns_tref,) k_raw_colscan, k_raw_scatter<time>.  For per-mode kernel times run one mode
# per rocprofv3 --kernel-trace --stats run: BENCH_INGEST_MODE=<mode> (the modes share kernels).
R = synth.SENSORS["HDL-64E"][0]
vel = synth.to_records(sw, "velodyne", bad_every=64)
ous = synth.to_records(sw, "ouster", bad_every=64)
modes = {
    "bounds_azimuth": (vel, loamx.SensorModel.from_mapper("HDL-64E")),
    "field_ring_azimuth": (vel, loamx.SensorModel.from_dtype(vel.dtype, ring="ring", n_rings=R)),
    "table_azimuth": (vel, loamx.SensorModel().set_table(np.linspace(-24.9, 2.0, R), 0.2)),
    "field_ring_field_time": (vel, loamx.SensorModel.from_dtype(vel.dtype, ring="ring", time="time", n_rings=R)),
    "field_time_ring_major": (ous, loamx.SensorModel.from_dtype(ous.dtype, ring="ring", time="t", time_scale=1e-9, n_rings=R)),
}
only = os.environ.get("BENCH_INGEST_MODE")
for name, (rec, model) in modes.items():
    if only and name != only:
        continue
    g = loamx.ScanRegistration()
    ref = g.process_sensor(rec, model)                                  # warm-up
    t0 = time.perf_counter()
    for k in range(20):
        g.process_sensor(rec, model)
    tg = (time.perf_counter() - t0) / 20
    print("sensor %-22s points %d kept %d  GPU call (H2D + ingestion + features + D2H) %.2f ms" % (name, len(rec), len(ref["full"]), tg * 1e3))
