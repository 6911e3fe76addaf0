"""numpy restatements of the sensor-model binning (include/loamx.h, loamx_sensor_model), shared by the GPU tests."""
import numpy as np


def _np_bin_time_field(rec, time, scale, n_rings, scan_period=0.1):
    """include/loamx.h's semantics for RING_FROM_FIELD + TIME_FROM_FIELD restated in numpy"""
    X, Y, Z = rec["y"].astype(np.float32), rec["z"].astype(np.float32), rec["x"].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        keep = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
        keep &= (X * X + Y * Y + Z * Z).astype(np.float64) >= 0.0001
    ring = rec["ring"].astype(np.int64)
    t = rec[time].astype(np.float64)
    keep &= (ring < n_rings) & np.isfinite(t)
    idx = np.nonzero(keep)[0]
    tref = t[idx].min()
    rel = ((t[idx] - tref) * scale).astype(np.float32)
    rel = np.where(rel > np.float32(scan_period), np.float32(scan_period), rel)
    order = np.argsort(ring[idx], kind="stable")
    full = np.stack([X[idx], Y[idx], Z[idx], ring[idx].astype(np.float32) + rel], 1)[order]
    return full, np.bincount(ring[idx], minlength=n_rings).astype(np.int32)
