"""numpy model of the dense global map (include/loamx.h, loamx_densemap_*), exact to the bit: f32 per-point arithmetic with the roundings
of the library (built with -ffp-contract=off), integer sums per voxel, f64 export.  The checker of tests/test_densemap_cpu.py and
tests/test_gpu_densemap.py (the dense map is not in the reference, so there is no oracle for it)."""
import numpy as np

QBITS = 20
KBITS = 21
QS = np.float32(1 << QBITS)


def keys_of(points, origin, leaf, min_range=0.0, max_range=0.0):
    """(keys uint64, q (n, 3) uint64, dropped by range, dropped by key) of the points the map keeps, in input order"""
    p = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
    o = np.asarray(origin, np.float32)
    d = p - o
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    min2 = np.float32(min_range) * np.float32(min_range)
    keep = d2 >= min2
    if max_range > 0:
        keep &= d2 <= np.float32(max_range) * np.float32(max_range)
    dropped_range = int((~keep).sum())
    inv = np.float32(1.0) / np.float32(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        t = p[keep] * inv
        i = np.floor(t)
        ok = np.all(np.abs(i) < np.float32(1 << QBITS), axis=1)
    dropped_key = int((~ok).sum())
    t, i = t[ok], i[ok]
    f = t - i
    q = np.minimum((f * QS).astype(np.uint64), np.uint64((1 << QBITS) - 1))
    ii = (i.astype(np.int64) + (1 << QBITS)).astype(np.uint64)
    keys = ii[:, 0] | (ii[:, 1] << np.uint64(KBITS)) | (ii[:, 2] << np.uint64(2 * KBITS))
    return keys, q, dropped_range, dropped_key


class Model:
    def __init__(self, leaf=0.1, min_range=0.0, max_range=0.0, max_voxels=0):
        self.leaf, self.min_range, self.max_range, self.max_voxels = leaf, min_range, max_range, max_voxels
        self.keys = np.zeros(0, np.uint64)           # ascending
        self.vals = np.zeros((0, 4), np.uint64)      # n, Sx, Sy, Sz per voxel
        self.offered = self.dropped_range = self.dropped_key = 0

    def __len__(self):
        return len(self.keys)

    def would_refuse(self, n_points):
        return self.max_voxels > 0 and len(self.keys) + n_points > self.max_voxels

    def add(self, points, origin):
        """True when added, False when refused by the capacity rule (nothing changes)"""
        points = np.asarray(points, np.float32)
        if self.would_refuse(len(points)):
            return False
        keys, q, dr, dk = keys_of(points, origin, self.leaf, self.min_range, self.max_range)
        self.offered += len(points)
        self.dropped_range += dr
        self.dropped_key += dk
        new = np.concatenate([np.ones((len(keys), 1), np.uint64), q], axis=1)
        uk, inv = np.unique(np.concatenate([self.keys, keys]), return_inverse=True)
        acc = np.zeros((len(uk), 4), np.uint64)
        np.add.at(acc, inv.reshape(-1), np.concatenate([self.vals, new]))   # (integer sums: exact)
        self.keys, self.vals = uk, acc
        return True

    def stats(self):
        return dict(voxels=len(self.keys), offered=self.offered, added=self.offered - self.dropped_range - self.dropped_key,
                    dropped_range=self.dropped_range, dropped_key=self.dropped_key)

    def points(self, axes="loam"):
        return export(self.keys, self.vals, self.leaf, axes)


def export(keys, vals, leaf, axes="loam"):
    """records of the voxels (ascending keys, their n, Sx, Sy, Sz) as the library exports them: f64 arithmetic, one f32 rounding"""
    keys = np.asarray(keys, np.uint64)
    vals = np.asarray(vals, np.uint64)
    out = np.zeros((len(keys), 4), np.float32)
    leaf = np.float64(np.float32(leaf))   # (the configuration holds the leaf in f32)
    n = vals[:, 0].astype(np.float64)
    for a in range(3):
        ia = ((keys >> np.uint64(KBITS * a)) & np.uint64((1 << KBITS) - 1)).astype(np.int64) - (1 << QBITS)
        out[:, a] = ((ia.astype(np.float64) + vals[:, 1 + a].astype(np.float64) / (n * np.float64(1 << QBITS))) * leaf).astype(np.float32)
    out[:, 3] = n.astype(np.float32)
    if axes == "sensor":
        out = out[:, [2, 0, 1, 3]].copy()
    return out


def read_pcd(path):
    """(header dict, (n, 4) float32 body) of a binary PCD v0.7 file with fields x y z intensity"""
    raw = open(path, "rb").read()
    hdr, pos = {}, 0
    while True:
        end = raw.index(b"\n", pos)
        line = raw[pos:end].decode()
        pos = end + 1
        if line.startswith("#"):
            continue
        k, _, v = line.partition(" ")
        hdr[k] = v
        if k == "DATA":
            break
    n = int(hdr["POINTS"])
    body = np.frombuffer(raw[pos:], np.float32)
    assert body.size == 4 * n, (body.size, n)
    return hdr, body.reshape(n, 4)
