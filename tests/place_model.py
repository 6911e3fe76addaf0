"""numpy model of the place-recognition database (include/loamx.h, loamx_place_*), exact to the bit: the scan-context descriptor, its ring
key, the shift-minimised column-cosine distance and the search, in f32 with the roundings and the summation orders of the header's
definition (the library is built with -ffp-contract=off).  The checker of tests/test_place_cpu.py and tests/test_gpu_place.py (place
recognition is not in the reference, so there is no oracle for it) — and the builder of the revisit cases both of them use."""
import functools
import math

import numpy as np

F = np.float32


@functools.lru_cache(maxsize=None)
def sector_table(S):
    """(S, 2) f32: the boundary directions (cos, sin)(2 pi k / S), evaluated in double (the C library's cos / sin)"""
    return np.array([[math.cos(2.0 * math.pi * k / S), math.sin(2.0 * math.pi * k / S)] for k in range(S)], np.float64).astype(F)


def cells_of(points, origin=(0, 0, 0), R=20, S=60, max_range=80.0, min_range=0.0, height_offset=2.0):
    """per point: (used, ring, sector, h, ambiguous); sector -1 = no sector qualifies (the point is dropped); ambiguous = more than one
    qualifies (the smallest is taken; counted by the test that claims the rule names exactly one sector on real sweeps)"""
    p = np.ascontiguousarray(np.asarray(points, F)[:, :3])
    o = np.asarray(origin, F)
    tab = sector_table(S)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p - o
        a, b = d[:, 2], d[:, 0]
        r2 = a * a + b * b
        h = d[:, 1] + F(height_offset)
        used = np.isfinite(p).all(axis=1) & (r2 >= F(min_range) * F(min_range)) & (r2 < F(max_range) * F(max_range)) & (h > 0)
        ring_scale = F(R) / F(max_range)
        t = np.sqrt(r2) * ring_scale
        ring = np.minimum(np.where(used, t, 0).astype(np.int64), R - 1)
        cross = tab[None, :, 0] * b[:, None] - tab[None, :, 1] * a[:, None]     # (n, S): two rounded products, one subtraction
        ok = (cross >= 0) & (np.roll(cross, -1, axis=1) < 0)
    nq = ok.sum(axis=1)
    sector = np.where(nq > 0, ok.argmax(axis=1), -1)
    used = used & (sector >= 0)
    ambiguous = used & (nq > 1)
    return used, ring, sector, h, ambiguous


def descriptor(points, origin=(0, 0, 0), R=20, S=60, max_range=80.0, min_range=0.0, height_offset=2.0):
    """(R, S) f32: the maximum height per cell, 0 where empty"""
    D = np.zeros((R, S), F)
    if len(points):
        used, ring, sector, h, _ = cells_of(points, origin, R, S, max_range, min_range, height_offset)
        np.maximum.at(D, (ring[used], sector[used]), h[used])
    return D


def ring_key(D):
    """(..., R) f32: the row sums in ascending k, one f32 addition at a time, over (float)S"""
    D = np.asarray(D, F)
    acc = np.zeros(D.shape[:-1], F)
    for k in range(D.shape[-1]):
        acc = acc + D[..., k]
    return acc / F(D.shape[-1])


def ring_key_distance(rq, rc):
    """sum_i (rq[i] - rc[i])^2 in ascending i; rc may be (n, R)"""
    rq, rc = np.asarray(rq, F), np.asarray(rc, F)
    acc = np.zeros(rc.shape[:-1], F)
    for i in range(rc.shape[-1]):
        t = rq[..., i] - rc[..., i]
        acc = acc + t * t
    return acc


def col_norms(D):
    D = np.asarray(D, F)
    acc = np.zeros(D.shape[:-2] + D.shape[-1:], F)
    for i in range(D.shape[-2]):
        acc = acc + D[..., i, :] * D[..., i, :]
    return np.sqrt(acc)


def distances(Q, Cs):
    """d(s) of Q (R, S) against every C of Cs (n, R, S): (n, S) f32"""
    Q, Cs = np.asarray(Q, F), np.asarray(Cs, F)
    n, R, S = Cs.shape
    out = np.zeros((n, S), F)
    nq = col_norms(Q)
    jj = (np.arange(S)[None, :] + np.arange(S)[:, None]) % S     # jj[s][j] = (j + s) mod S
    j0 = np.broadcast_to(np.arange(S)[None, :], (S, S))
    for lo in range(0, n, 256):
        C = Cs[lo:lo + 256]
        nc = col_norms(C)
        T = np.zeros((len(C), S, S), F)                           # T[c][j][j'] = sum_i Q[i][j] * C[i][j'], i ascending
        for i in range(R):
            T = T + Q[i][None, :, None] * C[:, i, None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            V = T / (nq[None, :, None] * nc[:, None, :])
        valid = (nq[None, :, None] > 0) & (nc[:, None, :] > 0)
        Vs, ok = V[:, j0, jj], valid[:, j0, jj]                   # (c, s, j)
        acc = np.zeros(Vs.shape[:2], F)
        for j in range(S):
            acc = np.where(ok[:, :, j], acc + Vs[:, :, j], acc)
        cnt = ok.sum(axis=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = F(1.0) - acc / cnt.astype(F)
        out[lo:lo + 256] = np.where(cnt > 0, d, F(1.0))
    return out


def pair_distance(Q, C):
    """(distance, shift) of one pair: the smallest d(s), ties to the smaller s"""
    d = distances(Q, np.asarray(C, F)[None])[0]
    s = int(np.argmin(d))
    return d[s], s


class Model:
    def __init__(self, R=20, S=60, max_range=80.0, min_range=0.0, height_offset=2.0, n_candidates=0, exclude_recent=50, max_entries=0):
        self.R, self.S, self.max_range, self.min_range, self.height_offset = R, S, max_range, min_range, height_offset
        self.K, self.exclude_recent, self.max_entries = n_candidates, exclude_recent, max_entries
        self.desc, self.keys = [], []

    def __len__(self):
        return len(self.desc)

    def describe(self, points, origin=(0, 0, 0)):
        D = descriptor(points, origin, self.R, self.S, self.max_range, self.min_range, self.height_offset)
        return D, ring_key(D)

    def add(self, points, origin=(0, 0, 0)):
        """the new entry's id, or None when max_entries refuses it"""
        if self.max_entries and len(self.desc) + 1 > self.max_entries:
            return None
        D, k = self.describe(points, origin)
        self.desc.append(D)
        self.keys.append(k)
        return len(self.desc) - 1

    def reset(self):
        self.desc, self.keys = [], []

    def candidates(self, rq, q, exclude_recent):
        """ids searched for a query with id q: id + exclude_recent < q, cut to the K smallest by (ring-key distance, id) with K > 0"""
        ids = np.arange(max(min(q - exclude_recent, len(self.desc)), 0))
        if not len(ids):
            return ids, np.zeros(0, F)
        rkd = ring_key_distance(rq, np.stack(self.keys)[ids])
        if self.K > 0 and len(ids) > self.K:
            order = np.lexsort((ids, rkd))[:self.K]
            sel = np.sort(order)
            ids, rkd = ids[sel], rkd[sel]
        return ids, rkd

    def search(self, Q, rq, q, exclude_recent, n_results, only=None):
        """[(id, shift, distance, ring_key_distance)]: the n_results best candidates by (distance, id); only: restrict to these ids"""
        ids, rkd = self.candidates(rq, q, exclude_recent)
        if only is not None:
            keep = np.isin(ids, only)
            ids, rkd = ids[keep], rkd[keep]
        if not len(ids):
            return []
        d = distances(Q, np.stack(self.desc)[ids])
        sh = d.argmin(axis=1)
        best = d[np.arange(len(ids)), sh]
        order = np.lexsort((ids, best))[:n_results]
        return [(int(ids[c]), int(sh[c]), best[c], rkd[c]) for c in order]

    def query_entry(self, q, n_results=5, only=None):
        return self.search(self.desc[q], self.keys[q], q, self.exclude_recent, n_results, only)

    def query(self, points, origin=(0, 0, 0), exclude_recent=0, n_results=5, only=None):
        D, k = self.describe(points, origin)
        return self.search(D, k, len(self.desc), exclude_recent, n_results, only)


# ---- the revisit cases of tests/test_place_cpu.py and tests/test_gpu_place.py ----------------------------------------------------------
# (k, yaw of the query relative to entry k in degrees, displacement +off in x and -off in z)
REVISITS = ((10, 90.0, 0.5), (25, 180.0, 1.0), (5, -48.0, 0.3))
_REVISIT_CACHE = {}


def revisit_case(sensor="HDL-64E", az_steps=1024, n=40):
    """(database sweeps, [(k, dyaw_deg, query sweep)]): n sweeps taken at rest at the poses of synth.trajectory(n, step=2.5,
    yaw_step_deg=1.0) in synth.World(half_extent=125) (range noise seed k), and the REVISITS queries (noise seed 100 + k; sensor-frame
    clouds, origin 0)"""
    key = (sensor, az_steps, n)
    if key not in _REVISIT_CACHE:
        from loam_velodyne_amd import synth
        w = synth.World(half_extent=125.0)
        poses = synth.trajectory(n, step=2.5, yaw_step_deg=1.0)
        db = [synth.make_sweep(w, sensor, poses[k], poses[k], seed=k, az_steps=az_steps).points for k in range(n)]
        qs = []
        for k, dyaw, off in REVISITS:
            pose = poses[k].copy()
            pose[1] += np.deg2rad(dyaw)
            pose[3] += off
            pose[5] -= off
            qs.append((k, dyaw, synth.make_sweep(w, sensor, pose, pose, seed=100 + k, az_steps=az_steps).points))
        _REVISIT_CACHE[key] = (db, qs)
    return _REVISIT_CACHE[key]
