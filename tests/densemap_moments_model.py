"""numpy / Python model of the dense map's second moments and surfels (include/loamx.h, loamx_densemap_enable_moments and what follows
it): the nine integer words per voxel, exact (uint64 sums that wrap as the library's, the viewpoint terms from f32 arithmetic with the
library's roundings), and the surfel of a voxel from the exact integer scatter n*M_ab - S_a*S_b (Python integers) with
numpy.linalg.eigh in float64.  Built on tests/densemap_model.py and tests/densemap_carve_model.py, which stay the models of the map
and of carving.  The checker of tests/test_densemap_moments_cpu.py and tests/test_gpu_densemap_moments.py."""
import numpy as np

import densemap_carve_model as cm
import densemap_model as dm

F = np.float32
MOM_WORDS = 9
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # Mxx, Myy, Mzz, Mxy, Mxz, Myz
M64 = (1 << 64) - 1
DEFAULT_MIN_POINTS, DEFAULT_MIN_PLANAR_RATIO = 5, 0.01


def terms_of(points, origin, leaf, min_range=0.0, max_range=0.0):
    """(keys uint64, terms (n, 9) uint64) of the points the map keeps, in input order: the six products of q and the three w_a"""
    points = np.asarray(points, np.float32)
    keys, q, _, _ = dm.keys_of(points, origin, leaf, min_range, max_range)
    keep, _ = cm.added_mask(points, origin, leaf, min_range, max_range)
    assert len(keys) == int(keep.sum())
    d = np.ascontiguousarray(points[keep, :3]) - np.asarray(origin, np.float32)
    with np.errstate(over="ignore"):
        w = np.minimum(np.maximum(d * F(1024.0), F(-(1 << 30))), F(1 << 30)).astype(np.int64)   # (f32 product; truncated toward zero)
    t = np.zeros((len(keys), MOM_WORDS), np.uint64)
    for k, (a, b) in enumerate(PAIRS):
        t[:, k] = q[:, a] * q[:, b]
    t[:, 6:] = w.astype(np.uint64)   # (two's complement)
    return keys, t


class _Moments:
    """mix-in in front of densemap_model.Model or densemap_carve_model.CarveModel: self.mom, (n, 9) uint64 in the order of self.keys"""

    def add(self, points, origin):
        points = np.asarray(points, np.float32)
        old_keys = self.keys
        old_mom = getattr(self, "mom", np.zeros((0, MOM_WORDS), np.uint64))
        if not super().add(points, origin):
            return False
        keys, t = terms_of(points, origin, self.leaf, self.min_range, self.max_range)
        acc = np.zeros((len(self.keys), MOM_WORDS), np.uint64)
        acc[np.searchsorted(self.keys, old_keys)] = old_mom
        np.add.at(acc, np.searchsorted(self.keys, keys), t)   # (uint64: sums modulo 2^64)
        self.mom = acc
        return True

    def moments(self):
        return getattr(self, "mom", np.zeros((0, MOM_WORDS), np.uint64))

    def surfels(self, axes="loam", min_points=DEFAULT_MIN_POINTS, min_planar_ratio=DEFAULT_MIN_PLANAR_RATIO, keep=None):
        """((n, 8) float32 records, list of the per-voxel details of surfel_of), over the voxels of the mask keep (default: all)"""
        keep = np.ones(len(self.keys), bool) if keep is None else keep
        recs, infos = [], []
        for key, vals, mom in zip(self.keys[keep].tolist(), self.vals[keep].tolist(), self.moments()[keep].tolist()):
            r, info = surfel_of(self.leaf, idx_of(key), vals, mom, min_points, min_planar_ratio, axes)
            recs.append(r)
            infos.append(info)
        return np.array(recs, np.float32).reshape(-1, 8), infos


class MomentsModel(_Moments, dm.Model):
    """densemap_model.Model with moments enabled from the start"""


class CarveMomentsModel(_Moments, cm.CarveModel):
    """densemap_carve_model.CarveModel with moments enabled from the start"""

    def prune(self, rule=cm.DEFAULT_RULE):
        dyn = self.dynamic_mask(rule)
        self.mom = self.moments()[~dyn]
        return super().prune(rule)

    def static_surfels(self, rule, **kw):
        return self.surfels(keep=~self.dynamic_mask(rule), **kw)


def idx_of(key):
    """the voxel indices (ix, iy, iz) of a key"""
    return tuple(((int(key) >> (dm.KBITS * a)) & ((1 << dm.KBITS) - 1)) - cm.IMAX for a in range(3))


def words_of_q(q, w=None):
    """(vals, mom) as Python integers of a voxel that holds the points with the integer offsets q (n, 3) and viewpoint terms w (n, 3)"""
    q = [[int(x) for x in row] for row in q]
    w = [[0, 0, 0]] * len(q) if w is None else [[int(x) for x in row] for row in w]
    vals = [len(q)] + [sum(r[a] for r in q) for a in range(3)]
    mom = [sum(r[a] * r[b] for r in q) & M64 for a, b in PAIRS] + [sum(r[a] for r in w) & M64 for a in range(3)]
    return vals, mom


def scatter_of(vals, mom):
    """the exact integer N_ab = n*M_ab - S_a*S_b as a 3x3 list of Python integers"""
    n, s = int(vals[0]), [int(v) for v in vals[1:4]]
    N = [[0] * 3 for _ in range(3)]
    for k, (a, b) in enumerate(PAIRS):
        N[a][b] = N[b][a] = n * int(mom[k]) - s[a] * s[b]
    return N


def surfel_of(leaf, idx, vals, mom, min_points=DEFAULT_MIN_POINTS, min_planar_ratio=DEFAULT_MIN_PLANAR_RATIO, axes="loam"):
    """((8,) float32 record, details): details has `has` (the voxel has a surfel), `lam` (ascending eigenvalues, float64), `normal`
    (float64, signed; LOAM frame), `dot` (normal . V before the flip decided it, as |.|), `v` (the signed V)"""
    n = int(vals[0])
    N = scatter_of(vals, mom)
    v = [int(x) - (1 << 64) if int(x) >> 63 else int(x) for x in mom[6:9]]
    key = sum((int(idx[a]) + cm.IMAX) << (dm.KBITS * a) for a in range(3))
    rec = np.zeros(8, np.float32)
    rec[:4] = dm.export([key], [[int(x) for x in vals]], leaf, axes)[0]
    info = dict(has=False, lam=None, normal=np.zeros(3), dot=0.0, v=v)
    if n >= min_points and N[0][0] + N[1][1] + N[2][2] > 0:
        nn = float(n) * float(n)
        C = np.array([[float(N[a][b]) / nn for b in range(3)] for a in range(3)], np.float64)
        lam, vec = np.linalg.eigh(C)
        info["lam"] = lam
        if lam[1] >= float(F(min_planar_ratio)) * lam[2]:
            e = vec[:, 0].copy()
            dot = (e[0] * float(v[0]) + e[1] * float(v[1])) + e[2] * float(v[2])
            flip = dot > 0.0
            if dot == 0.0:
                flip = e[np.flatnonzero(e)[0]] < 0.0
            e = -e if flip else e
            info.update(has=True, normal=e, dot=abs(dot))
            o = [2, 0, 1] if axes == "sensor" else [0, 1, 2]
            rec[4:7] = e[o].astype(np.float32)
            rec[7] = F(lam[0] / ((lam[0] + lam[1]) + lam[2]))
    return rec, info
