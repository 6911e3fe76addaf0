"""Designed voxels for the device-side surfel (loam_velodyne_amd/csrc/densemap_surfel.hpp, k_dm_surfels), shared by
tests/test_densemap_freeze_cpu.py and tests/test_gpu_densemap_freeze.py.

POINT_CASES are voxels given as points: integer offsets q inside a voxel of a map of leaf 0.5 and a sensor origin, so that every
coordinate is exact in f32 (|index| < 8: three integer bits and twenty fraction bits) and the map's words follow from the points by
the model (tests/densemap_moments_model.py).  The CPU test takes the model's words; the GPU test adds the points, checks that the
device holds those words, and freezes.  WORD_CASES are voxels given as words only: the word sets that test_densemap_moments_cpu.py
builds from formulas and the scatter integers whose conversion to double is a tie, which are not the sums of a point set we know of;
the GPU test puts those on the device as words, through a map file.
"""
import numpy as np

import densemap_moments_model as mm

LEAF = 0.5
Q = (1 << 20) - 1


def case_index(k):
    """the voxel of point case k: distinct voxels with |index| < 8"""
    return ((k % 5) * 3 - 7, ((k // 5) % 5) * 3 - 7, (k // 25) * 3 - 7)


def points_of(idx, q):
    """(n, 4) float32, exact: offsets q (n, 3) inside voxel idx at leaf 0.5"""
    q = np.asarray(q, np.int64).reshape(-1, 3)
    p = np.zeros((len(q), 4), np.float32)
    p[:, :3] = ((np.asarray(idx, np.float64) + q / float(1 << 20)) * LEAF).astype(np.float32)
    assert np.array_equal(np.floor(p[:, :3].astype(np.float64) / LEAF), np.broadcast_to(np.asarray(idx, np.float64), (len(q), 3)))
    return p


def origin_of(idx, q):
    """the sensor origin at offsets q (may lie outside [0, 2^20): another voxel) relative to voxel idx, exact in f32"""
    return ((np.asarray(idx, np.float64) + np.asarray(q, np.float64) / float(1 << 20)) * LEAF).astype(np.float32)


def _point_cases():
    rng = np.random.default_rng(20250)
    out = []   # (name, q (n, 3), origin offsets (3,), min_points or None, min_planar_ratio or None)
    low, high = (-3 << 20, -2 << 20, -5 << 20), (4 << 20, 3 << 20, 6 << 20)
    out.append(("one point", [[5, 6, 7]], low, None, None))
    out.append(("two points", [[5, 6, 7], [900, 10, 20]], low, 3, None))
    q5 = rng.integers(0, Q + 1, (5, 3))
    out.append(("n == min_points", q5, low, None, None))
    out.append(("n == min_points - 1", q5[:4], low, None, None))
    out.append(("n == 4 with min_points 4", q5[:4], high, 4, None))
    out.append(("eight equal points", [[Q, 3, 9]] * 8, low, None, None))
    out.append(("collinear", [[100 + 1000 * k, 7 + 2000 * k, 90000 + 3000 * k] for k in range(10)], low, None, None))
    out.append(("collinear, three points", [[100 + 1000 * k, 7 + 2000 * k, 90000 + 3000 * k] for k in range(3)], high, 3, None))
    out.append(("along one axis", [[5, 1000 * k * k, 77] for k in range(10)], low, None, None))
    for axis in range(3):
        q = rng.integers(0, Q + 1, (40, 3))
        q[:, axis] = 123456
        inplane = [500000, 400000, 300000]
        inplane[axis] = 123456   # the origin lies in the plane: the dot product is exactly 0
        for name, o in (("low side", low), ("high side", high), ("origin in the plane", inplane)):
            out.append((f"coplanar on axis {axis}, {name}", q, o, None, None))
    a = 2 * rng.integers(0, 200000, 60)
    b = rng.integers(0, 200000, 60)
    q = np.stack([a, b, a // 2 + b + 1000], axis=1)   # x + 2 y - 2 z = -2000: unit normal (1, 2, -2) / 3
    out.append(("tilted plane, low side", q, low, None, None))
    out.append(("tilted plane, high side", q, high, None, None))
    blob = rng.integers(0, Q + 1, (500, 3))
    out.append(("isotropic blob", blob, low, None, None))
    out.append(("isotropic blob, demanding ratio", blob, high, None, 0.5))
    thin = blob.copy()
    thin[:, 1] //= 16
    thin[:, 2] //= 256
    out.append(("elongated, demanding ratio", thin, low, None, 0.5))
    out.append(("elongated, ratio 0", thin, high, None, 0.0))
    slab = rng.integers(0, Q + 1, (200, 3))
    slab[:, 1] = 500000 + rng.integers(-3000, 3000, 200)
    out.append(("slab across y, seen from below", slab, (100000, -(3 << 20), 200000), None, None))
    out.append(("slab across y, seen from above", slab, (100000, 4 << 20, 200000), None, None))
    # V = (0, 0, 0): the points come in pairs c + d, c - d and the sensor stands at c, so the truncated w_a cancel exactly and the
    # sign of the normal is decided by its first non-zero component
    c = np.array([524288, 524288, 524288])
    d = np.stack([rng.integers(-200000, 200000, 20), rng.integers(-200000, 200000, 20), rng.integers(-300, 300, 20)], axis=1)
    d[:, 2] += d[:, 0] // 7
    out.append(("symmetric about the origin, V = 0", np.concatenate([c + d, c - d]), c, None, None))
    d2 = d[:, [2, 0, 1]]
    out.append(("symmetric about the origin, V = 0, thin along x", np.concatenate([c + d2, c - d2]), c, None, None))
    # two equal eigenvalues: the scatter is exactly diag(12 d^2, 12 d^2, 12 e^2); ties keep the index order
    for name, dd, ee in (("the two smallest equal", 20000, 70000), ("the two largest equal", 70000, 20000)):
        q = [c + s * np.array(v) for v in ((dd, 0, 0), (0, dd, 0), (0, 0, ee)) for s in (1, -1)]
        out.append((f"a cross, {name}", q, low, None, None))
        out.append((f"a cross, {name}, V = 0", q, c, None, None))
    # 65,536 points with offsets near 2^20 - 1: n * M is near 2^72, the scatter passes through the high word
    r = rng.integers(0, 64, (65536, 2))
    out.append(("65536 points near the far corner", np.stack([Q - r[:, 0], Q - r[:, 1], Q - (r[:, 0] + 2 * r[:, 1]) // 3 - rng.integers(0, 2, 65536)],
                                                             axis=1), low, None, None))
    return out


def point_cases():
    """[dict(name, idx, points (n, 4) f32, origin (3,) f32, vals [4], mom [9], min_points, min_planar_ratio)]: the words are the
    model's for an add of `points` with `origin` into a map of leaf 0.5"""
    out = []
    for k, (name, q, o, mp, ratio) in enumerate(_point_cases()):
        idx = case_index(k)
        pts, origin = points_of(idx, q), origin_of(idx, o)
        m = mm.MomentsModel(leaf=LEAF)
        m.add(pts, origin)
        assert len(m.keys) == 1 and mm.idx_of(m.keys[0]) == idx, name
        out.append(dict(name=name, idx=idx, points=pts, origin=origin, vals=[int(v) for v in m.vals[0]], mom=[int(v) for v in m.moments()[0]],
                        min_points=mp, min_planar_ratio=ratio))
    return out


def _solve_words(diag_floor, off, base):
    """vals, six M words (Python integers, 0 <= M < 2^64) of the smallest n in 3 .. 11 and sums S_a = base + 0 .. 39 (base^2 above every
    |off|, so that a negative scatter integer has a non-negative M) for which the three off-diagonal scatter integers
    n * M_ab - S_a * S_b are exactly off = (Nxy, Nxz, Nyz); the diagonal ones are the smallest that are >= diag_floor"""
    for n in range(3, 12):
        for s in range(40):
            for t in range(40):
                for u in range(40):
                    S = (base + s, base + t, base + u)
                    if all((off[k] + S[a] * S[b]) % n == 0 for k, (a, b) in enumerate(mm.PAIRS[3:])):
                        m6 = [-((-(diag_floor + S[a] * S[a])) // n) for a in range(3)] + [(off[k] + S[a] * S[b]) // n
                                                                                       for k, (a, b) in enumerate(mm.PAIRS[3:])]
                        if all(0 <= m < 1 << 64 for m in m6):
                            return [n, S[0], S[1], S[2]], m6
    raise AssertionError("no words for these targets")


def word_cases():
    """[dict(name, idx, vals, mom, min_points, min_planar_ratio)] given as words only"""
    out = []
    # the 128-bit path of test_densemap_moments_cpu.py: 2^24 - 1 points on three corners, n * Mxx about 2^86
    n = (1 << 24) - 1
    k = [n // 3 + 5, n // 3 - 1000, n - 2 * (n // 3) + 995]
    out.append(dict(name="2^24 - 1 points on three corners", idx=(1 << 19, -(1 << 19), 0), vals=[n] + [x * Q for x in k],
                    mom=[x * Q * Q for x in k] + [0, 0, 0, 3 * n, 5 * n, (-2 * n) % (1 << 64)], min_points=None, min_planar_ratio=None))
    k2 = [k[0] - 1, k[1] + 1, k[2] + 1]
    out.append(dict(name="2^24 - 1 points, one on a fourth corner", idx=(0, 0, 0), vals=[n] + [x * Q for x in k2],
                    mom=[x * Q * Q for x in k2] + [0, 0, Q * Q, 3 * n, 5 * n, (-2 * n) % (1 << 64)], min_points=None, min_planar_ratio=None))
    # scatter integers whose conversion to double is a tie.  Below 2^54 the spacing of the doubles is 2: 2^53 + 1 lies halfway and goes
    # DOWN to the even 2^53, 2^53 + 3 goes UP to 2^53 + 4.  From 2^64 on the integer has a high word and the spacing is 2^12:
    # 2^64 + 2^11 goes down, 2^64 + 3 * 2^11 goes up.  The negatives stand on the off-diagonals
    lo_dn, lo_up, hi_dn, hi_up = (1 << 53) + 1, (1 << 53) + 3, (1 << 64) + (1 << 11), (1 << 64) + 3 * (1 << 11)
    for name, floor, off, base in (("ties just above 2^53", 4 * lo_up, (-lo_dn, lo_up, -lo_up), 1 << 27),
                                   ("ties just above 2^53, signs swapped", 4 * lo_up, (lo_dn, -lo_up, lo_dn), 1 << 27),
                                   ("ties just above 2^64", 4 * hi_up, (-hi_dn, hi_up, -hi_up), 3 << 31),
                                   ("ties just above 2^64, signs swapped", 4 * hi_up, (hi_up, -hi_dn, hi_dn), 3 << 31)):
        vals, m6 = _solve_words(floor, off, base)
        N = mm.scatter_of(vals, m6 + [0, 0, 0])
        assert (N[0][1], N[0][2], N[1][2]) == off and min(N[0][0], N[1][1], N[2][2]) >= floor and max(m6) < 1 << 64
        out.append(dict(name=name, idx=(3, -2, 1), vals=vals, mom=m6 + [7, (-9) % (1 << 64), 4], min_points=3, min_planar_ratio=0.0))
    return out


def random_cases(count, seed):
    """`count` voxels of 1 .. 60 random points each in random shapes (blob, slab, rod), random indices and viewpoints, as words"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(1, 61))
        scale = np.array([1 << 19] * 3)
        shape = int(rng.integers(0, 4))
        if shape >= 1:
            scale[int(rng.integers(0, 3))] = int(rng.integers(1, 4000))
        if shape == 3:
            scale[int(rng.integers(0, 3))] = int(rng.integers(1, 4000))
        q = np.clip((1 << 19) + (rng.normal(size=(n, 3)) * scale / 3).astype(np.int64), 0, Q)
        w = rng.integers(-60000, 60000, (1, 3)) + rng.integers(-2000, 2000, (n, 3))
        vals = [n] + [int(v) for v in q.sum(axis=0)]
        mom = [int((q[:, a] * q[:, b]).sum()) for a, b in mm.PAIRS] + [int(v) % (1 << 64) for v in w.sum(axis=0)]
        out.append(dict(name="random", idx=tuple(int(v) for v in rng.integers(-(1 << 20) + 1, 1 << 20, 3)), vals=vals, mom=mom,
                        min_points=int(rng.integers(3, 8)), min_planar_ratio=float(rng.choice([0.0, 0.01, 0.2]))))
    return out
