"""Python model of the dense map's coarser levels and of the coarse-to-fine alignment (include/loamx.h, loamx_densemap_coarsen and what
follows it).  coarsen_once() / cascade(): the thirteen words of a level from the level below, in Python integers, restating the
header's per-child expressions; the sums wrap modulo 2^64 as the library's words do.  frozen_of_level(): the entries of a level's
snapshot from its words.  align_pyramid(): the loop of densemap_align_model.align level by level.  Built on tests/densemap_model.py,
tests/densemap_moments_model.py and tests/densemap_align_model.py, which stay the models of the map, its surfels and the alignment.
The checker of tests/test_densemap_pyramid_cpu.py and tests/test_gpu_densemap_pyramid.py.

How far a coarse voxel's exported position is from the mean of the points it holds.  A child's S_a enters its parent as
(S_a >> 1) + n b_a 2^19: one floor per child and word, an error in [0, 1) units of the parent's leaf_l / 2^20.  A parent has at most
eight children, so level 1 is short by fewer than 8 units in each S'_a.  The error a child already carries is halved with its S (the
parent's unit is twice the child's), so with E_l the bound at level l:  E_1 < 8,  E_l < E_(l-1) / 2 + 8,  hence E_l < 16 at every
level.  The exported position is (I + S' / (n 2^20)) leaf_l, so it lies below the n-weighted mean of the level-0 voxels' exact means
by fewer than 16 leaf_l / (2^20 n) per axis (position_bound()), and never above it.  The export rounds once to f32 and so does every
level-0 record the mean is taken from: together at most one f32 spacing at the largest coordinate involved."""
import numpy as np

import densemap_align_model as am
import densemap_model as dm
import densemap_moments_model as mm

F = np.float32
M64 = mm.M64
IMAX = 1 << dm.QBITS
MAX_LEVELS = 6
FIELD = (1 << dm.KBITS) - 1


def indices_of(key):
    return [((int(key) >> (dm.KBITS * a)) & FIELD) - IMAX for a in range(3)]


def key_of(idx):
    return sum((int(idx[a]) + IMAX) << (dm.KBITS * a) for a in range(3))


def level_leaf(leaf, level):
    """the leaf of a level as the library computes it: one f32 multiply by a power of two"""
    return float(F(leaf) * F(1 << level))


def coarsen_once(keys, vals, mom, keep=None):
    """(keys (m,) uint64 ascending, vals (m, 4) uint64, mom (m, 9) uint64) of the level above the voxels given (those of the mask keep,
    default all)"""
    keys, vals, mom = np.asarray(keys, np.uint64), np.asarray(vals, np.uint64).reshape(-1, 4), np.asarray(mom, np.uint64).reshape(-1, 9)
    keep = np.ones(len(keys), bool) if keep is None else np.asarray(keep, bool)
    acc = {}
    for key, v, m in zip(keys[keep].tolist(), vals[keep].tolist(), mom[keep].tolist()):
        i = indices_of(key)
        b = [x & 1 for x in i]
        parent = key_of([x >> 1 for x in i])    # (Python's >> is arithmetic: floor for negative indices)
        n, S = v[0], v[1:4]
        w = acc.setdefault(parent, [0] * 13)
        w[0] += n
        for a in range(3):
            w[1 + a] += (S[a] >> 1) + n * b[a] * (1 << 19)
        for k, (a, c) in enumerate(mm.PAIRS):
            w[4 + k] += (m[k] >> 2) + b[a] * (1 << 18) * S[c] + b[c] * (1 << 18) * S[a] + n * b[a] * b[c] * (1 << 38)
        for a in range(3):
            w[10 + a] += m[6 + a]    # (two's complement words: the sum modulo 2^64 is the signed sum)
    out_keys = np.array(sorted(acc), np.uint64)
    words = np.array([[x & M64 for x in acc[int(k)]] for k in out_keys.tolist()], np.uint64).reshape(-1, 13)
    return out_keys, np.ascontiguousarray(words[:, :4]), np.ascontiguousarray(words[:, 4:])


def cascade(keys, vals, mom, levels, keep=None):
    """[(keys, vals, mom) of level 1, ..., of level `levels`]; keep: the mask of the level-0 voxels that enter level 1"""
    out = []
    for l in range(levels):
        keys, vals, mom = coarsen_once(keys, vals, mom, keep if l == 0 else None)
        out.append((keys, vals, mom))
    return out


def surfels_of_level(leaf_l, keys, vals, mom, min_points=mm.DEFAULT_MIN_POINTS, min_planar_ratio=mm.DEFAULT_MIN_PLANAR_RATIO):
    """(n, 8) float32: the model's surfel of every voxel of a level whose leaf is leaf_l"""
    recs = [mm.surfel_of(leaf_l, mm.idx_of(k), v, m, min_points, min_planar_ratio)[0]
            for k, v, m in zip(np.asarray(keys).tolist(), np.asarray(vals).tolist(), np.asarray(mom).tolist())]
    return np.array(recs, np.float32).reshape(-1, 8)


def frozen_of_level(keys, surfels, max_curvature=0.0):
    """(keys, (m, 6) float32 records) of a coarse level's snapshot: the voxels that have a normal and, with max_curvature > 0, a
    curvature that is not larger"""
    keys, surfels = np.asarray(keys, np.uint64), np.asarray(surfels, np.float32).reshape(-1, 8)
    ok = surfels[:, 4:7].any(axis=1)
    if max_curvature > 0:
        ok &= ~(surfels[:, 7] > F(max_curvature))
    return keys[ok], np.ascontiguousarray(surfels[ok][:, [0, 1, 2, 4, 5, 6]])


def position_bound(leaf_l, n):
    """how far below the n-weighted mean of its points' level-0 means a coarse voxel's position may lie, per axis, before the f32
    roundings (the module's docstring)"""
    return 16.0 * leaf_l / (float(1 << dm.QBITS) * np.asarray(n, np.float64))


def align_pyramid(tables, points, pose_in, leaf, first_level=None, centre=None, **cfg):
    """loamx_densemap_align_pyramid: tables[l] = (keys, records) of level l's snapshot; the results of the levels first_level .. 0 in
    that order, each the model loop from the pose the level before reported"""
    first_level = len(tables) - 1 if first_level is None else first_level
    out, pose = [], np.asarray(pose_in, np.float64).reshape(3, 4)
    for l in range(first_level, -1, -1):
        keys, recs = tables[l]
        r = am.align(keys, recs, points, pose, level_leaf(leaf, l), centre=centre, **cfg)
        out.append(r)
        pose = r["pose"]
    return out


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
DYADIC_LEAF = 0.25
DYADIC_ORIGIN = (0.5, 0.25, -0.125)


def dyadic_cloud(n=3000, seed=5, leaf=DYADIC_LEAF):
    """n points whose coordinates are integer multiples of leaf / 1024 within +-40 leaves (negative indices included): their offsets
    are multiples of 2^10, so no floor of three levels of coarsening drops a bit; (n, 4) float32"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = rng.integers(-40 * 1024, 40 * 1024, (n, 3)).astype(np.float64) * (leaf / 1024.0)
    return out


BASIN_LEAF = 0.25


def basin_start(truth):
    """the start of the basin case: the truth turned by exp_so3([0.1, 0.1, -0.15]) and moved by (-1.2, 0.8, 0.5) m"""
    P = np.asarray(truth, np.float64).reshape(3, 4)
    return np.concatenate([am.exp_so3([0.1, 0.1, -0.15]) @ P[:, :3], (P[:, 3] + np.array([-1.2, 0.8, 0.5]))[:, None]], axis=1)
