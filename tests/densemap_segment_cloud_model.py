"""Python model of loamx_densemap_segment_cloud and loamx_segments_match (include/loamx.h), a composition of the models that tests/
already has: cm.added_mask / dm.keys_of for admission and cells, the live dm.Model / cm.CarveModel for the map test, a fresh dm.Model
fed with the entered points, sm.segment on it, and the labels per point through the point's key.  The checker of
tests/test_densemap_segment_cloud_cpu.py and tests/test_gpu_densemap_segment_cloud.py."""
import numpy as np

import densemap_carve_model as cm
import densemap_model as dm
import densemap_segment_model as sm

NONE = sm.NONE
ALL, NEW, KNOWN = range(3)
LIM = sm.LIM
DEFAULTS = dict(which=NEW, margin=1, map_min_points=1, connectivity=26, min_points=1, min_voxels=1, lo=(-LIM,) * 3, hi=(LIM,) * 3)
STAT_KEYS = ("offered", "dropped_range", "dropped_key", "rejected", "entered", "voxels", "selected", "components", "kept", "kept_voxels",
             "largest", "labelled")   # the twelve exact words of stats


def check(cfg):
    """None when the configuration passes loamx_densemap_segment_cloud_check, otherwise the name of the first field that does not"""
    if not 0 <= cfg["which"] <= 2:
        return "which"
    if not 0 <= cfg["margin"] <= 2:
        return "margin"
    if cfg["map_min_points"] < 1:
        return "map_min_points"
    return sm.check(dict(which=sm.ALL, **{k: cfg[k] for k in ("connectivity", "min_points", "min_voxels", "lo", "hi")}))


def mapped_mask(live, map_min_points=1, rule=None):
    """per voxel of the live model, in live.keys order: is it mapped?  rule None: every voxel with enough points, else without those
    that (min_misses, num, den) calls dynamic (over a CarveModel)"""
    ok = live.vals[:, 0] >= np.uint64(map_min_points)
    if rule is not None:
        ok &= ~live.dynamic_mask(rule)
    return ok


def near_mask(keys, live, mapped, margin):
    """per key of `keys` (uint64, any order, repeats allowed): does a mapped voxel lie within `margin` cells (Chebyshev) of its cell?
    A cell with an index outside |i| < 2^20 does not exist and is not looked up"""
    uk, inv = np.unique(np.asarray(keys, np.uint64), return_inverse=True)
    m = np.uint64((1 << dm.KBITS) - 1)
    cells = np.stack([((uk >> np.uint64(dm.KBITS * a)) & m).astype(np.int64) - sm.IMAX for a in range(3)], axis=1)
    near = np.zeros(len(uk), bool)
    if len(live.keys) == 0 or len(uk) == 0:
        return near[inv.reshape(-1)]
    r = range(-margin, margin + 1)
    for dz in r:
        for dy in r:
            for dx in r:
                c = cells + np.array([dx, dy, dz], np.int64)
                exists = np.all(np.abs(c) < sm.IMAX, axis=1)
                cc = np.where(exists[:, None], c, 0) + sm.IMAX
                k = (cc[:, 0] | (cc[:, 1] << dm.KBITS) | (cc[:, 2] << (2 * dm.KBITS))).astype(np.uint64)
                at = np.minimum(np.searchsorted(live.keys, k), len(live.keys) - 1)
                near |= exists & (live.keys[at] == k) & mapped[at]
    return near[inv.reshape(-1)]


def segment_cloud(live, points, origin=(0.0, 0.0, 0.0), rule=None, **cfg):
    """(labels uint32 per point, records SEGMENT in ascending min_key, stats dict of STAT_KEYS, the fresh model that holds the
    entered points) of the cloud against the live model"""
    c = dict(DEFAULTS, **cfg)
    assert check(c) is None, check(c)
    points = np.asarray(points, np.float32)
    if points.size == 0:
        points = points.reshape(0, 4)
    n = len(points)
    keep, _ = cm.added_mask(points, origin, live.leaf, live.min_range, live.max_range) if n else (np.zeros(0, bool), None)
    keys, _, dr, dk = dm.keys_of(points, origin, live.leaf, live.min_range, live.max_range) if n else (np.zeros(0, np.uint64), None, 0, 0)
    admitted = np.flatnonzero(keep)
    assert len(admitted) == len(keys)
    if c["which"] == ALL:
        enter = np.ones(len(admitted), bool)
    else:
        near = near_mask(keys, live, mapped_mask(live, c["map_min_points"], rule), c["margin"])
        enter = near if c["which"] == KNOWN else ~near
    entered = admitted[enter]
    fresh = dm.Model(leaf=live.leaf, min_range=live.min_range, max_range=live.max_range)
    if len(entered):
        fresh.add(points[entered], origin)
        assert fresh.dropped_range == 0 and fresh.dropped_key == 0
    vlabels, rec, st = sm.segment(fresh, **{k: c[k] for k in ("connectivity", "min_points", "min_voxels", "lo", "hi")})
    labels = np.full(n, NONE, np.uint32)
    if len(entered):
        labels[entered] = vlabels[np.searchsorted(fresh.keys, keys[enter])]
    stats = dict(offered=n, dropped_range=dr, dropped_key=dk, rejected=len(admitted) - len(entered), entered=len(entered), voxels=len(fresh),
                 selected=st["selected"], components=st["components"], kept=st["kept"], kept_voxels=st["kept_voxels"], largest=st["largest"],
                 labelled=int((labels != NONE).sum()))
    return labels, rec, stats, fresh


def segments_match(prev, cur, gap=0):
    """loamx_segments_match in Python integers: uint32 per record of cur"""
    out = np.full(len(cur), NONE, np.uint32)
    for j in range(len(cur)):
        best, best_v = None, 0
        for i in range(len(prev)):
            v = 1
            for a in range(3):
                lo = max(int(prev[i]["lo"][a]) - gap, int(cur[j]["lo"][a]))
                hi = min(int(prev[i]["hi"][a]) + gap, int(cur[j]["hi"][a]))
                v *= max(hi - lo + 1, 0)
            if v == 0:
                continue
            if best is None or v > best_v or (v == best_v and int(prev[i]["min_key"]) < int(prev[best]["min_key"])):
                best, best_v = i, v
        if best is not None:
            out[j] = best
    return out
