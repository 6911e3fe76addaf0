"""numpy model of the dense map's regions, eviction and paging (include/loamx.h, loamx_densemap_region_* ... loamx_densemap_page), exact:
every compared quantity is an integer word or a byte string.  Built over the records of tests/densemap_file_model.py (records_of /
to_bytes / merge): a region selects records by the voxel indices in their keys, a file of selected records follows the header rule
(offered = the sum of n, every other statistic 0, flags, leaf and carving configuration kept), an evict splits a map into such a file
and the kept records, and page keeps a dict {tile: records} for the directory.  The checker of tests/test_densemap_region_cpu.py and
tests/test_gpu_densemap_region.py."""
import math

import numpy as np

import densemap_file_model as fm

IMAX = (1 << 20) - 1
INSIDE, OUTSIDE = 0, 1


def region(lo=(-IMAX,) * 3, hi=(IMAX,) * 3, side=INSIDE):
    return dict(lo=[int(v) for v in lo], hi=[int(v) for v in hi], side=int(side))


def clamp(v):
    return max(-IMAX, min(IMAX, int(v)))


def indices(keys):
    """(n, 3) int64: the voxel indices in the keys"""
    k = np.asarray(keys, np.uint64).reshape(-1)
    return np.stack([((k >> np.uint64(21 * a)) & np.uint64((1 << 21) - 1)).astype(np.int64) - (1 << 20) for a in range(3)], axis=1)


def key_of(idx):
    return sum((int(idx[a]) + (1 << 20)) << (21 * a) for a in range(3))


def mask_of(keys, reg):
    i = indices(keys)
    inside = np.all((i >= np.asarray(reg["lo"], np.int64)) & (i <= np.asarray(reg["hi"], np.int64)), axis=1)
    return inside if reg["side"] == INSIDE else ~inside


def _rows(r, m):
    return dict(keys=np.asarray(r["keys"], np.uint64)[m], vals=np.asarray(r["vals"], np.uint64).reshape(-1, 4)[m],
                miss=np.asarray(r["miss"], np.uint32)[m] if r["flags"] & fm.CARVING else None,
                mom=np.asarray(r["mom"], np.uint64).reshape(-1, 9)[m] if r["flags"] & fm.MOMENTS else None)


def region_file(r, m):
    """the header rule of a file of records taken out of a map: the rows m of r; offered = the sum of their n, the drop counts and the
    carve statistics 0, flags, leaf and the carving configuration as they are"""
    out = _rows(r, m)
    out.update(flags=r["flags"], leaf=r["leaf"], stats=(int(out["vals"][:, 0].sum(dtype=np.uint64)), 0, 0), carve_stats=(0,) * 6,
               carve=r["carve"])
    return out


def select(records, reg):
    """the records of loamx_densemap_save_region"""
    r = fm.records_of(records)
    return region_file(r, mask_of(r["keys"], reg))


def split(records, reg):
    """(removed, kept) of loamx_densemap_evict: removed is the file, kept the map afterwards (offered less the removed points, the
    other statistics as they were)"""
    r = fm.records_of(records)
    m = mask_of(r["keys"], reg)
    removed = region_file(r, m)
    kept = _rows(r, ~m)
    kept.update(flags=r["flags"], leaf=r["leaf"], stats=(r["stats"][0] - removed["stats"][0],) + tuple(r["stats"][1:]),
                carve_stats=r["carve_stats"], carve=r["carve"])
    return removed, kept


def counts(records, reg):
    s = select(records, reg)
    return len(s["keys"]), s["stats"][0]


def region_about(leaf, centre, half):
    """loamx_densemap_region_about: the inputs are f32, the arithmetic double"""
    lf = float(np.float32(leaf))
    c, h = [float(np.float32(v)) for v in centre], [float(np.float32(v)) for v in half]
    return region([clamp(math.floor((c[a] - h[a]) / lf)) for a in range(3)], [clamp(math.floor((c[a] + h[a]) / lf)) for a in range(3)])


def tile_of(idx, T):
    return tuple(int(i) // int(T) for i in idx)    # (Python's // rounds towards minus infinity)


def tile_region(tile, T):
    return region([clamp(t * T) for t in tile], [clamp(t * T + T - 1) for t in tile])


def tile_name(tile):
    return "tile_%d_%d_%d.lxdm" % tuple(tile)


def bucket(records, T):
    """{tile: file records} of the records by the tile of their voxel"""
    r = fm.records_of(records)
    tiles = indices(r["keys"]) // int(T)
    out = {}
    for t in sorted({tuple(int(v) for v in row) for row in tiles}):
        out[t] = region_file(r, np.all(tiles == np.asarray(t, np.int64), axis=1))
    return out


def page(resident, tiles, T, radius, centre):
    """loamx_densemap_page on the model: resident (records) and tiles ({tile: records}, the directory) -> (resident, tiles, stats)"""
    res = fm.records_of(resident)
    tiles = dict(tiles)
    lf = float(np.float32(res["leaf"]))
    ct = tile_of([clamp(math.floor(float(np.float32(c)) / lf)) for c in centre], T)
    lo, hi = [ct[a] - radius[a] for a in range(3)], [ct[a] + radius[a] for a in range(3)]
    stats = [0] * 6
    for t in sorted(tiles, key=lambda t: (t[2], t[1], t[0])):
        if all(lo[a] <= t[a] <= hi[a] for a in range(3)):
            f = tiles.pop(t)
            res = fm.merge(res, f)
            stats[0] += 1
            stats[1] += len(f["keys"])
    keep = region([clamp(lo[a] * T) for a in range(3)], [clamp(hi[a] * T + T - 1) for a in range(3)], OUTSIDE)
    removed, kept = split(res, keep)
    if len(removed["keys"]):
        for t, f in bucket(removed, T).items():
            if t in tiles:
                f = fm.merge(tiles[t], f)
                stats[4] += 1
            tiles[t] = f
            stats[2] += 1
        stats[3] = len(removed["keys"])
        res = kept
    stats[5] = len(res["keys"])
    return res, tiles, stats


def line(n, leaf, first=0, y=0.1, z=0.2):
    """n points, one per voxel, on a line along x from cell `first`"""
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = (first + np.arange(n) + 0.25) * leaf
    p[:, 1], p[:, 2] = y, z
    return p


def march(leaf, T, sweeps=6, blob=300, far=20, seed=7):
    """the paging scene: `sweeps` sweeps march along +x, one tile per sweep; each is a blob of `blob` points inside the vehicle's tile
    plus `far` points that land three tiles behind it, in the tile of the blob of three sweeps earlier, which a radius of one tile
    paged out two sweeps before (so the page-out meets a tile file that exists).  [(points, origin)], the vehicle's positions"""
    rng = np.random.default_rng(seed)
    out, centres = [], []
    span = T * leaf
    for k in range(sweeps):
        cx = (k + 0.5) * span
        p = np.zeros((blob + far, 4), np.float32)
        p[:blob, :3] = rng.uniform(-0.45 * span, 0.45 * span, (blob, 3)) + (cx, 0.5 * span, 0.5 * span)
        p[blob:, :3] = rng.uniform(-0.45 * span, 0.45 * span, (far, 3)) + (cx - 3 * span, 0.5 * span, 0.5 * span)
        out.append((p, (cx, 0.5 * span, 0.5 * span)))
        centres.append((cx, 0.5 * span, 0.5 * span))
    return out, centres


def model_from(records):
    """a model of the map (tests/densemap_model.py and its carving / moments kin) that holds the records, as a handle that loaded
    them: later adds go on from there.  Stamps are not in the records: 0, which no later call's sequence number equals"""
    import densemap_carve_model as cm
    r = fm.records_of(records)
    flags, leaf = r["flags"], float(r["leaf"])
    if flags & fm.CARVING:
        c = r["carve"]
        m = fm.model_of(flags, leaf, carve_max_range=float(c[0]), ray_stride=int(c[1]), end_margin=int(c[2]), max_steps=int(c[3]))
        m.miss = {int(k): int(v) for k, v in zip(r["keys"].tolist(), np.asarray(r["miss"]).tolist()) if v}
        m.stamp = {int(k): 0 for k in r["keys"].tolist()}
        m.cstats = dict(zip(cm.CARVE_KEYS, (int(v) for v in r["carve_stats"])))
    else:
        m = fm.model_of(flags, leaf)
    m.keys, m.vals = np.array(r["keys"], np.uint64), np.array(r["vals"], np.uint64).reshape(-1, 4)
    m.offered, m.dropped_range, m.dropped_key = (int(v) for v in r["stats"])
    if flags & fm.MOMENTS:
        m.mom = np.array(r["mom"], np.uint64).reshape(-1, 9)
    return m
