"""numpy / Python model of the dense map's distance field (include/loamx.h, loamx_densemap_dist and loamx_densemap_dist_query), exact to
the bit: the definition by brute force over every occupied cell of the window, on the keys / vals of a tests/densemap_model.py Model (a
rule needs a tests/densemap_carve_model.py CarveModel), integers throughout; a second, separable statement of the same field (three
passes, each with the tie it owns), which tests/test_densemap_dist_cpu.py holds against the first; and the query's cell of a point in
f32, as densemap_model.keys_of computes the voxel.  The checker of tests/test_densemap_dist_cpu.py and tests/test_gpu_densemap_dist.py."""
import numpy as np

import densemap_carve_model as cm
import densemap_grid_model as gm
import densemap_model as dm

NONE = 0xffffffff      # near of a capped cell
OUTSIDE = 0xffffffff   # d2 of a point without a cell in the window
DEFAULTS = dict(cell_leaves=2, x0=0, y0=0, z0=0, nx=128, ny=32, nz=128, min_points=2, d_max=16)
DIST_SAMPLE = np.dtype([("d2", "<u4"), ("near", "<u4")])
STATS = ("voxels", "occupied", "within", "max_d2")
QUERY_STATS = ("inside", "outside", "capped", "below", "best")


def check(c):
    """the name of the first field of the configuration (a dict with every key of DEFAULTS) that is out of its bounds, or None"""
    if not 1 <= c["cell_leaves"] <= 64:
        return "cell_leaves"
    for f in ("x0", "y0", "z0"):
        if abs(c[f]) > 1 << 21:
            return f
    for f in ("nx", "ny", "nz"):
        if not 1 <= c[f] <= 1024:
            return f
    if c["nx"] * c["ny"] * c["nz"] > 1 << 26:
        return "nx * ny * nz"
    if c["min_points"] < 1:
        return "min_points"
    if not 0 <= c["d_max"] <= 254:
        return "d_max"
    return None


window = gm.window   # (first cell, count) of one axis of loamx_densemap_dist_window: the grid's expression


def pack(rx, ry, rz):
    return rx | (ry << 10) | (rz << 20)


def unpack(near):
    return near & 1023, (near >> 10) & 1023, near >> 20


def occupied(model, rule=None, **cfg):
    """(occ, voxels): the (nz, ny, nx) bool volume of the occupied cells, and the number of qualifying voxels inside the window"""
    c = dict(DEFAULTS, **cfg)
    assert set(c) == set(DEFAULTS) and check(c) is None, check(c)
    assert rule is None or (rule[2] != 0 and hasattr(model, "miss"))
    k = c["cell_leaves"]
    miss_of = getattr(model, "miss", {})
    occ = np.zeros((c["nz"], c["ny"], c["nx"]), bool)
    voxels = 0
    for key, v in zip(model.keys.tolist(), model.vals.tolist()):
        ix, iy, iz = gm.indices_of(key)
        rx, ry, rz = ix // k - c["x0"], iy // k - c["y0"], iz // k - c["z0"]   # (Python's // is the floor)
        n = int(v[0])
        if not (0 <= rx < c["nx"] and 0 <= ry < c["ny"] and 0 <= rz < c["nz"]) or n < c["min_points"]:
            continue
        if rule is not None and cm.is_dynamic(rule, n, int(miss_of.get(key, 0))):
            continue
        occ[rz, ry, rx] = True
        voxels += 1
    return occ, voxels


def field(occ, R):
    """the definition, by brute force: (d2 uint16, near uint32) of an (nz, ny, nx) bool volume.  The occupied cells are visited in
    ascending (rz, ry, rx) and a later one replaces an earlier one only when it is strictly nearer"""
    nz, ny, nx = occ.shape
    zz, yy, xx = np.meshgrid(np.arange(nz, dtype=np.int64), np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64), indexing="ij")
    best = np.full(occ.shape, np.iinfo(np.int64).max, np.int64)
    near = np.full(occ.shape, NONE, np.int64)
    for sz, sy, sx in np.argwhere(occ).tolist():   # (argwhere: row-major, that is ascending (rz, ry, rx))
        d = (xx - sx) ** 2 + (yy - sy) ** 2 + (zz - sz) ** 2
        better = d < best
        best[better] = d[better]
        near[better] = pack(sx, sy, sz)
    capped = best > R * R
    return np.where(capped, (R + 1) * (R + 1), best).astype(np.uint16), np.where(capped, NONE, near).astype(np.uint32)


def separable(occ, R):
    """the same field by three passes along x, y and z, in plain Python integers: the x pass takes the nearer occupied cell of the row
    and the smaller x on a tie, the y pass and the z pass scan ascending with a strict <, and a partial sum above R * R is dropped"""
    nz, ny, nx = occ.shape
    R2 = R * R
    sx = {}   # (z, y, x) -> x of the row's nearest occupied cell within R
    for z in range(nz):
        for y in range(ny):
            xs = np.flatnonzero(occ[z, y]).tolist()
            for x in range(nx):
                cand = [(abs(s - x), s) for s in xs if abs(s - x) <= R]
                if cand:
                    sx[z, y, x] = min(cand)[1]
    syx = {}   # (z, y, x) -> (partial sum, y, x of the plane's nearest occupied cell)
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                best = None
                for y2 in range(max(0, y - R), min(ny, y + R + 1)):
                    if (z, y2, x) in sx:
                        v = (sx[z, y2, x] - x) ** 2 + (y2 - y) ** 2
                        if v <= R2 and (best is None or v < best[0]):
                            best = (v, y2, sx[z, y2, x])
                if best is not None:
                    syx[z, y, x] = best
    d2 = np.full(occ.shape, (R + 1) * (R + 1), np.uint16)
    near = np.full(occ.shape, NONE, np.uint32)
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                best = None
                for z2 in range(max(0, z - R), min(nz, z + R + 1)):
                    if (z2, y, x) in syx:
                        v = syx[z2, y, x][0] + (z2 - z) ** 2
                        if v <= R2 and (best is None or v < best[0]):
                            best = (v, pack(syx[z2, y, x][2], syx[z2, y, x][1], z2))
                if best is not None:
                    d2[z, y, x], near[z, y, x] = best
    return d2, near


def stats_of(occ, voxels, d2, R):
    within = d2[d2 <= R * R]
    return dict(voxels=int(voxels), occupied=int(occ.sum()), within=int(within.size), max_d2=int(within.max()) if within.size else 0)


def dist(model, rule=None, **cfg):
    """loamx_densemap_dist on a densemap_model.Model: (d2, near, stats); rule = (min_misses, num, den) or None"""
    occ, voxels = occupied(model, rule, **cfg)
    R = dict(DEFAULTS, **cfg)["d_max"]
    d2, near = field(occ, R)
    return d2, near, stats_of(occ, voxels, d2, R)


def cells_of_points(points, leaf, **cfg):
    """(inside, record): per point whether it has a cell in the window, and that cell's record index.  The voxel as the map's add
    computes it: f32 product with inv = 1.0f / leaf, floor, the key rule on every axis (a NaN fails it), no range filter"""
    c = dict(DEFAULTS, **cfg)
    p = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
    inv = np.float32(1.0) / np.float32(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        i = np.floor(p * inv)
        ok = np.all(np.abs(i) < np.float32(1 << dm.QBITS), axis=1)
    inside = np.zeros(len(p), bool)
    record = np.zeros(len(p), np.int64)
    for j in np.flatnonzero(ok).tolist():
        rx, ry, rz = (int(i[j, a]) // c["cell_leaves"] - c[f] for a, f in enumerate(("x0", "y0", "z0")))
        if 0 <= rx < c["nx"] and 0 <= ry < c["ny"] and 0 <= rz < c["nz"]:
            inside[j] = True
            record[j] = (rz * c["ny"] + ry) * c["nx"] + rx
    return inside, record


def query(d2, near, points, leaf, min_d2=0, **cfg):
    """loamx_densemap_dist_query over the planes of dist(): (samples, stats)"""
    inside, record = cells_of_points(points, leaf, **cfg)
    out = np.zeros(len(inside), DIST_SAMPLE)
    out["d2"] = np.where(inside, d2.reshape(-1)[record].astype(np.uint32), np.uint32(OUTSIDE))
    out["near"] = np.where(inside, near.reshape(-1)[record].astype(np.uint32), np.uint32(NONE))
    best = (1 << 64) - 1
    if inside.any():
        lo = int(out["d2"][inside].min())
        best = (lo << 32) | int(np.flatnonzero(inside & (out["d2"] == lo))[0])
    return out, dict(inside=int(inside.sum()), outside=int((~inside).sum()), capped=int((inside & (out["near"] == NONE)).sum()),
                     below=int((inside & (out["d2"] < min_d2)).sum()), best=best)
