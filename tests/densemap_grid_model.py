"""numpy / Python model of the dense map's navigation grid (include/loamx.h, loamx_densemap_grid and what precedes it), exact to the bit:
the definition spelled out over the keys / vals of a tests/densemap_model.py Model (a rule needs a tests/densemap_carve_model.py
CarveModel), Python integers throughout, the elevation in the pattern of densemap_model.export (f64 arithmetic, one f32 rounding) and
clear2 by brute force over every obstacle cell of the window.  The checker of tests/test_densemap_grid_cpu.py and
tests/test_gpu_densemap_grid.py."""
import numpy as np

import densemap_carve_model as cm
import densemap_model as dm

UNKNOWN, FREE, OBSTACLE, STEP = range(4)
NONE = 0x7fffffff   # INT32_MAX: ground / overhead of a cell without one
DEFAULTS = dict(cell_leaves=2, x0=0, z0=0, nx=256, nz=256, min_points=2, y_min=-(1 << 20), y_max=1 << 20, band_lo=3, band_hi=20,
                min_obstacle_voxels=1, max_step=2, clear_max=10)
# loamx_grid_cell, 24 bytes
GRID_CELL = np.dtype([("ground", np.int32), ("elevation", np.float32), ("obstacles", np.uint32), ("overhead", np.int32),
                      ("clear2", np.uint32), ("cls", np.uint32)])
M64 = (1 << 64) - 1


def check(c):
    """the name of the first field of the configuration (a dict with every key of DEFAULTS) that is out of its bounds, or None"""
    if not 1 <= c["cell_leaves"] <= 64:
        return "cell_leaves"
    for f in ("x0", "z0"):
        if abs(c[f]) > 1 << 21:
            return f
    for f in ("nx", "nz"):
        if not 1 <= c[f] <= 8192:
            return f
    if c["nx"] * c["nz"] > 1 << 26:
        return "nx * nz"
    if c["min_points"] < 1:
        return "min_points"
    if c["y_min"] > c["y_max"]:
        return "y_min"
    if c["band_lo"] < 1:
        return "band_lo"
    if c["band_hi"] < c["band_lo"]:
        return "band_hi"
    if c["min_obstacle_voxels"] < 1:
        return "min_obstacle_voxels"
    if not 0 <= c["clear_max"] <= 64:
        return "clear_max"
    return None


def window(leaf, centre, half_extent, k):
    """(first cell, count) of one axis of loamx_densemap_grid_window: in double, from the f32 arguments"""
    e = np.float64(np.float32(leaf)) * np.float64(k)
    c, h = np.float64(np.float32(centre)), np.float64(np.float32(half_extent))
    lo, hi = int(np.floor((c - h) / e)), int(np.floor((c + h) / e))
    return lo, hi - lo + 1


def indices_of(key):
    """(ix, iy, iz) of a voxel key"""
    m = (1 << dm.KBITS) - 1
    return tuple(((int(key) >> (dm.KBITS * a)) & m) - (1 << dm.QBITS) for a in range(3))


def clear2_of(cls, R):
    """brute force: per cell the smallest dx*dx + dz*dz to a cell with cls >= 2, capped"""
    nz, nx = cls.shape
    out = np.full((nz, nx), (R + 1) * (R + 1), np.int64)
    obs = np.argwhere(cls >= OBSTACLE).astype(np.int64)   # (z, x) rows
    if len(obs):
        zz, xx = np.meshgrid(np.arange(nz, dtype=np.int64), np.arange(nx, dtype=np.int64), indexing="ij")
        d = np.full((nz, nx), np.iinfo(np.int64).max, np.int64)
        for oz, ox in obs.tolist():
            d = np.minimum(d, (xx - ox) ** 2 + (zz - oz) ** 2)
        out = np.where(d <= R * R, d, out)
    return out


def grid(model, rule=None, **cfg):
    """loamx_densemap_grid on a densemap_model.Model: the (nz, nx) array of GRID_CELL records; rule = (min_misses, num, den) or None"""
    c = dict(DEFAULTS, **cfg)
    assert set(c) == set(DEFAULTS) and check(c) is None, check(c)
    assert rule is None or (rule[2] != 0 and hasattr(model, "miss"))
    k, x0, z0, nx, nz = c["cell_leaves"], c["x0"], c["z0"], c["nx"], c["nz"]
    miss_of = getattr(model, "miss", {})
    columns = {}   # (rz, rx) -> [(iy, n, Sy)] of the qualifying voxels
    for key, v in zip(model.keys.tolist(), model.vals.tolist()):
        ix, iy, iz = indices_of(key)
        rx, rz = ix // k - x0, iz // k - z0   # (Python's // is the floor)
        n = int(v[0])
        if not (0 <= rx < nx and 0 <= rz < nz) or n < c["min_points"] or not c["y_min"] <= iy <= c["y_max"]:
            continue
        if rule is not None and cm.is_dynamic(rule, n, int(miss_of.get(key, 0))):
            continue
        columns.setdefault((rz, rx), []).append((iy, n, int(v[2])))
    out = np.zeros((nz, nx), GRID_CELL)
    out["ground"] = NONE
    out["overhead"] = NONE
    leaf = np.float64(np.float32(model.leaf))
    for (rz, rx), col in columns.items():
        ground = min(iy for iy, _, _ in col)
        ssn = sum(n for iy, n, _ in col if iy == ground) & M64
        ssy = sum(sy for iy, _, sy in col if iy == ground) & M64
        r = out[rz, rx]
        r["ground"] = ground
        r["elevation"] = np.float32((np.float64(ground) + np.float64(ssy) / (np.float64(ssn) * np.float64(1 << dm.QBITS))) * leaf)
        r["obstacles"] = sum(1 for iy, _, _ in col if c["band_lo"] <= iy - ground <= c["band_hi"])
        above = [iy for iy, _, _ in col if iy - ground > c["band_hi"]]
        r["overhead"] = min(above) if above else NONE
    for (rz, rx) in columns:
        r = out[rz, rx]
        if r["obstacles"] >= c["min_obstacle_voxels"]:
            r["cls"] = OBSTACLE
            continue
        r["cls"] = FREE
        for dz, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            nb = (rz + dz, rx + dx)
            if nb in columns and abs(int(r["ground"]) - int(out[nb]["ground"])) > c["max_step"]:   # (in columns: inside the window, not UNKNOWN)
                r["cls"] = STEP
    out["clear2"] = clear2_of(out["cls"], c["clear_max"])
    return out


def class_counts(cells):
    """(UNKNOWN, FREE, OBSTACLE, STEP) cells"""
    return tuple(int((cells["cls"] == k).sum()) for k in range(4))


def occupancy(cells):
    """loamx_grid_occupancy: -1 UNKNOWN, 0 FREE, 100 OBSTACLE or STEP"""
    return np.array([-1, 0, 100, 100], np.int8)[cells["cls"]]


def pgm_bytes(cells):
    """the pixels of loamx_write_grid_pgm, row-major, width nz and height nx: row r, column u is cells[u, nx - 1 - r]"""
    nz, nx = cells.shape
    px = np.array([205, 254, 0, 0], np.uint8)[cells["cls"]]
    return np.ascontiguousarray(px.T[::-1, :]).tobytes()


# ---- the staircase of the tests: lattice points (one per voxel column and layer, several per voxel) that put level h over the cells of band b
def staircase_points(levels, leaf, k, depth=3, per_voxel=3, first=0):
    """(N, 4) float32: for band b (cells cx = first + b, cz = 0 .. depth - 1) every voxel of the layer iy = levels[b] gets per_voxel
    points at its centre, exact in f32 for a leaf that is a power of two"""
    pts = []
    for b, h in enumerate(levels):
        for ix in range((first + b) * k, (first + b + 1) * k):
            for iz in range(depth * k):
                pts += [((ix + 0.5) * leaf, (h + 0.5) * leaf, (iz + 0.5) * leaf, 0.0)] * per_voxel
    return np.array(pts, np.float32)
