"""Python model of the frontiers of the navigation grid (include/loamx.h, loamx_densemap_frontiers and what goes with it), exact: the
definition spelled out in Python integers over an (nz, nx) array of GRID_CELL records — the frontier predicate with unknown8, the
components by breadth-first search, the records, the labels, stats[0:5] and best.  The costs come from densemap_route_model.field with
the start as the only goal.  The named synthetic grids.  The checker of tests/test_densemap_frontier_cpu.py and
tests/test_gpu_densemap_frontier.py."""
from collections import deque

import numpy as np

import densemap_grid_model as gm
import densemap_route_model as rm

DEFAULTS = dict(connectivity=8, min_unknown=1, min_clear2=1, min_cells=1)
NONE = 0xffffffff
UNREACHABLE = rm.UNREACHABLE
FRONTIER = np.dtype([("min_cell", "<u4"), ("cells", "<u4"), ("lo", "<u4", 2), ("hi", "<u4", 2), ("sum_rx", "<u8"), ("sum_rz", "<u8"),
                     ("unknown_links", "<u8"), ("reachable", "<u4"), ("best_cost", "<u4"), ("best_cell", "<u4"), ("reserved", "<u4")])
assert FRONTIER.itemsize == 64
MAX_CELLS, MAX_ROUTED = 1 << 26, 1 << 22
EIGHT = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))   # (dx, dz)


def check(c):
    """the name of the first field of the configuration (a dict with every key of DEFAULTS) that is out of its bounds, or None"""
    if c["connectivity"] not in (4, 8):
        return "connectivity"
    if not 1 <= c["min_unknown"] <= 8:
        return "min_unknown"
    if c["min_clear2"] < 1:
        return "min_clear2"
    if c["min_cells"] < 1:
        return "min_cells"
    return None


def config(**cfg):
    c = dict(DEFAULTS, **cfg)
    assert set(c) == set(DEFAULTS) and check(c) is None, check(c)
    return c


def unknown8(cells):
    """rows of Python integers: the UNKNOWN cells among the eight neighbours that lie inside the window"""
    cls = cells["cls"].tolist()
    nz, nx = len(cls), len(cls[0])
    return [[sum(1 for dx, dz in EIGHT if 0 <= x + dx < nx and 0 <= z + dz < nz and cls[z + dz][x + dx] == gm.UNKNOWN) for x in range(nx)]
            for z in range(nz)]


def frontier_cells(cells, cfg=None):
    """(rows of booleans: the frontier cells; unknown8)"""
    c = config(**(cfg or {}))
    cls, clear2, u8 = cells["cls"].tolist(), cells["clear2"].tolist(), unknown8(cells)
    nz, nx = len(cls), len(cls[0])
    return [[cls[z][x] == gm.FREE and clear2[z][x] >= c["min_clear2"] and u8[z][x] >= c["min_unknown"] for x in range(nx)] for z in range(nz)], u8


def frontiers(cells, cfg=None, route_cfg=None, start=None):
    """loamx_densemap_frontiers_cells: (the FRONTIER records of the kept frontiers, the (nz, nx) uint32 labels, stats[0:5], the field
    of the route towards start as densemap_route_model gives it, None without a start)"""
    c = config(**(cfg or {}))
    nz, nx = cells.shape
    assert nx * nz <= (MAX_CELLS if start is None else MAX_ROUTED)
    is_fr, u8 = frontier_cells(cells, c)
    field = None if start is None else rm.field(cells, route_cfg, [start])
    cost = None if field is None else field["cost"].tolist()
    moves = [(dx, dz) for dx, dz in EIGHT if abs(dx) + abs(dz) <= (1 if c["connectivity"] == 4 else 2)]
    seen = [[False] * nx for _ in range(nz)]
    found = []   # in ascending min_cell: the scan is in record order and a component is met at its smallest index first
    for z0 in range(nz):
        for x0 in range(nx):
            if not is_fr[z0][x0] or seen[z0][x0]:
                continue
            seen[z0][x0] = True
            comp, queue = [], deque([(x0, z0)])
            while queue:
                x, z = queue.popleft()
                comp.append((x, z))
                for dx, dz in moves:
                    ax, az = x + dx, z + dz
                    if 0 <= ax < nx and 0 <= az < nz and is_fr[az][ax] and not seen[az][ax]:
                        seen[az][ax] = True
                        queue.append((ax, az))
            found.append(comp)
    out = np.zeros(sum(1 for comp in found if len(comp) >= c["min_cells"]), FRONTIER)
    labels = np.full((nz, nx), NONE, np.uint32)
    k = 0
    for comp in found:
        if len(comp) < c["min_cells"]:
            continue
        r = out[k]
        r["min_cell"] = min(z * nx + x for x, z in comp)
        r["cells"] = len(comp)
        r["lo"] = (min(x for x, _ in comp), min(z for _, z in comp))
        r["hi"] = (max(x for x, _ in comp), max(z for _, z in comp))
        r["sum_rx"], r["sum_rz"] = sum(x for x, _ in comp), sum(z for _, z in comp)
        r["unknown_links"] = sum(u8[z][x] for x, z in comp)
        finite = sorted((cost[z][x], z * nx + x) for x, z in comp if cost is not None and cost[z][x] != UNREACHABLE)
        r["reachable"] = len(finite)
        r["best_cost"], r["best_cell"] = finite[0] if finite else (UNREACHABLE, NONE)
        for x, z in comp:
            labels[z, x] = k
        k += 1
    stats = (sum(len(comp) for comp in found), len(found), len(out), int(out["cells"].sum()), int((out["reachable"] > 0).sum()))
    return out, labels, stats, field


def best(records, min_cost=0):
    """loamx_frontiers_best"""
    pick, cost = NONE, UNREACHABLE
    for i, r in enumerate(records):
        if min_cost <= int(r["best_cost"]) < cost:
            pick, cost = i, int(r["best_cost"])
    return pick


# ---- the synthetic grids (cells_of: FREE and UNKNOWN cells carry a large clear2, OBSTACLE and STEP cells 0)
def filled(nx, nz, cls):
    return rm.cells_of(np.full((nz, nx), cls))


def runs(nx, nz):
    """a 1 x n or n x 1 window of alternating runs of three: FREE, UNKNOWN, FREE ..."""
    assert nx == 1 or nz == 1
    return rm.cells_of(np.where((np.arange(nx * nz) // 3) % 2 == 0, gm.FREE, gm.UNKNOWN).reshape(nz, nx))


def square(nx, nz, x0, z0, s):
    """a FREE square of side s with its first cell at (x0, z0), in UNKNOWN"""
    cls = np.full((nz, nx), gm.UNKNOWN)
    cls[z0:z0 + s, x0:x0 + s] = gm.FREE
    return rm.cells_of(cls)


def staircase(n, first, last):
    """FREE cells (i, i), first <= i <= last, in UNKNOWN: they touch by corners only"""
    cls = np.full((n, n), gm.UNKNOWN)
    for i in range(first, last + 1):
        cls[i, i] = gm.FREE
    return rm.cells_of(cls)


def spiral(nx=70, nz=45):
    """a one-cell-wide FREE corridor that winds inwards from (0, 0), its turns one UNKNOWN cell apart"""
    cls = np.full((nz, nx), gm.UNKNOWN)
    x = z = 0
    dx, dz = 1, 0
    cls[0, 0] = gm.FREE

    def free(ax, az):
        return 0 <= ax < nx and 0 <= az < nz and cls[az, ax] == gm.FREE

    while True:
        for _ in range(2):
            ax, az = x + dx, z + dz
            if 0 <= ax < nx and 0 <= az < nz and not free(ax, az) and not free(ax + dx, az + dz):
                x, z = ax, az
                cls[z, x] = gm.FREE
                break
            dx, dz = -dz, dx   # +x, +z, -x, -z
        else:
            return rm.cells_of(cls)


def combs(nx=70, nz=45):
    """two combs in UNKNOWN, teeth up, spine below: 22 teeth three cells apart over rows 5 .. 37 on a spine in row 38 (across two tile
    borders in x and one in z), and 4 teeth over rows 41 .. 43 on a spine in row 44 (inside one tile)"""
    cls = np.full((nz, nx), gm.UNKNOWN)
    cls[5:38, 3:67:3] = gm.FREE
    cls[38, 3:67] = gm.FREE
    cls[41:44, 2:12:3] = gm.FREE
    cls[44, 2:12] = gm.FREE
    return rm.cells_of(cls)


def no_unknown(nx=40, nz=36):
    """FREE beside OBSTACLE and STEP cells only"""
    cls = np.full((nz, nx), gm.FREE)
    cls[::5, ::7] = gm.OBSTACLE
    cls[3::6, 2::5] = gm.STEP
    return rm.cells_of(cls)


def narrow(min_clear2=3):
    """three FREE cells in a row in UNKNOWN; the middle one has clear2 = min_clear2 - 1"""
    cls = np.full((3, 5), gm.UNKNOWN)
    cls[1, 1:4] = gm.FREE
    a = rm.cells_of(cls)
    a["clear2"][1, 2] = min_clear2 - 1
    return a


def random70(seed=23):
    rng = np.random.default_rng(seed)
    cls = rng.choice(4, size=(70, 70), p=[0.25, 0.6, 0.1, 0.05])
    clear2 = rng.integers(1, 30, size=(70, 70))
    clear2[cls >= gm.OBSTACLE] = 0
    return rm.cells_of(cls, clear2)


def walled(nx=40, nz=12):
    """two FREE rooms in an UNKNOWN rim, an OBSTACLE wall two cells thick between them"""
    cls = np.full((nz, nx), gm.UNKNOWN)
    cls[1:nz - 1, 1:nx - 1] = gm.FREE
    cls[:, nx // 2 - 1:nx // 2 + 1] = gm.OBSTACLE
    return rm.cells_of(cls)
