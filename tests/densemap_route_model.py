"""Python model of routing on the navigation grid (include/loamx.h, loamx_densemap_route and what goes with it), exact: the definition
spelled out in Python integers over an (nz, nx) array of GRID_CELL records — the weight of a cell, the legal moves and their costs, the
cost-to-go field by heapq Dijkstra with next derived from the final costs, the trace, the metres of a route and the cell of a position
— and min_crossings, the figure the schedule bound of the GPU test is stated in.  Two named synthetic grids.  The checker of
tests/test_densemap_route_cpu.py and tests/test_gpu_densemap_route.py."""
import heapq

import numpy as np

import densemap_grid_model as gm

DEFAULTS = dict(connectivity=8, min_clear2=1, soft_clear2=0, soft_weight=0, unknown_weight=0)
UNREACHABLE, GOAL, NONE = 0xffffffff, 8, 9
MOVES = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))   # (dx, dz) of direction d
ROUTE_CELL = np.dtype([("cost", np.uint32), ("next", np.uint32)])   # loamx_route_cell, 8 bytes
MAX_CELLS = 1 << 22
FAR = 4225   # the clear2 of the FREE cells of the synthetic grids: the largest cap, (64 + 1)^2


def check(c):
    """the name of the first field of the configuration (a dict with every key of DEFAULTS) that is out of its bounds, or None"""
    if c["connectivity"] not in (4, 8):
        return "connectivity"
    if c["min_clear2"] < 1:
        return "min_clear2"
    if not 0 <= c["soft_clear2"] <= 4225:
        return "soft_clear2"
    if not 0 <= c["soft_weight"] <= 15:
        return "soft_weight"
    if not 0 <= c["unknown_weight"] <= 16:
        return "unknown_weight"
    return None


def config(**cfg):
    c = dict(DEFAULTS, **cfg)
    assert set(c) == set(DEFAULTS) and check(c) is None, check(c)
    return c


def weight_of(cls, clear2, c):
    """w of one cell: 0 blocked, otherwise 1..32"""
    cls, clear2 = int(cls), int(clear2)
    if clear2 < c["min_clear2"]:
        return 0
    if not (cls == gm.FREE or (cls == gm.UNKNOWN and c["unknown_weight"] > 0)):
        return 0
    p = c["soft_weight"] * (c["soft_clear2"] - clear2) // c["soft_clear2"] if clear2 < c["soft_clear2"] else 0
    return 1 + p + (c["unknown_weight"] if cls == gm.UNKNOWN else 0)


def weight(cells, cfg=None):
    """the weights of an (nz, nx) GRID_CELL array as a list of rows of Python integers"""
    c = config(**(cfg or {}))
    return [[weight_of(r["cls"], r["clear2"], c) for r in row] for row in cells]


def moves(w, x, z, connectivity):
    """the legal moves from (x, z) over the weights w: (d, bx, bz, cost), smallest d first"""
    nz, nx = len(w), len(w[0])
    wa = w[z][x]
    if not wa:
        return
    for d in range(0, 8, 1 if connectivity == 8 else 2):
        dx, dz = MOVES[d]
        bx, bz = x + dx, z + dz
        if not (0 <= bx < nx and 0 <= bz < nz) or not w[bz][bx]:
            continue
        if d & 1 and not (w[z][bx] and w[bz][x]):   # no corner cutting
            continue
        yield d, bx, bz, (7 if d & 1 else 5) * (wa + w[bz][bx])


def used_goals(w, goals):
    nz, nx = len(w), len(w[0])
    return [(int(x), int(z)) for x, z in goals if 0 <= int(x) < nx and 0 <= int(z) < nz and w[int(z)][int(x)]]


def field(cells, cfg=None, goals=()):
    """loamx_densemap_route_cells: the (nz, nx) array of ROUTE_CELL records"""
    c = config(**(cfg or {}))
    w = weight(cells, c)
    nz, nx = len(w), len(w[0])
    assert nx * nz <= MAX_CELLS
    cost = [[UNREACHABLE] * nx for _ in range(nz)]
    heap = []
    for x, z in used_goals(w, goals):
        cost[z][x] = 0
        heap.append((0, x, z))
    heapq.heapify(heap)
    while heap:
        k, x, z = heapq.heappop(heap)
        if k != cost[z][x]:
            continue
        for _, bx, bz, m in moves(w, x, z, c["connectivity"]):   # (the cost of a move is symmetric)
            if k + m < cost[bz][bx]:
                cost[bz][bx] = k + m
                heapq.heappush(heap, (k + m, bx, bz))
    out = np.zeros((nz, nx), ROUTE_CELL)
    for z in range(nz):
        for x in range(nx):
            k = cost[z][x]
            nxt = GOAL if k == 0 else NONE
            if 0 < k < UNREACHABLE:
                nxt = next(d for d, bx, bz, m in moves(w, x, z, c["connectivity"]) if cost[bz][bx] != UNREACHABLE and cost[bz][bx] + m == k)
            out[z, x] = (k, nxt)
    return out


def stats(cells, cfg, goals, f):
    """stats[0:4] of the call that gave the field f: traversable, reachable, goals used, the largest finite cost"""
    w = weight(cells, cfg)
    finite = f["cost"][f["cost"] != UNREACHABLE]
    return (sum(1 for row in w for v in row if v), int(len(finite)), len(used_goals(w, goals)), int(finite.max()) if len(finite) else 0)


def min_crossings(cells, cfg=None, goals=(), tile=32):
    """the largest, over the reachable cells, of the fewest tile-border crossings on any cheapest path to a goal: Dijkstra on the pair
    (cost, crossings), compared lexicographically.  A move crosses when its two cells lie in different tiles."""
    c = config(**(cfg or {}))
    w = weight(cells, c)
    best = {}
    heap = []
    for x, z in used_goals(w, goals):
        best[(x, z)] = (0, 0)
        heap.append((0, 0, x, z))
    heapq.heapify(heap)
    while heap:
        k, n, x, z = heapq.heappop(heap)
        if (k, n) != best[(x, z)]:
            continue
        for _, bx, bz, m in moves(w, x, z, c["connectivity"]):
            lab = (k + m, n + ((bx // tile, bz // tile) != (x // tile, z // tile)))
            if lab < best.get((bx, bz), (UNREACHABLE, 0)):
                best[(bx, bz)] = lab
                heapq.heappush(heap, (*lab, bx, bz))
    return max((n for _, n in best.values()), default=0)


def trace(f, start, capacity=None):
    """loamx_grid_route_trace on a field of ours: ((min(n, capacity), 2) uint32 pairs (rx, rz), n)"""
    nz, nx = f.shape
    x, z = int(start[0]), int(start[1])
    route = []
    if 0 <= x < nx and 0 <= z < nz and f[z, x]["next"] != NONE:
        nxt, cost = f["next"].tolist(), f["cost"].tolist()   # (Python integers from here on)
        while True:
            route.append((x, z))
            d = nxt[z][x]
            if d == GOAL:
                break
            bx, bz = x + MOVES[d][0], z + MOVES[d][1]
            assert 0 <= bx < nx and 0 <= bz < nz and cost[bz][bx] < cost[z][x]
            x, z = bx, bz
    n = len(route)
    return np.array(route[:n if capacity is None else capacity], np.uint32).reshape(-1, 2), n


def points(grid_cfg, leaf, route, cells=None):
    """loamx_grid_route_points: (n, 3) float32; grid_cfg a dict with x0, z0, cell_leaves"""
    leaf = float(np.float32(leaf))
    out = np.zeros((len(route), 3), np.float32)
    for i, (rx, rz) in enumerate(route):
        rx, rz = int(rx), int(rz)
        out[i, 0] = np.float32((float(grid_cfg["x0"]) + float(rx) + 0.5) * leaf * float(grid_cfg["cell_leaves"]))
        out[i, 2] = np.float32((float(grid_cfg["z0"]) + float(rz) + 0.5) * leaf * float(grid_cfg["cell_leaves"]))
        if cells is not None and cells[rz, rx]["cls"] != gm.UNKNOWN:
            out[i, 1] = cells[rz, rx]["elevation"]
    return out


def cell_of(grid_cfg, leaf, x, z):
    """loamx_densemap_grid_cell_of: (rx, rz), or None outside the window"""
    e = float(np.float32(leaf)) * float(grid_cfg["cell_leaves"])
    rx = int(np.floor(float(np.float32(x)) / e)) - grid_cfg["x0"]
    rz = int(np.floor(float(np.float32(z)) / e)) - grid_cfg["z0"]
    return (rx, rz) if 0 <= rx < grid_cfg["nx"] and 0 <= rz < grid_cfg["nz"] else None


# ---- the synthetic grids: FREE cells carry a large clear2, walls are OBSTACLE with clear2 0
def cells_of(cls, clear2=None):
    a = np.zeros(np.shape(cls), gm.GRID_CELL)
    a["cls"] = cls
    a["ground"] = np.where(a["cls"] == gm.UNKNOWN, gm.NONE, 0)
    a["overhead"] = gm.NONE
    a["clear2"] = np.where(a["cls"] >= gm.OBSTACLE, 0, FAR) if clear2 is None else clear2
    return a


def open(nx, nz):   # noqa: A001 (the grid's name)
    return cells_of(np.full((nz, nx), gm.FREE))


def serpentine(nx=70, nz=45):
    """walls on the rows z = 4, 8, ..., the 1st, 3rd, ... over x in [0, nx - 2), the 2nd, 4th, ... over x in [2, nx): one corridor
    that winds from the first row to the last"""
    cls = np.full((nz, nx), gm.FREE)
    for i, z in enumerate(range(4, nz - 1, 4)):
        if i % 2 == 0:
            cls[z, :nx - 2] = gm.OBSTACLE
        else:
            cls[z, 2:] = gm.OBSTACLE
    return cells_of(cls)
