"""Python model of routing in 3-D over the distance field (include/loamx.h, loamx_densemap_route3 and what goes with it), exact: the
definition spelled out in Python integers over an (nz, ny, nx) array of d2 values — the weight of a cell, the legal moves with the
corner rule and their costs, the cost-to-go field by heapq Dijkstra with next derived from the final costs, the trace, the metres of a
route and the cell of a position — and min_crossings, the figure the schedule bound of the GPU test is stated in.  Two named synthetic
fields.  The checker of tests/test_densemap_route3_cpu.py and tests/test_gpu_densemap_route3.py."""
import heapq

import numpy as np

DEFAULTS = dict(connectivity=26, min_d2=1, soft_d2=0, soft_weight=0)
UNREACHABLE, GOAL, NONE = 0xffffffff, 26, 27
# (dx, dy, dz) of direction d, written out as include/loamx.h has them
MOVES = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
         (1, 1, 0), (-1, 1, 0), (1, -1, 0), (-1, -1, 0), (1, 0, 1), (-1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 1), (0, -1, 1), (0, 1, -1),
         (0, -1, -1)) + tuple((-1 if i & 1 else 1, -1 if i & 2 else 1, -1 if i & 4 else 1) for i in range(8))
SCALE = tuple(3 + 2 * sum(1 for v in m if v) for m in MOVES)   # 5, 7, 9 for one, two, three non-zero components
# the cells between a and b that the corner rule asks for: a + (sx, sy, sz), s in {0, d} per axis, but for a and b themselves
BETWEEN = tuple(tuple(sorted({(sx, sy, sz) for sx in (0, m[0]) for sy in (0, m[1]) for sz in (0, m[2])} - {(0, 0, 0), m})) for m in MOVES)
ROUTE_CELL = np.dtype([("cost", np.uint32), ("next", np.uint32)])   # loamx_route_cell, 8 bytes
MAX_CELLS = 1 << 22
FAR = 65025   # the d2 of the open cells of the synthetic fields: the largest cap, (254 + 1)^2


def check(c):
    """the name of the first field of the configuration (a dict with every key of DEFAULTS) that is out of its bounds, or None"""
    if c["connectivity"] not in (6, 18, 26):
        return "connectivity"
    if c["min_d2"] < 1:
        return "min_d2"
    if not 0 <= c["soft_d2"] <= 65025:
        return "soft_d2"
    if not 0 <= c["soft_weight"] <= 15:
        return "soft_weight"
    return None


def config(**cfg):
    c = dict(DEFAULTS, **cfg)
    assert set(c) == set(DEFAULTS) and check(c) is None, check(c)
    return c


def weight_of(d2, c):
    """w of one cell: 0 blocked, otherwise 1..16"""
    d2 = int(d2)
    if d2 < c["min_d2"]:
        return 0
    return 1 + (c["soft_weight"] * (c["soft_d2"] - d2) // c["soft_d2"] if d2 < c["soft_d2"] else 0)


def weight(d2, cfg=None):
    """the weights of an (nz, ny, nx) d2 array as nested lists [z][y][x] of Python integers"""
    c = config(**(cfg or {}))
    return [[[weight_of(v, c) for v in row] for row in plane] for plane in np.asarray(d2).tolist()]


def moves(w, x, y, z, connectivity):
    """the legal moves from (x, y, z) over the weights w: (d, bx, by, bz, cost), smallest d first"""
    nz, ny, nx = len(w), len(w[0]), len(w[0][0])
    wa = w[z][y][x]
    if not wa:
        return
    for d in range(connectivity):
        dx, dy, dz = MOVES[d]
        bx, by, bz = x + dx, y + dy, z + dz
        if not (0 <= bx < nx and 0 <= by < ny and 0 <= bz < nz) or not w[bz][by][bx]:
            continue
        if not all(w[z + sz][y + sy][x + sx] for sx, sy, sz in BETWEEN[d]):   # no corner cutting (inside the window: between a and b)
            continue
        yield d, bx, by, bz, SCALE[d] * (wa + w[bz][by][bx])


def used_goals(w, goals):
    nz, ny, nx = len(w), len(w[0]), len(w[0][0])
    return [(int(x), int(y), int(z)) for x, y, z in goals
            if 0 <= int(x) < nx and 0 <= int(y) < ny and 0 <= int(z) < nz and w[int(z)][int(y)][int(x)]]


def field(d2, cfg=None, goals=()):
    """loamx_densemap_route3_cells: the (nz, ny, nx) array of ROUTE_CELL records"""
    c = config(**(cfg or {}))
    w = weight(d2, c)
    nz, ny, nx = len(w), len(w[0]), len(w[0][0])
    assert nx * ny * nz <= MAX_CELLS
    cost = [[[UNREACHABLE] * nx for _ in range(ny)] for _ in range(nz)]
    heap = []
    for x, y, z in used_goals(w, goals):
        cost[z][y][x] = 0
        heap.append((0, x, y, z))
    heapq.heapify(heap)
    while heap:
        k, x, y, z = heapq.heappop(heap)
        if k != cost[z][y][x]:
            continue
        for _, bx, by, bz, m in moves(w, x, y, z, c["connectivity"]):   # (the cost and the legality of a move are symmetric)
            if k + m < cost[bz][by][bx]:
                cost[bz][by][bx] = k + m
                heapq.heappush(heap, (k + m, bx, by, bz))
    out = np.zeros((nz, ny, nx), ROUTE_CELL)
    out["cost"] = cost
    nxt = np.where(out["cost"] == 0, GOAL, NONE).astype(np.uint32)
    for z, y, x in np.argwhere((out["cost"] > 0) & (out["cost"] != UNREACHABLE)).tolist():
        k = cost[z][y][x]
        nxt[z, y, x] = next(d for d, bx, by, bz, m in moves(w, x, y, z, c["connectivity"])
                            if cost[bz][by][bx] != UNREACHABLE and cost[bz][by][bx] + m == k)
    out["next"] = nxt
    return out


def stats(d2, cfg, goals, f):
    """stats[0:4] of the call that gave the field f: traversable, reachable, goals used, the largest finite cost"""
    w = weight(d2, cfg)
    finite = f["cost"][f["cost"] != UNREACHABLE]
    return (sum(1 for plane in w for row in plane for v in row if v), int(len(finite)), len(used_goals(w, goals)),
            int(finite.max()) if len(finite) else 0)


def min_crossings(d2, cfg=None, goals=(), brick=8):
    """the largest, over the reachable cells, of the fewest brick-border crossings on any cheapest path to a goal: Dijkstra on the pair
    (cost, crossings), compared lexicographically.  A move crosses when its two cells lie in different bricks."""
    c = config(**(cfg or {}))
    w = weight(d2, c)
    best = {}
    heap = []
    for g in used_goals(w, goals):
        best[g] = (0, 0)
        heap.append((0, 0, *g))
    heapq.heapify(heap)
    while heap:
        k, n, x, y, z = heapq.heappop(heap)
        if (k, n) != best[(x, y, z)]:
            continue
        for _, bx, by, bz, m in moves(w, x, y, z, c["connectivity"]):
            lab = (k + m, n + ((bx // brick, by // brick, bz // brick) != (x // brick, y // brick, z // brick)))
            if lab < best.get((bx, by, bz), (UNREACHABLE, 0)):
                best[(bx, by, bz)] = lab
                heapq.heappush(heap, (*lab, bx, by, bz))
    return max((n for _, n in best.values()), default=0)


def trace(f, start, capacity=None):
    """loamx_route3_trace on a field of ours: ((min(n, capacity), 3) uint32 triples (rx, ry, rz), n)"""
    nz, ny, nx = f.shape
    x, y, z = int(start[0]), int(start[1]), int(start[2])
    route = []
    if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and f[z, y, x]["next"] != NONE:
        nxt, cost = f["next"].tolist(), f["cost"].tolist()   # (Python integers from here on)
        while True:
            route.append((x, y, z))
            d = nxt[z][y][x]
            if d == GOAL:
                break
            bx, by, bz = x + MOVES[d][0], y + MOVES[d][1], z + MOVES[d][2]
            assert 0 <= bx < nx and 0 <= by < ny and 0 <= bz < nz and cost[bz][by][bx] < cost[z][y][x]
            x, y, z = bx, by, bz
    n = len(route)
    return np.array(route[:n if capacity is None else capacity], np.uint32).reshape(-1, 3), n


def points(dist_cfg, leaf, route):
    """loamx_route3_points: (n, 3) float32; dist_cfg a dict with x0, y0, z0, cell_leaves"""
    leaf = float(np.float32(leaf))
    out = np.zeros((len(route), 3), np.float32)
    for i, r in enumerate(route):
        for a, first in enumerate(("x0", "y0", "z0")):
            out[i, a] = np.float32((float(dist_cfg[first]) + float(int(r[a])) + 0.5) * leaf * float(dist_cfg["cell_leaves"]))
    return out


def cell_of(dist_cfg, leaf, x, y, z):
    """loamx_densemap_dist_cell_of: (rx, ry, rz), or None outside the window"""
    e = float(np.float32(leaf)) * float(dist_cfg["cell_leaves"])
    r = tuple(int(np.floor(float(np.float32(p)) / e)) - dist_cfg[first] for p, first in ((x, "x0"), (y, "y0"), (z, "z0")))
    return r if all(0 <= v < dist_cfg[n] for v, n in zip(r, ("nx", "ny", "nz"))) else None


# ---- the synthetic fields: open cells carry a large d2, walls are occupied cells, d2 0
def open(nx, ny, nz):   # noqa: A001 (the field's name)
    return np.full((nz, ny, nx), FAR, np.uint16)


def serpentine3(nx=20, ny=9, nz=19):
    """floors on the planes z = 3, 6, ... (3, 6, 9, 12, 15 at nz = 19); the 1st, 3rd, ... leave the four cells with y >= ny - 2 and
    x >= nx - 2 open, the 2nd, 4th, ... the four cells with y < 2 and x < 2: one shaft that winds from the first storey to the last"""
    d2 = open(nx, ny, nz)
    for i, z in enumerate(range(3, nz - 3, 3)):
        d2[z] = 0
        if i % 2 == 0:
            d2[z, ny - 2:, nx - 2:] = FAR
        else:
            d2[z, :2, :2] = FAR
    return d2
