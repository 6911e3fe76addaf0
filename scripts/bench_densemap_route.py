"""Dense map, routing on the navigation grid (loamx_densemap_route ...): the terrain and the 1024 x 1024 window of
scripts/bench_densemap_grid.py (a rolling ground of one voxel per column, two points each, --pillars random pillars of ten voxels on
it), a goal at the free cell nearest the window's centre.  Wall times of the blocking C calls into arrays that stand, median
[min, max] of --reps, with stats[4] (relaxation rounds launched) and stats[5] (tile runs that did work) of each:
  loamx_densemap_grid alone;
  loamx_densemap_route with the field back;
  loamx_densemap_route with nothing back, followed by loamx_densemap_route_trace of 64 starts;
  loamx_densemap_route_cells on a --window x --window serpentine, the worst case for rounds (one corridor through every tile, again
  and again).
--batches 1,2,4,8,16,32,64 repeats the two routes with nothing back for each number of rounds per look (how DmRoute::batch was chosen).
There is no reference implementation to race: no time is gated."""
import argparse, ctypes as C, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=1000)
ap.add_argument("--leaf", type=float, default=0.125)
ap.add_argument("--pillars", type=int, default=2000)
ap.add_argument("--window", type=int, default=1024)
ap.add_argument("--clear-max", type=int, default=10)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--serpentine-reps", type=int, default=10)
ap.add_argument("--starts", type=int, default=64)
ap.add_argument("--capacity", type=int, default=4096)
ap.add_argument("--batches", default="", help="comma-separated rounds per look to sweep")
args = ap.parse_args()

from loam_velodyne_amd import loamx

rng = np.random.default_rng(1)
n = args.side
ix, iz = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
height = np.floor(3.0 * np.sin(ix / 40.0) + 2.0 * np.cos(iz / 55.0)).astype(np.int64)   # a rolling ground, steps of one leaf
px, pz = rng.integers(0, n, args.pillars), rng.integers(0, n, args.pillars)
cols = [np.stack([ix.ravel(), height.ravel(), iz.ravel()], axis=1)]
for k in range(1, 11):
    cols.append(np.stack([px, height[px, pz] + k, pz], axis=1))
vox = np.concatenate(cols)
pts = np.zeros((2 * len(vox), 4), np.float32)
pts[:, :3] = (np.repeat(vox, 2, axis=0) + rng.uniform(0.1, 0.9, (2 * len(vox), 3))) * args.leaf

d = loamx.DenseMap(leaf=args.leaf, initial_slots=1 << 22)
for k in range(0, len(pts), 1 << 21):
    d.add(pts[k:k + (1 << 21)], (0.0, 0.0, 0.0))
st = d.stats()
print("map: %d points, %d voxels, %d slots" % (len(pts), st["voxels"], st["slots"]), flush=True)

L = loamx.lib()
W = args.window
lo = (n - W) // 2
cfg = loamx.GridConfig(cell_leaves=1, x0=lo, z0=lo, nx=W, nz=W, clear_max=args.clear_max)
rc = loamx.RouteConfig()
cells = d.grid(cfg)
free = np.argwhere(cells["cls"] == loamx.GRID_FREE)
goal = free[np.argmin(((free - W // 2) ** 2).sum(axis=1))]
goals = np.array([[goal[1], goal[0]]], np.uint32)
field = np.zeros((W, W), loamx.ROUTE_CELL)
stats = (C.c_uint64 * 6)()
gp, fp, cp = goals.ctypes.data_as(C.c_void_p), field.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p)


def timed(call, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert call() == loamx.OK
        t.append(time.perf_counter() - t0)
    return np.array(t) * 1e3


def line(name, t, with_stats=True):
    tail = "; stats[4] %d rounds, stats[5] %d tile runs" % (stats[4], stats[5]) if with_stats else ""
    print("%-46s median %8.2f ms [min %.2f, max %.2f] of %d (wall)%s" % (name + ":", np.median(t), t.min(), t.max(), len(t), tail), flush=True)


def route_field():
    return L.loamx_densemap_route(d.h, C.byref(cfg), None, C.byref(rc), gp, 1, None, fp, stats)


def route_nothing():
    return L.loamx_densemap_route(d.h, C.byref(cfg), None, C.byref(rc), gp, 1, None, None, stats)


t0 = time.perf_counter()
assert route_field() == loamx.OK
print("first route (allocates the planes): %.1f ms; traversable %d, reachable %d, goals %d, largest cost %d"
      % ((time.perf_counter() - t0) * 1e3, stats[0], stats[1], stats[2], stats[3]), flush=True)
reach = np.argwhere(field["cost"] != loamx.ROUTE_UNREACHABLE)
starts = np.ascontiguousarray(reach[rng.choice(len(reach), args.starts, replace=False)][:, ::-1].astype(np.uint32))
routes = np.zeros((args.starts, args.capacity, 2), np.uint32)
lengths = np.zeros(args.starts, np.uint32)


def route_and_trace():
    r = route_nothing()
    return r if r != loamx.OK else L.loamx_densemap_route_trace(d.h, starts.ctypes.data_as(C.c_void_p), args.starts,
                                                                routes.ctypes.data_as(C.c_void_p), args.capacity,
                                                                lengths.ctypes.data_as(C.c_void_p))


line("loamx_densemap_grid", timed(lambda: L.loamx_densemap_grid(d.h, C.byref(cfg), None, cp), args.reps), with_stats=False)
line("loamx_densemap_route, field back", timed(route_field, args.reps))
line("loamx_densemap_route, nothing back", timed(route_nothing, args.reps))
line("the same + route_trace of %d starts" % args.starts, timed(route_and_trace, args.reps))
print("routes: %d cells on average, the longest %d (capacity %d)" % (lengths.mean(), lengths.max(), args.capacity), flush=True)
host, m = loamx.route_trace(field, tuple(starts[0]), args.capacity)
assert m == lengths[0] and host.tobytes() == routes[0, :min(m, args.capacity)].tobytes()

# the serpentine: walls on the rows 4, 8, ..., gaps of two cells at alternating ends
cls = np.full((W, W), loamx.GRID_FREE, np.uint32)
for i, z in enumerate(range(4, W - 1, 4)):
    if i % 2 == 0:
        cls[z, :W - 2] = loamx.GRID_OBSTACLE
    else:
        cls[z, 2:] = loamx.GRID_OBSTACLE
serp = np.zeros((W, W), loamx.GRID_CELL)
serp["cls"] = cls
serp["clear2"] = np.where(cls == loamx.GRID_FREE, 121, 0)
zero = np.zeros((1, 2), np.uint32)
sp, zp = serp.ctypes.data_as(C.c_void_p), zero.ctypes.data_as(C.c_void_p)


def route_serpentine(out=fp):
    return L.loamx_densemap_route_cells(d.h, sp, W, W, C.byref(rc), zp, 1, out, stats)


line("loamx_densemap_route_cells, serpentine", timed(route_serpentine, args.serpentine_reps))
print("serpentine: reachable %d, largest cost %d" % (stats[1], stats[3]), flush=True)
for batch in [int(b) for b in args.batches.split(",") if b]:
    d.route_set_batch(batch)
    line("batch %2d: route, nothing back" % batch, timed(route_nothing, args.reps))
    line("batch %2d: route_cells, serpentine, nothing back" % batch, timed(lambda: route_serpentine(None), args.serpentine_reps))
d.close()
