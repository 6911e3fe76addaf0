"""Dense map, routing in 3-D over the distance field (loamx_densemap_route3 ...): the blocking loamx_densemap_route3_cells on d2 planes
made here, on a handle with an empty map.  Wall times of the C calls into arrays that stand, a host clock around calls that end in a
stream synchronise, --warmup calls first, then median [min, max] of --reps, with stats[4] (relaxation rounds launched) and stats[5]
(brick runs that did work) of each:
  an open --nx x --ny x --nz window (128 x 64 x 128: 2^20 cells), the goal at its centre, the field back and nothing back;
  beside it, in the same process, the unchanged loamx_densemap_route_cells on an open 1024 x 1024 grid (2^20 cells as well), the goal
  at its centre, nothing back: the yardstick a reader knows, not a ratio to hold (26 neighbours, bricks and other round counts);
  a 3-D serpentine of the same size, the worst case for rounds (floors every third plane with a hole of four cells at alternating
  corners: one shaft through every brick of a storey, storey after storey), nothing back;
  loamx_densemap_route3_trace of --starts starts over it.
--batches 1,2,4,8,16,32,64 repeats the open window and the serpentine, nothing back, for each number of rounds per look (how
DmRoute3::batch was chosen).  There is no reference implementation to race: no time is gated."""
import argparse, ctypes as C, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--nx", type=int, default=128)
ap.add_argument("--ny", type=int, default=64)
ap.add_argument("--nz", type=int, default=128)
ap.add_argument("--grid", type=int, default=1024, help="side of the 2-D yardstick")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--serpentine-reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--starts", type=int, default=64)
ap.add_argument("--capacity", type=int, default=8192)
ap.add_argument("--batches", default="", help="comma-separated rounds per look to sweep")
args = ap.parse_args()

from loam_velodyne_amd import loamx

assert loamx.device_count() >= 1, "this benchmark needs a GPU"
L = loamx.lib()
nx, ny, nz = args.nx, args.ny, args.nz
d = loamx.DenseMap(leaf=0.125, initial_slots=1024)
rc3, rc2 = loamx.Route3Config(), loamx.RouteConfig()
stats = (C.c_uint64 * 6)()

open3 = np.full((nz, ny, nx), 65025, np.uint16)
serp3 = open3.copy()   # tests/densemap_route3_model.py, serpentine3, at this size
for i, z in enumerate(range(3, nz - 3, 3)):
    serp3[z] = 0
    if i % 2 == 0:
        serp3[z, ny - 2:, nx - 2:] = 65025
    else:
        serp3[z, :2, :2] = 65025
field3 = np.zeros((nz, ny, nx), loamx.ROUTE_CELL)
centre3 = np.array([[nx // 2, ny // 2, nz // 2]], np.uint32)
zero3 = np.zeros((1, 3), np.uint32)

G = args.grid
open2 = np.zeros((G, G), loamx.GRID_CELL)
open2["cls"] = loamx.GRID_FREE
open2["clear2"] = 121
centre2 = np.array([[G // 2, G // 2]], np.uint32)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def timed(call, reps):
    for _ in range(args.warmup):
        assert call() == loamx.OK
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert call() == loamx.OK   # (blocks: the call ends in a stream synchronise)
        t.append(time.perf_counter() - t0)
    return np.array(t) * 1e3


def line(name, t, what="brick"):
    print("%-52s median %8.3f ms [min %.3f, max %.3f] of %d (wall); stats[4] %d rounds, stats[5] %d %s runs"
          % (name + ":", np.median(t), t.min(), t.max(), len(t), stats[4], stats[5], what), flush=True)


def route3_open(out=None):
    return L.loamx_densemap_route3_cells(d.h, ptr(open3), nx, ny, nz, C.byref(rc3), ptr(centre3), 1, out, stats)


def route3_serpentine(out=None):
    return L.loamx_densemap_route3_cells(d.h, ptr(serp3), nx, ny, nz, C.byref(rc3), ptr(zero3), 1, out, stats)


def route2_open():
    return L.loamx_densemap_route_cells(d.h, ptr(open2), G, G, C.byref(rc2), ptr(centre2), 1, None, stats)


t0 = time.perf_counter()
assert route3_open(ptr(field3)) == loamx.OK
print("first route3 (allocates the planes): %.1f ms; traversable %d, reachable %d, goals %d, largest cost %d"
      % ((time.perf_counter() - t0) * 1e3, stats[0], stats[1], stats[2], stats[3]), flush=True)
a = np.sort(np.abs(np.stack(np.meshgrid(np.arange(nz) - nz // 2, np.arange(ny) - ny // 2, np.arange(nx) - nx // 2, indexing="ij"))), axis=0)
assert np.array_equal(field3["cost"], 18 * a[0] + 14 * (a[1] - a[0]) + 10 * (a[2] - a[1]))   # the open field's closed form

line("route3_cells, open %d x %d x %d, field back" % (nx, ny, nz), timed(lambda: route3_open(ptr(field3)), args.reps))
line("route3_cells, open %d x %d x %d, nothing back" % (nx, ny, nz), timed(route3_open, args.reps))
line("route_cells (2-D), open %d x %d, nothing back" % (G, G), timed(route2_open, args.reps), what="tile")
line("route3_cells, open, nothing back (again)", timed(route3_open, args.reps))
line("route3_cells, serpentine3, nothing back", timed(route3_serpentine, args.serpentine_reps))
print("serpentine3: traversable %d, reachable %d, largest cost %d" % (stats[0], stats[1], stats[3]), flush=True)

rng = np.random.default_rng(1)
open_cells = np.argwhere(serp3 != 0)
starts = np.ascontiguousarray(open_cells[rng.choice(len(open_cells), args.starts, replace=False)][:, ::-1].astype(np.uint32))
routes = np.zeros((args.starts, args.capacity, 3), np.uint32)
lengths = np.zeros(args.starts, np.uint32)
line("route3_trace of %d starts over it" % args.starts,
     timed(lambda: L.loamx_densemap_route3_trace(d.h, ptr(starts), args.starts, ptr(routes), args.capacity, ptr(lengths)), args.reps))
print("routes: %d cells on average, the longest %d (capacity %d)" % (lengths.mean(), lengths.max(), args.capacity), flush=True)

for batch in [int(b) for b in args.batches.split(",") if b]:
    d.route3_set_batch(batch)
    line("batch %2d: route3_cells, open, nothing back" % batch, timed(route3_open, args.reps))
    line("batch %2d: route3_cells, serpentine3, nothing back" % batch, timed(route3_serpentine, args.serpentine_reps))
d.close()
