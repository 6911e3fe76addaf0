"""Dense map, distance field (loamx_densemap_dist, loamx_densemap_dist_query): the synthetic terrain of bench_densemap_grid.py (--side x
--side voxels at --leaf, a rolling ground of one voxel per column, two points each, and --pillars random pillars of ten voxels on it:
about a million voxels at the default side of 1000) is added from the host; then four things are timed in the same run for a window
of --nx x --ny x --nz cells of --cell-leaves voxels about the terrain's middle with d_max = --d-max (median, min, max of --reps, the
first call of the window's size apart): the field with nothing back, the field with d2 back, a query of --points points spread over
the window and a margin around it, and download(), which is only the first step of doing the same on the host.

Each device step is given a time limit of its own by the caller:
    timeout -k 10 300 python scripts/bench_densemap_dist.py
Device times come from a run of their own,
    timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/bench_densemap_dist.py --no-download
and `--summarise DIR` (no device needed) then prints the median time of each kernel over the calls of that run."""
import argparse, csv, glob, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=1000)
ap.add_argument("--leaf", type=float, default=0.125)
ap.add_argument("--pillars", type=int, default=2000)
ap.add_argument("--nx", type=int, default=256)
ap.add_argument("--ny", type=int, default=64)
ap.add_argument("--nz", type=int, default=256)
ap.add_argument("--cell-leaves", type=int, default=2)
ap.add_argument("--d-max", type=int, default=32)
ap.add_argument("--points", type=int, default=131072)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--download-reps", type=int, default=5)
ap.add_argument("--no-download", action="store_true")
ap.add_argument("--summarise", default=None, metavar="DIR", help="print the kernel times of the kernel_trace.csv files under DIR and exit")
args = ap.parse_args()

KERNELS = ("k_dm_dist_mark", "k_dm_dist_xy", "k_dm_dist_z", "k_dm_dist_query")


def summarise(root):
    paths = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True))
    assert paths, "no kernel_trace.csv under " + root
    for path in paths:
        rows = list(csv.DictReader(open(path)))
        name_col = next(k for k in rows[0] if k.lower() in ("kernel_name", "name"))
        start_col = next(k for k in rows[0] if k.lower().startswith("start"))
        end_col = next(k for k in rows[0] if k.lower().startswith("end"))
        print("device times from %s" % path)
        total = 0.0
        for name in KERNELS:
            t = np.array([(int(x[end_col]) - int(x[start_col])) / 1e3 for x in rows if name in x[name_col]])
            assert len(t) > 1, name
            t = t[1:]   # (without the first launch)
            if name != "k_dm_dist_query":
                total += np.median(t)
            print("%-20s median %8.1f us [min %.1f, max %.1f] over %d launches" % (name + ":", np.median(t), t.min(), t.max(), len(t)))
        print("%-20s %8.1f us (sum of the medians of the field's three kernels)" % ("the field:", total))


if args.summarise:
    summarise(args.summarise)
    sys.exit(0)

import ctypes as C
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
t0 = time.perf_counter()
for k in range(0, len(pts), 1 << 21):
    d.add(pts[k:k + (1 << 21)], (0.0, 0.0, 0.0))
st = d.stats()
print("map: %d points, %d voxels, %d slots in %.1f s" % (len(pts), st["voxels"], st["slots"], time.perf_counter() - t0), flush=True)

k = args.cell_leaves
mid = n // (2 * k)
cfg = loamx.DistConfig(cell_leaves=k, x0=mid - args.nx // 2, y0=-(args.ny // 4), z0=mid - args.nz // 2, nx=args.nx, ny=args.ny, nz=args.nz,
                       d_max=args.d_max)
t0 = time.perf_counter()
d.dist(cfg, want_d2=False)
print("first call (allocates the buffers): %.1f ms; %s" % ((time.perf_counter() - t0) * 1e3, d.dist_stats), flush=True)

# the C calls alone, into arrays that stand (DenseMap.dist also allocates its result)
L = loamx.lib()
d2 = np.zeros((cfg.nz, cfg.ny, cfg.nx), np.uint16)
st4, st5 = (C.c_uint64 * 4)(), (C.c_uint64 * 5)()
e = args.leaf * k
lo = np.array([cfg.x0, cfg.y0, cfg.z0]) * e
hi = lo + np.array([cfg.nx, cfg.ny, cfg.nz]) * e
q = np.zeros((args.points, 4), np.float32)
q[:, :3] = rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), (args.points, 3))
cloud = loamx.cloud_of(q)
samples = np.zeros(args.points, loamx.DIST_SAMPLE)
t_none, t_d2, t_query = [], [], []
for _ in range(args.reps):
    t0 = time.perf_counter()
    rc = L.loamx_densemap_dist(d.h, C.byref(cfg), None, None, None, st4)
    t_none.append(time.perf_counter() - t0)
    assert rc == loamx.OK
    t0 = time.perf_counter()
    rc = L.loamx_densemap_dist(d.h, C.byref(cfg), None, d2.ctypes.data_as(C.c_void_p), None, st4)
    t_d2.append(time.perf_counter() - t0)
    assert rc == loamx.OK
    t0 = time.perf_counter()
    rc = L.loamx_densemap_dist_query(d.h, C.byref(cloud), C.c_uint32(4), samples.ctypes.data_as(C.c_void_p), C.c_uint64(args.points), st5)
    t_query.append(time.perf_counter() - t0)
    assert rc == loamx.OK
inside = samples["d2"] != loamx.DIST_OUTSIDE
assert int(inside.sum()) == st5[0] and st5[0] + st5[1] == args.points and int(samples["d2"][inside].min()) == st5[4] >> 32
shape = "%d x %d x %d cells of %d voxels, d_max %d" % (cfg.nx, cfg.ny, cfg.nz, k, cfg.d_max)
for name, t in (("field, nothing back", t_none), ("field, d2 back", t_d2), ("query, %d points" % args.points, t_query)):
    t = np.array(t) * 1e3
    print("%-26s %s: median %.3f ms [min %.3f, max %.3f] per call (wall)" % (name + ":", shape, np.median(t), t.min(), t.max()), flush=True)
print("stats %s; query %s; %d bytes of d2" % (list(st4), list(st5), d2.nbytes), flush=True)
med_none = float(np.median(t_none)) * 1e3
if not args.no_download:
    times = []
    for _ in range(args.download_reps):
        t0 = time.perf_counter()
        p = d.points()
        times.append(time.perf_counter() - t0)
    t = np.array(times) * 1e3
    print("DenseMap.points():         %d voxels, %d bytes: median %.1f ms [min %.1f, max %.1f] per call (wall)"
          % (len(p), p.nbytes, np.median(t), t.min(), t.max()), flush=True)
    print("the field with nothing back costs %.3f ms against %.1f ms for the download: %s"
          % (med_none, np.median(t), "less" if med_none < np.median(t) else "NOT LESS"), flush=True)
    assert med_none < np.median(t), "the field with nothing back must cost less than download()"
d.close()
