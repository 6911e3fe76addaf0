"""Dense map, navigation grid (loamx_densemap_grid): a synthetic terrain of --side x --side voxels at --leaf (a rolling ground of one
voxel per column, two points each, and --pillars random pillars of ten voxels on it: about a million voxels at the default side of
1000) is added from the host; then the blocking call is timed for a --window x --window window of cells of one voxel that covers the
terrain (median, min, max of --reps, the first call of the window's size apart), and beside it download(), the route a host has
without the grid: every voxel over PCIe, sorted, to be binned into columns on the host.

Device times come from a run of their own under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python
scripts/bench_densemap_grid.py --no-download`; `--summarise DIR` (no device needed) then prints the median time of each of the four
kernels over the calls of that run."""
import argparse, csv, glob, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=1000)
ap.add_argument("--leaf", type=float, default=0.125)
ap.add_argument("--pillars", type=int, default=2000)
ap.add_argument("--window", type=int, default=1024)
ap.add_argument("--clear-max", type=int, default=10)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--download-reps", type=int, default=5)
ap.add_argument("--no-download", action="store_true")
ap.add_argument("--summarise", default=None, metavar="DIR", help="print the kernel times of the kernel_trace.csv files under DIR and exit")
args = ap.parse_args()

KERNELS = ("k_dm_grid_ground", "k_dm_grid_fill", "k_dm_grid_classify", "k_dm_grid_clear")


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
            total += np.median(t)
            print("%-20s median %8.1f us [min %.1f, max %.1f] over %d launches" % (name + ":", np.median(t), t.min(), t.max(), len(t)))
        print("%-20s %8.1f us (sum of the medians)" % ("the four kernels:", total))


if args.summarise:
    summarise(args.summarise)
    sys.exit(0)

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

lo = (n - args.window) // 2
cfg = loamx.GridConfig(cell_leaves=1, x0=lo, z0=lo, nx=args.window, nz=args.window, clear_max=args.clear_max)
t0 = time.perf_counter()
g = d.grid(cfg)
print("first call (allocates the planes): %.1f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)
# the C call alone, into an array that stands (DenseMap.grid also allocates its result)
import ctypes as C
out = np.zeros((cfg.nz, cfg.nx), loamx.GRID_CELL)
times, times_py = [], []
for _ in range(args.reps):
    t0 = time.perf_counter()
    rc = loamx.lib().loamx_densemap_grid(d.h, C.byref(cfg), None, out.ctypes.data_as(C.c_void_p))
    times.append(time.perf_counter() - t0)
    assert rc == loamx.OK
    t0 = time.perf_counter()
    g = d.grid(cfg)
    times_py.append(time.perf_counter() - t0)
assert g.tobytes() == out.tobytes()
counts = [int((g["cls"] == k).sum()) for k in range(4)]
for name, t in (("loamx_densemap_grid", np.array(times) * 1e3), ("DenseMap.grid", np.array(times_py) * 1e3)):
    print("%-22s %d x %d cells, clear_max %d: median %.2f ms [min %.2f, max %.2f] per call (wall)"
          % (name + ":", cfg.nx, cfg.nz, cfg.clear_max, np.median(t), t.min(), t.max()), flush=True)
print("cells UNKNOWN %d, FREE %d, OBSTACLE %d, STEP %d; %d bytes per grid" % (*counts, g.nbytes), flush=True)
if not args.no_download:
    times = []
    for _ in range(args.download_reps):
        t0 = time.perf_counter()
        p = d.points()
        times.append(time.perf_counter() - t0)
    t = np.array(times) * 1e3
    print("DenseMap.points():     %d voxels, %d bytes: median %.1f ms [min %.1f, max %.1f] per call (wall)"
          % (len(p), p.nbytes, np.median(t), t.min(), t.max()), flush=True)
d.close()
