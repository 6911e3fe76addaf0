"""Dense map, frontiers of the navigation grid (loamx_densemap_frontiers_cells): a synthetic --window x --window grid (default 2048, the
routing limit, then 512) of explored ground: FREE where a smooth field of a few sines is above a threshold, UNKNOWN elsewhere,
--pillars random OBSTACLE cells in it, clear2 121 off the obstacles; the start at the free cell nearest the window's centre.  Wall times
of the blocking C calls into arrays that stand, median [min, max] of --reps:
  loamx_densemap_frontiers_cells without a start (the upload of the records and the frontier stages), records back, and with labels;
  loamx_densemap_frontiers_cells with a start (the upload, the route, the frontier stages);
  loamx_densemap_route_cells alone, nothing back, on the same grid (the upload and the route: this pull request changes nothing in it);
  the upload alone and the fetch of both record arrays (24 and 8 bytes per cell) to pinned host memory, which is what a host-side
  implementation pays before it starts, by torch copies.
The frontier stages alone, by the wall clock: the call with a start and route_cells alone alternated --reps times, the median of the
paired differences (both contain the same upload, the same check of every cls on the host and the same route; a call without a start
less a torch upload is printed as well, but that difference still holds the host's check and the library's own upload).  By the
device's clock: `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/bench_densemap_frontier.py --windows 2048
--no-copies`, then `--summarise DIR` (no device needed) prints the median time of each frontier kernel over the launches of that run.
There is no reference implementation to race: no time is gated."""
import argparse, csv, glob, ctypes as C, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--windows", default="2048,512")
ap.add_argument("--pillars-per-mcell", type=int, default=2000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-copies", action="store_true", help="leave the torch copies out (a profiled run)")
ap.add_argument("--summarise", default=None, metavar="DIR", help="print the kernel times of the kernel_trace.csv files under DIR and exit")
args = ap.parse_args()

KERNELS = ("k_dm_fr_mark", "k_dm_fr_link", "k_dm_fr_flatten", "k_scan_chained", "k_dm_fr_totals", "k_dm_fr_ids", "k_dm_fr_reduce", "k_dm_fr_labels")


def summarise(root):
    paths = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True))
    assert paths, "no kernel_trace.csv under " + root
    for path in paths:
        rows = list(csv.DictReader(open(path)))
        name_col = next(k for k in rows[0] if k.lower() in ("kernel_name", "name"))
        start_col = next(k for k in rows[0] if k.lower().startswith("start"))
        end_col = next(k for k in rows[0] if k.lower().startswith("end"))
        print("device times from %s" % path)
        grid_cols = [k for k in rows[0] if k.lower().startswith("grid_size")]
        sizes = sorted({tuple(int(x[k]) for k in grid_cols) for x in rows if "k_dm_fr_mark" in x[name_col]}, reverse=True)
        for size in sizes:   # one window per launch shape of k_dm_fr_mark: the launches between two of its are that window's
            total, window = 0.0, None
            per = {name: [] for name in KERNELS}
            for x in rows:
                if "k_dm_fr_mark" in x[name_col]:
                    window = tuple(int(x[k]) for k in grid_cols)
                for name in KERNELS:
                    if name in x[name_col] and window == size:
                        per[name].append((int(x[end_col]) - int(x[start_col])) / 1e3)
            print("window of %d x %d cells:" % (size[0] // 256 * 32, size[1] * 32))
            for name in KERNELS:
                t = np.array(per[name][1:])   # (without the first launch)
                if not len(t):
                    print("  %-18s no launches" % (name + ":"))
                    continue
                total += np.median(t)
                print("  %-18s median %8.1f us [min %.1f, max %.1f] over %d launches" % (name + ":", np.median(t), t.min(), t.max(), len(t)))
            print("  %-18s %8.1f us (sum of the medians; k_dm_fr_labels runs only when labels are wanted)" % ("these kernels:", total))


if args.summarise:
    summarise(args.summarise)
    sys.exit(0)

if not args.no_copies:
    import torch
from loam_velodyne_amd import loamx

L = loamx.lib()
d = loamx.DenseMap(leaf=0.125, initial_slots=1024)   # an empty map: the calls need a handle, not its voxels


def timed(call, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert call() == loamx.OK
        t.append(time.perf_counter() - t0)
    return np.array(t) * 1e3


def line(name, t, tail=""):
    print("%-58s median %8.2f ms [min %.2f, max %.2f] of %d (wall)%s" % (name + ":", np.median(t), t.min(), t.max(), len(t), tail), flush=True)
    return float(np.median(t))


for W in [int(w) for w in args.windows.split(",")]:
    rng = np.random.default_rng(3)
    x, z = np.meshgrid(np.arange(W), np.arange(W), indexing="xy")
    f = np.sin(x / 37.0) * np.cos(z / 53.0) + 0.6 * np.sin((x + 2 * z) / 91.0) + 0.4 * np.cos((3 * x - z) / 29.0)
    cls = np.where(f > -0.3, loamx.GRID_FREE, loamx.GRID_UNKNOWN).astype(np.uint32)
    n_p = args.pillars_per_mcell * W * W // (1 << 20)
    cls[rng.integers(0, W, n_p), rng.integers(0, W, n_p)] = loamx.GRID_OBSTACLE
    cells = np.zeros((W, W), loamx.GRID_CELL)
    cells["cls"] = cls
    cells["clear2"] = np.where(cls == loamx.GRID_OBSTACLE, 0, 121)
    free = np.argwhere(cls == loamx.GRID_FREE)
    s = free[np.argmin(((free - W // 2) ** 2).sum(axis=1))]
    start = np.array([s[1], s[0]], np.uint32)
    goals = start.reshape(1, 2).copy()
    labels = np.zeros((W, W), np.uint32)
    out = np.zeros(1 << 20, loamx.FRONTIER)
    n_fr = C.c_uint64(0)
    stats, rstats = (C.c_uint64 * 6)(), (C.c_uint64 * 6)()
    cp, sp, gp = cells.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p), goals.ctypes.data_as(C.c_void_p)
    lp, op, cap = labels.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_uint64(len(out))

    def frontiers(start_p, labels_p):
        return L.loamx_densemap_frontiers_cells(d.h, cp, W, W, None, None, start_p, labels_p, op, cap, C.byref(n_fr), stats)

    def route_alone():
        return L.loamx_densemap_route_cells(d.h, cp, W, W, None, gp, 1, None, rstats)

    t0 = time.perf_counter()
    assert frontiers(sp, lp) == loamx.OK
    print("\n%d x %d: first call (allocates) %.1f ms; %s, %d reachable; free %d, unknown %d, obstacle %d"
          % (W, W, (time.perf_counter() - t0) * 1e3, dict(zip(loamx.FRONTIER_STATS, stats)), stats[4], (cls == 1).sum(), (cls == 0).sum(),
             (cls == 2).sum()), flush=True)
    a = line("frontiers_cells, no start, records back", timed(lambda: frontiers(None, None), args.reps), "; hooks lost %d" % stats[5])
    line("frontiers_cells, no start, records and labels back", timed(lambda: frontiers(None, lp), args.reps))
    c = line("frontiers_cells with a start, records back", timed(lambda: frontiers(sp, None), args.reps))
    b = line("route_cells alone, nothing back", timed(route_alone, args.reps), "; %d rounds" % rstats[4])
    pairs = np.array([(timed(lambda: frontiers(sp, None), 1)[0], timed(route_alone, 1)[0]) for _ in range(args.reps)])
    line("with a start less route_cells alone, alternated", pairs[:, 0] - pairs[:, 1])
    if args.no_copies:
        continue
    # what a host-side implementation pays first: both record arrays down to pinned memory; and the upload the lines above contain
    n = W * W
    dev24, dev8 = torch.empty(n * 24, dtype=torch.uint8, device="cuda"), torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    pin24, pin8 = torch.empty(n * 24, dtype=torch.uint8).pin_memory(), torch.empty(n * 8, dtype=torch.uint8).pin_memory()
    src = torch.from_numpy(cells.view(np.uint8).reshape(-1))

    def fetch():
        pin24.copy_(dev24, non_blocking=True)
        pin8.copy_(dev8, non_blocking=True)
        torch.cuda.synchronize()
        return loamx.OK

    def upload():
        dev24.copy_(src)
        torch.cuda.synchronize()
        return loamx.OK

    fetch(), upload()
    g = line("fetch of %d + %d MiB to pinned memory" % (n * 24 >> 20, n * 8 >> 20), timed(fetch, args.reps))
    u = line("upload of %d MiB from pageable memory" % (n * 24 >> 20), timed(upload, args.reps))
    print("frontier stages alone: %.2f ms (no start, less the upload), %.2f ms (with a start, less route_cells alone); the fetch: %.2f ms"
          % (a - u, c - b, g), flush=True)
    del dev24, dev8, pin24, pin8
d.close()
