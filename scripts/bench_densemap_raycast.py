"""Dense map, ray casts (loamx_densemap_raycast): the noisy ground plane of scripts/bench_densemap_align.py (--side x --side metres at
--leaf) is added from the host, then two casts are measured from a pose 2 m above its middle: a sweep of rings x azimuths returns on
the plane (64 x 2048 = 131,072: every ray ends in the surface it hits) and the range image of the same directions at --max-range
(the rays go on through the plane: first hits well before their ends, and misses where they leave the map).  Prints the wall time of
the blocking call with and without records (median, min, max of --reps) and what the casts counted.

The yardstick is the carve kernel, which walks the same rays and adds atomics: a second handle with carving on receives the same
plane (from an origin so far above it that none of its rays is traced: n_steps > max_steps) and then --carve-reps times the sweep,
whose rays k_dm_carve walks.  Device times come from a run under `rocprofv3 --kernel-trace --output-format csv` of its own;
`--summarise kernel_trace.csv` then prints, from that file and the counts of a run of this script without the profiler, the median
device time of k_dm_raycast per cast and of k_dm_carve, each also per cell looked up."""
import argparse, csv, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=float, default=100.0)
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--per-voxel", type=float, default=12.0)
ap.add_argument("--rings", type=int, default=64)
ap.add_argument("--azimuths", type=int, default=2048)
ap.add_argument("--max-range", type=float, default=120.0)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--carve-reps", type=int, default=10)
ap.add_argument("--summarise", default=None, help="kernel_trace.csv of a profiled run with the same arguments (several: comma-separated)")
args = ap.parse_args()

CASTS = ("sweep, records", "sweep, counts only", "range image, records", "range image, counts only")

rng = np.random.default_rng(1)


def ground(n):
    p = np.zeros((n, 4), np.float32)
    p[:, :2] = rng.uniform(0.0, args.side, (n, 2))
    p[:, 2] = args.leaf / 2 + rng.normal(0.0, args.leaf / 10, n)
    return p


def build(d, origin):
    total = int(args.per_voxel * (args.side / args.leaf) ** 2)
    for k in range(0, total, 1 << 21):
        d.add(ground(min(1 << 21, total - k)), origin)
    return total


# the pose: LOAM axes (y up) turned so that the plane z = leaf / 2 of the map is the ground: sensor x -> map x, y -> z, z -> -y
origin = np.float32([args.side / 2, args.side / 2, 2.0])
pose = np.array([[1.0, 0.0, 0.0, origin[0]], [0.0, 0.0, -1.0, origin[1]], [0.0, 1.0, 0.0, origin[2]]])
elev = np.linspace(-24.8, -2.3, args.rings)   # (at -2.3 degrees a ray reaches the plane 49.8 m out: every return lies on the map)
image = loamx.range_image_ends(pose, elev, args.azimuths, args.max_range)
d_unit = (image[:, :3].astype(np.float64) - origin) / args.max_range
sweep = image.copy()
r = (origin[2] - args.leaf / 2 + rng.normal(0.0, args.leaf / 10, len(image))) / -d_unit[:, 2]   # range to the noisy plane
sweep[:, :3] = origin + d_unit * r[:, None]
n_rays = len(sweep)


def run():
    d = loamx.DenseMap(leaf=args.leaf, initial_slots=1 << 22)
    t0 = time.perf_counter()
    total = build(d, origin)
    print("map: %d points, %d voxels in %.1f s; %d rays per cast" % (total, len(d), time.perf_counter() - t0, n_rays), flush=True)
    results = {}
    for name, ends, records in zip(CASTS, (sweep, sweep, image, image), (True, False, True, False)):
        d.raycast(ends, origin, records=records)   # (warm-up: the buffers of the first cast)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rec, counts = d.raycast(ends, origin, records=records)
            times.append(time.perf_counter() - t0)
        t = np.array(times) * 1e6
        results[name] = counts
        print("%-26s %.0f us [min %.0f, max %.0f] per call (wall)  %s" % (name + ":", np.median(t), t.min(), t.max(), counts), flush=True)
        if records:
            hit = rec["status"] >= loamx.RAY_HIT
            print("%-26s median range of the hits %.2f m, median steps %d" % ("", np.median(rec["range"][hit]), np.median(rec["steps"][hit])),
                  flush=True)
    d.close()
    # the yardstick: the same sweep through k_dm_carve
    c = loamx.DenseMap(leaf=args.leaf, initial_slots=1 << 22)
    c.enable_carving(end_margin=0)
    build(c, np.float32([origin[0], origin[1], 1000.0]))
    before = c.carve_stats()
    assert before["traced"] == 0, before
    times = []
    for _ in range(args.carve_reps):
        c.stats()
        t0 = time.perf_counter()
        c.add(sweep, origin)
        c.stats()   # (waits for the add)
        times.append(time.perf_counter() - t0)
    after = c.carve_stats()
    cells = (after["cells_visited"] - before["cells_visited"]) // args.carve_reps
    print("carve yardstick: add of the sweep %.0f us per call (wall: staging, insert, carve, wait); cells visited per add %d, traced %d"
          % (np.median(times) * 1e6, cells, (after["traced"] - before["traced"]) // args.carve_reps), flush=True)
    c.close()
    return results, cells


def summarise(path, results, carve_cells):
    rows = list(csv.DictReader(open(path)))
    name_col = next(k for k in rows[0] if k.lower() in ("kernel_name", "name"))
    start_col = next(k for k in rows[0] if k.lower().startswith("start"))
    end_col = next(k for k in rows[0] if k.lower().startswith("end"))

    def durations(prefix):
        se = sorted((int(x[start_col]), int(x[end_col])) for x in rows if prefix in x[name_col])
        return np.array([(e - s) / 1e3 for s, e in se])

    cast, carve = durations("k_dm_raycast"), durations("k_dm_carve")
    per = args.reps + 1
    assert len(cast) == per * len(CASTS), (len(cast), per)
    for k, name in enumerate(CASTS):
        t = cast[k * per + 1:(k + 1) * per]
        cells = results[name]["cells"]
        print("k_dm_raycast, %-26s median %8.1f us [min %.1f, max %.1f]  %d cells: %.3f ns per cell"
              % (name + ":", np.median(t), t.min(), t.max(), cells, np.median(t) * 1e3 / cells))
    t = carve[-args.carve_reps:]
    print("k_dm_carve, the sweep:                  median %8.1f us [min %.1f, max %.1f]  %d cells: %.3f ns per cell"
          % (np.median(t), t.min(), t.max(), carve_cells, np.median(t) * 1e3 / carve_cells))


results, carve_cells = run()
for path in (args.summarise.split(",") if args.summarise else []):
    print("device times from %s" % path)
    summarise(path, results, carve_cells)
