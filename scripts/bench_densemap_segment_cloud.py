"""Dense map, objects of a sweep that is not in the map (loamx_densemap_segment_cloud): the scene of
tests/test_gpu_densemap_segment_cloud.py::test_measured_on_a_sweep_against_the_terrain (one HDL-64E sweep of 131,072 points against
the million-voxel terrain), and --calls blocking calls with labels after --warmup.  Prints the wall time per call; meant to run
under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_densemap_segment_cloud.py` for the device
time per kernel, and with --trace FILE (a *_kernel_trace.csv written by such a run) it prints, per kernel, the launches per call and
the median [min, max] of the launches of the last --calls calls instead of running anything.  Needs a device unless --trace is given."""
import argparse, csv, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--margin", type=int, default=1)
ap.add_argument("--trace", default=None)
args = ap.parse_args()

if args.trace:
    rows = list(csv.DictReader(open(args.trace)))
    by = {}
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        by.setdefault(r["Kernel_Name"].split("(")[0], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    total = args.calls + args.warmup + 1      # (the scene's first call allocates)
    for name, t in sorted(by.items(), key=lambda kv: -np.median(kv[1])):
        per = len(t) // total
        if per == 0:
            continue      # not a kernel of the call (the adds that built the map)
        last = np.array(t[-per * args.calls:])
        print("%-48s %d per call: median %.1f us [min %.1f, max %.1f] over %d launches" % (name[-48:], per, np.median(last), last.min(), last.max(), len(last)))
    sys.exit(0)

from loam_velodyne_amd import loamx
from test_gpu_densemap_segment_cloud import terrain_and_sweep

leaf, pts, cloud, origin = terrain_and_sweep()
d = loamx.DenseMap(leaf=leaf, initial_slots=1 << 22)
for k in range(0, len(pts), 1 << 21):
    d.add(pts[k:k + (1 << 21)], (0.0, 0.0, 0.0))
labels, segs, st = d.segment_cloud(cloud, origin, margin=args.margin)     # the first call allocates
print("map: %d voxels; sweep: %s" % (len(d), st), flush=True)
times = []
for k in range(args.warmup + args.calls):
    t0 = time.perf_counter()
    d.segment_cloud(cloud, origin, margin=args.margin)
    times.append((time.perf_counter() - t0) * 1e3)
t = np.array(times[args.warmup:])
print("DenseMap.segment_cloud, NEW margin %d, with labels: median %.2f ms [min %.2f, max %.2f] per call (wall, through the binding)"
      % (args.margin, np.median(t), t.min(), t.max()), flush=True)
d.close()
