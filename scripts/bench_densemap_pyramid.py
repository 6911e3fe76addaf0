"""Dense map, coarser levels (loamx_densemap_coarsen, loamx_densemap_freeze_pyramid): a noisy ground plane of --side x --side metres
at --leaf (100 m at 0.1 m: about a million voxels) is added from the host, then --phase picks what is timed (wall, the calls block):
  freeze     loamx_densemap_freeze
  pyramid1   loamx_densemap_freeze_pyramid with levels = 1 (the same launches and copies as freeze: compare the two runs' kernel traces)
  pyramid3   loamx_densemap_freeze_pyramid with levels = 3
  coarsen    loamx_densemap_coarsen at levels 1, 2, 3 (cascade + download of the level)
Device times come from a run of its own under `rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -- python
scripts/bench_densemap_pyramid.py --phase pyramid3`; --trace DIR then prints, per kernel, its launches and time, the dispatches of
k_dm_coarsen one by one in launch order (level 1, level 2, ...), and the totals of launches and copies."""
import argparse, csv, glob, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=float, default=100.0)
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--per-voxel", type=float, default=8.0)
ap.add_argument("--phase", choices=("freeze", "pyramid1", "pyramid3", "coarsen"), default="pyramid3")
ap.add_argument("--trace", help="summarise the kernel trace rocprofv3 wrote under this directory instead of running")
args = ap.parse_args()

if args.trace:
    rows = []
    for path in glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, t in sorted(per.items()):
        shown = ", ".join("%.1f" % x for x in t) if "coarsen" in name else "%.1f total" % sum(t)
        print("%-60s %4d launches  us: %s" % (name[:60], len(t), shown))
    copies = sum(len(list(csv.DictReader(open(p)))) for p in glob.glob(os.path.join(args.trace, "**", "*memory_copy_trace.csv"), recursive=True))
    print("kernel launches %d, memory copies %d (with --memory-copy-trace)" % (len(rows), copies))
    sys.exit(0)

from loam_velodyne_amd import loamx

rng = np.random.default_rng(1)


def ground(n):
    p = np.zeros((n, 4), np.float32)
    p[:, :2] = rng.uniform(0.0, args.side, (n, 2))
    p[:, 2] = args.leaf / 2 + rng.normal(0.0, args.leaf / 10, n)
    return p


d = loamx.DenseMap(leaf=args.leaf, initial_slots=1 << 22)
d.enable_moments()
total = int(args.per_voxel * (args.side / args.leaf) ** 2)
origin = np.float32([args.side / 2, args.side / 2, 2.0])
t0 = time.perf_counter()
for k in range(0, total, 1 << 21):
    d.add(ground(min(1 << 21, total - k)), origin)
voxels = len(d)
print("map: %d points, %d voxels, %d slots in %.1f s" % (total, voxels, d.stats()["slots"], time.perf_counter() - t0), flush=True)

t0 = time.perf_counter()
if args.phase == "freeze":
    print("freeze: %d surfels in %.0f ms" % (d.freeze(), (time.perf_counter() - t0) * 1e3))
elif args.phase == "coarsen":
    for l in (1, 2, 3):
        t0 = time.perf_counter()
        keys, vals, mom = d.coarsen(l)
        print("coarsen level %d: %d voxels, %d points in %.0f ms" % (l, len(keys), int(vals[:, 0].sum()), (time.perf_counter() - t0) * 1e3), flush=True)
else:
    n = d.freeze_pyramid(levels=1 if args.phase == "pyramid1" else 3)
    print("freeze_pyramid levels %d: surfels %s in %.0f ms" % (len(n), n, (time.perf_counter() - t0) * 1e3))
d.close()
