"""Dense map, regions and paging (loamx_densemap_download_region / evict / page): a lattice map of --side^3 voxels (default 100^3 =
1 M) with --per-voxel points each, host-fed in chunks, and a window of --window^3 voxels in its middle (22^3 = about 1 % of 100^3).
In one process, alternated, --rounds of each; prints the median and the range of the wall times (each call ends in a device
synchronise):
  region_points(window)   against points() of the whole map on the same handle
  evict(outside, file)    followed by merge_file(file), which restores the map for the next round (timed apart)
  page                    the first call (everything but the keep box leaves) and then one step per round, the centre one tile further
The device times of k_dm_count, k_dm_compact and k_dm_rehash come from running it under `rocprofv3 --kernel-trace --stats` in a run of
its own (the REGION instantiations carry `true` as their last template argument)."""
import argparse, json, os, shutil, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=100)
ap.add_argument("--per-voxel", type=int, default=2)
ap.add_argument("--window", type=int, default=22)
ap.add_argument("--tile", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--moments", type=int, default=1)
ap.add_argument("--json", default="")
args = ap.parse_args()

rng = np.random.default_rng(11)
side, leaf = args.side, args.leaf
cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
d = loamx.DenseMap(leaf=leaf, initial_slots=1 << 20)
if args.moments:
    d.enable_moments()
origin = (0.5 * side * leaf,) * 3
for k in range(args.per_voxel):
    for part in np.array_split(rng.permutation(len(cells)), 8):
        p = np.zeros((len(part), 4), np.float32)
        p[:, :3] = (cells[part] + rng.uniform(0.2, 0.8, (len(part), 3))) * leaf
        d.add(p, origin)
lo = (side - args.window) // 2
window = loamx.DenseMapRegion([lo] * 3, [lo + args.window - 1] * 3)
n_all, (n_win, pts_win) = len(d), d.count_region(window)
print("map: %d voxels, %d slots, moments %d; window: %d voxels (%.2f %%), %d points" % (
    n_all, d.stats()["slots"], args.moments, n_win, 100.0 * n_win / n_all, pts_win), flush=True)
assert n_all == side ** 3 and n_win == args.window ** 3


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


work = tempfile.mkdtemp(prefix="lxdm_bench_")
T = {k: [] for k in ("region_points", "points", "evict", "merge_file", "page_step")}
try:
    path = os.path.join(work, "out.lxdm")
    d.region_points(window), d.points()    # warm-up: code objects, first allocations
    for r in range(args.rounds):
        ms, sub = timed(lambda: d.region_points(window))
        T["region_points"].append(ms)
        ms, whole = timed(lambda: d.points())
        T["points"].append(ms)
        assert len(sub) == n_win and len(whole) == n_all
        ms, removed = timed(lambda: d.evict(window.outside(), path))
        T["evict"].append(ms)
        assert removed[0] == n_all - n_win and len(d) == n_win
        ms, _ = timed(lambda: d.merge_file(path))
        T["merge_file"].append(ms)
        assert len(d) == n_all
    tiles = os.path.join(work, "tiles")
    os.mkdir(tiles)
    cfg = loamx.DenseMapPageConfig(tiles, args.tile, (1, 1, 1))
    span = args.tile * leaf
    c0 = 2.5 * span
    first_ms, st = timed(lambda: d.page(cfg, (c0, c0, c0)))
    print("page, first call: %.1f ms  %s" % (first_ms, st), flush=True)
    for r in range(args.rounds):
        ms, st = timed(lambda: d.page(cfg, (c0 + (r + 1) * span, c0, c0)))
        T["page_step"].append(ms)
        print("page, step %d: %.1f ms  %s" % (r, ms, st), flush=True)
finally:
    shutil.rmtree(work, ignore_errors=True)

out = dict(voxels=n_all, window_voxels=n_win, moments=args.moments, page_first_ms=first_ms)
for k, v in T.items():
    out[k] = dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), n=len(v))
    print("%-14s median %.2f ms  range %.2f .. %.2f ms  (n = %d)" % (k, out[k]["median_ms"], out[k]["min_ms"], out[k]["max_ms"], len(v)), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
