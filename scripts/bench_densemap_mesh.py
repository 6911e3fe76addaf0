"""Dense map, signed distance field and mesh (loamx_densemap_tsdf_*, loamx_densemap_mesh): one synthetic sweep of --points returns
from the walls of a box room of --room metres, seen from near its middle, into a --side^3 window of --leaf cells.  Prints, per
configuration, the wall time of one integration (median of --reps after a warm-up, the field cleared in between, the host waiting
for the device at the end of each): the band only and the whole ray, host-fed and from the sweep log (no copy up), and beside them
loamx_densemap_add of the same sweep with carving at ray_stride 1, the nearest existing kernel, into a fresh map each time.  Then the
mesh of the field: count-only and with the result brought back."""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=131072)
ap.add_argument("--side", type=int, default=256)
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--room", type=float, default=10.0, help="half extent of the room, metres")
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()

rng = np.random.default_rng(5)
origin = np.float32([0.3, -0.2, 0.1])
d = rng.normal(size=(args.points, 3))
d /= np.linalg.norm(d, axis=1, keepdims=True)
t = np.min((args.room * np.sign(d) - origin) / d, axis=1)      # the first wall each direction meets
pts = np.zeros((args.points, 4), np.float32)
pts[:, :3] = origin + d * t[:, None]
pts = loamx.pinned_copy(pts)
half = args.side // 2
cfg = dict(x0=-half, y0=-half, z0=-half, nx=args.side, ny=args.side, nz=args.side)
print("%d points, room +-%.1f m, window %d^3 of %.2f m cells" % (args.points, args.room, args.side, args.leaf), flush=True)


def median_ms(run, reset):
    times = []
    for k in range(args.reps + 1):
        reset()
        t0 = time.perf_counter()
        run()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times[1:]))


m = loamx.DenseMap(leaf=args.leaf)
m.enable_history(initial_points=args.points)
m.add(pts, origin)
m.stats()
for free_space in (0, 1):
    state = {}

    def reset():
        state["c"] = m.tsdf_begin(free_space=free_space, **cfg)
        m.tsdf(state["c"], want_w=False, want_d=False)      # (waits for the clear)

    host = median_ms(lambda: (m.tsdf_add(pts, origin), m.tsdf(state["c"], want_w=False, want_d=False)), reset)
    log = median_ms(lambda: m.tsdf_add_history(0, 1), reset)
    st = m.tsdf(state["c"], want_w=False, want_d=False)[2]
    print("tsdf free_space %d: %.3f ms host-fed (staging + H2D + kernel + stats), %.3f ms from the log; traced %d, cells visited %d, "
          "cells set %d, largest W %d" % (free_space, host, log, st["traced"], st["cells_visited"], st["cells_set"], st["max_weight"]), flush=True)
    if free_space == 0:
        band_host = host

carve = {}


def fresh():
    if "d" in carve:
        carve["d"].close()
    carve["d"] = loamx.DenseMap(leaf=args.leaf)
    carve["d"].enable_carving(ray_stride=1)
    carve["d"].stats()


ms = median_ms(lambda: (carve["d"].add(pts, origin), carve["d"].stats()), fresh)
cs = carve["d"].carve_stats()
print("add with carving, ray_stride 1: %.3f ms host-fed (insert + carve + stats); traced %d, cells visited %d" % (ms, cs["traced"], cs["cells_visited"]), flush=True)
print("rate against the carve: band %.2fx, whole ray %.2fx" % (band_host / ms, host / ms), flush=True)
carve["d"].close()

c = m.tsdf_begin(free_space=0, **cfg)
m.tsdf_add_history(0, 1)
count = median_ms(lambda: m.mesh(min_weight=1, count_only=True), lambda: None)
full = median_ms(lambda: m.mesh(min_weight=1), lambda: None)
nv, nt, st = m.mesh(min_weight=1, count_only=True)
print("mesh, min_weight 1: %.3f ms count-only, %.3f ms with %d vertices and %d triangles brought back (two calls: count, then fill); %s" % (count, full, nv, nt, st), flush=True)
m.close()
