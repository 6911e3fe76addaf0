"""Dense map, rebuild from corrected poses (loamx_densemap_enable_history, loamx_densemap_rebuild): the noisy ground plane of
scripts/bench_densemap_merge.py, --side x --side metres at --leaf with moments on (100 m at 0.1 m: about a million voxels), fed as
sweeps of --sweep points (131,072) with history on, once with carving off and once with carving on (--ray-stride).  Every logged sweep
gets a small random rigid correction (up to --rot rad about a random axis through the middle of the plane, up to one leaf of
translation).  Prints medians of --reps blocking wall times, alternated in one run, of:
  rebuild            loamx_densemap_rebuild under those corrections: the log replayed on the device;
  reset + re-add     what a host does without it: reset, then the host-transformed sweeps back over PCIe, one add at a time, and a wait
                     (the sweeps are already on the host and already transformed: the download of every registered sweep during the
                     run, which that host also pays, is not in the figure; the transform on the CPU is timed on its own).
Both leave the same map: the run checks that their exports and statistics are equal."""
import argparse, hashlib, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=float, default=100.0)
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--per-voxel", type=float, default=6.0)
ap.add_argument("--sweep", type=int, default=131072)
ap.add_argument("--rot", type=float, default=0.002)
ap.add_argument("--ray-stride", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

rng = np.random.default_rng(1)
origin = np.float32([args.side / 2, args.side / 2, 2.0])
total = int(args.per_voxel * args.side * args.side / args.leaf ** 2)
sweeps = []
for k in range(0, total, args.sweep):
    n = min(args.sweep, total - k)
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = rng.uniform(0.0, args.side, n)
    p[:, 1] = rng.uniform(0.0, args.side, n)
    p[:, 2] = args.leaf / 2 + rng.normal(0.0, args.leaf / 10, n)
    sweeps.append(p)


def rigid(w, t, centre):
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * (K @ K)
    return np.concatenate([R, (centre - R @ centre + t).reshape(3, 1)], axis=1)


middle = np.float64([args.side / 2, args.side / 2, args.leaf / 2])
corrections = []
for _ in sweeps:
    axis = rng.normal(size=3)
    corrections.append(rigid(axis / np.linalg.norm(axis) * rng.uniform(0.1, 1.0) * args.rot, rng.uniform(-args.leaf, args.leaf, 3), middle))
corrections = np.stack(corrections)


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def report(name, times, note=""):
    q = np.percentile(np.array(times), [0, 50, 100])
    print("  %-32s %9.1f ms  [%.1f, %.1f]%s" % (name, q[1], q[0], q[2], note), flush=True)


def view(d):
    st = d.stats()
    st.pop("slots")
    return st, hashlib.sha256(d.points().tobytes()).hexdigest(), hashlib.sha256(d.moments().tobytes()).hexdigest()


def fresh(carving, history):
    d = loamx.DenseMap(leaf=args.leaf, initial_slots=1 << 20)
    if carving:
        d.enable_carving(ray_stride=args.ray_stride)
    d.enable_moments()
    if history:
        d.enable_history()
    return d


for carving in (False, True):
    d, h = fresh(carving, True), fresh(carving, False)    # h: the handle of the host's path, as handles are without the log
    for p in sweeps:
        d.add(p, origin)
    st = d.stats()
    print("carving %s: %d sweeps, %d points, %d voxels in %d slots; the log holds %.1f MB"
          % ("on (ray_stride %d)" % args.ray_stride if carving else "off", len(sweeps), st["offered"], st["voxels"], st["slots"],
             d.history_size()[1] * 16 / 1e6), flush=True)
    t_rebuild, t_readd, t_transform, tables, moved = [], [], [], [], None
    for _ in range(args.reps):
        a = d.rebuild_stats()
        t_rebuild.append(timed(lambda: d.rebuild(corrections)))
        b = d.rebuild_stats()
        tables.append(b["tables_tried"] - a["tables_tried"])
        on_device = view(d) + ((d.carve_stats(), hashlib.sha256(d.misses().tobytes()).hexdigest()) if carving else ())

        def transform():
            global moved
            moved = [(loamx.correct(c, p), loamx.correct(c, origin.reshape(1, 3))[0]) for p, c in zip(sweeps, corrections)]
        t_transform.append(timed(transform))

        def readd():
            h.reset()
            for p, o in moved:
                h.add(p, o)
            h.stats()    # (waits for the adds)
        t_readd.append(timed(readd))
        from_host = view(h) + ((h.carve_stats(), hashlib.sha256(h.misses().tobytes()).hexdigest()) if carving else ())
        assert on_device == from_host, "the rebuilt map differs from the re-added one"
    st = d.stats()
    print("  under the corrections: %d voxels in %d slots; tables tried per rebuild: %s" % (st["voxels"], st["slots"], tables), flush=True)
    report("rebuild (on the device)", t_rebuild, "   (%d launches per table tried)" % ((b["launches"] - a["launches"]) // max(tables[-1], 1)))
    report("reset + re-add from the host", t_readd, "   (%d adds)" % len(sweeps))
    report("transform on the CPU (not in it)", t_transform)
    d.close()
    h.close()
