"""Dense map, alignment from many start poses (loamx_densemap_align_many) on the scene of bench_densemap_align.py: a noisy ground plane
of --side x --side metres at --leaf is added from the host and frozen, then clouds of --points points on the same plane are aligned
from K start poses (K of --poses), small perturbations of a pose 0.003 rad and 0.04 m off, for neighbourhood 0 and 1, with --iters
iterations forced (eps = 0, min_matched 0: every hypothesis runs every iteration).

--mode many: one align_many call for the K poses; --mode sequential: K calls of align (the only mode a library without the batched
functions can run; LOAMX_LIB selects the library).  Each row is the wall time of the whole call (the K calls), the cloud's staging
included, median [quartiles] of --reps repetitions, and that time per pose-iteration.  The device time of the two step kernels comes
from running the script alone under `rocprofv3 --kernel-trace --stats`."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("many", "sequential"), default="many")
ap.add_argument("--side", type=float, default=100.0)
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--per-voxel", type=float, default=12.0)
ap.add_argument("--points", type=int, nargs="+", default=[16384, 131072])
ap.add_argument("--poses", type=int, nargs="+", default=[1, 8, 64, 512])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--json", default=None, help="append one JSON line per row to this file")
args = ap.parse_args()

rng = np.random.default_rng(1)


def ground(n):
    p = np.zeros((n, 4), np.float32)
    p[:, :2] = rng.uniform(0.0, args.side, (n, 2))
    p[:, 2] = args.leaf / 2 + rng.normal(0.0, args.leaf / 10, n)
    return p


def exp_so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + K + 0.5 * K @ K if th < 1e-4 else np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * K @ K


d = loamx.DenseMap(leaf=args.leaf, initial_slots=1 << 22)
d.enable_moments()
total = int(args.per_voxel * (args.side / args.leaf) ** 2)
origin = np.float32([args.side / 2, args.side / 2, 2.0])
for k in range(0, total, 1 << 21):
    d.add(ground(min(1 << 21, total - k)), origin)
n = d.freeze()
print("map: %d points, %d voxels, %d surfels frozen; mode %s, library %s" % (total, len(d), n, args.mode, os.environ.get("LOAMX_LIB", "(in tree)")), flush=True)

c = origin.astype(np.float64)
cfg = dict(max_iterations=args.iters, eps_rot=0.0, eps_trans=0.0, min_matched=0)
prng = np.random.default_rng(2)
for n_points in args.points:
    cloud = loamx.pinned_copy(ground(n_points))
    for K in args.poses:
        poses = np.zeros((K, 3, 4))
        for k in range(K):
            R = exp_so3(np.array([0.001, -0.0015, 0.002]) + prng.normal(0.0, 0.001, 3))
            t = c + np.array([0.02, -0.03, 0.015]) + prng.normal(0.0, 0.01, 3)
            poses[k, :, :3], poses[k, :, 3] = R, t - R @ c
        for nb in (0, 1):
            times = []
            for rep in range(args.reps + 1):   # (the first is the warm-up)
                t0 = time.perf_counter()
                if args.mode == "many":
                    res, best = d.align_many(cloud, poses, centre=origin, neighbourhood=nb, **cfg)
                else:
                    res = [d.align(cloud, P, centre=origin, neighbourhood=nb, **cfg) for P in poses]
                times.append(time.perf_counter() - t0)
            assert all(r["iterations"] == args.iters for r in res)
            q = np.percentile(np.array(times[1:]) * 1e3, [25, 50, 75])
            row = dict(mode=args.mode, points=n_points, poses=K, neighbourhood=nb, ms=round(q[1], 4), q25=round(q[0], 4), q75=round(q[2], 4),
                       us_per_pose_iteration=round(q[1] * 1e3 / (K * args.iters), 3), matched=int(res[0]["counts"]["matched"]))
            print("%-10s points %6d  K %3d  nb %d: %9.3f ms [%9.3f, %9.3f]  %8.2f us per pose-iteration; matched %d"
                  % (args.mode, n_points, K, nb, q[1], q[0], q[2], row["us_per_pose_iteration"], row["matched"]), flush=True)
            if args.json:
                with open(args.json, "a") as f:
                    f.write(json.dumps(row) + "\n")
d.close()
