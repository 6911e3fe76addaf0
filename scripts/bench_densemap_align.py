"""Dense map, alignment against the frozen snapshot (loamx_densemap_freeze, loamx_densemap_align_step): a noisy ground plane of
--side x --side metres at --leaf (100 m at 0.1 m: about a million surfels) is added from the host and frozen, then a cloud of
--points points on the same plane, seen from a slightly wrong pose, is linearised against it.  Prints the wall time of the freeze, of
one align_step call (staging of the host cloud + kernel + readback; the call blocks) and of one iteration of the align loop (the cloud
staged once; max_iterations iterations forced by eps = 0), for neighbourhood 0 and 1.  The device time of k_dm_align_step comes from
running it under `rocprofv3 --kernel-trace --stats`."""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=float, default=100.0)
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--per-voxel", type=float, default=12.0)
ap.add_argument("--points", type=int, default=131072)
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()

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
t1 = time.perf_counter()
n = d.freeze()
t2 = time.perf_counter()
print("map: %d points, %d voxels in %.1f s; freeze: %d surfels in %.0f ms" % (total, voxels, t1 - t0, n, (t2 - t1) * 1e3), flush=True)

cloud = loamx.pinned_copy(ground(args.points))
c = origin.astype(np.float64)
w = np.array([0.001, -0.0015, 0.002])
K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
R = np.eye(3) + K + 0.5 * K @ K
t = c + np.array([0.02, -0.03, 0.015])
rtc = np.concatenate([R.reshape(9), t, c]).astype(np.float32)
pose = np.concatenate([R, (t - R @ c)[:, None]], axis=1)
for nb in (0, 1, 0, 1):
    d.align_step(cloud, rtc, nb)   # (warm-up)
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        sums, counts = d.align_step(cloud, rtc, nb)
        times.append(time.perf_counter() - t0)
    q = np.percentile(np.array(times) * 1e6, [25, 50, 75])
    t0 = time.perf_counter()
    r = d.align(cloud, pose, centre=origin, neighbourhood=nb, max_iterations=args.reps, eps_rot=0.0, eps_trans=0.0)
    per_it = (time.perf_counter() - t0) / r["iterations"] * 1e6
    print("neighbourhood %d: align_step %.0f us [%.0f, %.0f] per call (wall), %.0f us per loop iteration (%d iterations); matched %d of %d"
          % (nb, q[1], q[0], q[2], per_it, r["iterations"], int(counts[4]), args.points), flush=True)
d.close()
