"""Dense map, second moments (loamx_densemap_enable_moments): synthetic registered sweeps of one sensor along a drive, host-fed into a
dense map, alternating moments off and on (--rounds of each, a fresh map per round).  Prints the wall time per add and, for the maps
with moments, the wall time of one surfel export; the device times of k_dm_insert, k_dm_rehash and k_dm_compact come from running it
under `rocprofv3 --kernel-trace`, whose dispatches scripts/trace_by_kernel.py groups by kernel name (the template arguments in the
name tell the instantiations apart: the last one of k_dm_insert and k_dm_rehash is MOMENTS)."""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx, synth

ap = argparse.ArgumentParser()
ap.add_argument("--sensor", default="HDL-64E", choices=("HDL-64E", "VLP-16"))
ap.add_argument("--sweeps", type=int, default=60)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--initial-slots", type=int, default=1 << 20)
args = ap.parse_args()

w = synth.World()
poses = synth.trajectory(args.sweeps)
clouds = []
for t in range(args.sweeps):
    sw = synth.make_sweep(w, args.sensor, poses[t], poses[t + 1], seed=300 + t)
    p = loamx.pinned_copy(sw.points)
    origin = np.asarray(poses[t + 1][3:6], np.float32)
    p[:, :3] += origin   # (a map-frame cloud around a moving sensor)
    clouds.append((p, origin))
print("%s: %d sweeps of %d points, leaf %.2f" % (args.sensor, len(clouds), len(clouds[0][0]), args.leaf), flush=True)

for r in range(args.rounds):
    for moments in (False, True):
        d = loamx.DenseMap(leaf=args.leaf, initial_slots=args.initial_slots)
        if moments:
            d.enable_moments()
        t0 = time.perf_counter()
        for p, o in clouds:
            d.add(p, o)
        st = d.stats()   # (waits for every add)
        dt = (time.perf_counter() - t0) / len(clouds)
        line = "round %d moments %-3s  %.0f us/add (wall: staging + H2D + kernels)  voxels %d  slots %d  rehashes %d" % (
            r, "on" if moments else "off", dt * 1e6, st["voxels"], st["slots"], d.rehashes)
        if moments:
            t0 = time.perf_counter()
            s = d.surfels()
            line += "  surfel export %.0f ms for %d voxels (%d with a surfel)" % (
                (time.perf_counter() - t0) * 1e3, len(s), int(s[:, 4:7].any(axis=1).sum()))
            t0 = time.perf_counter()
            d.points()
            line += ", plain export %.0f ms" % ((time.perf_counter() - t0) * 1e3)
        print(line, flush=True)
        d.close()
