"""Dense map, free-space carving (loamx_densemap_enable_carving): synthetic registered sweeps of one sensor along a drive, host-fed into a
dense map, once per configuration: carving off, then ray_stride 1, 4, 16 (--configs).  Prints what the map counted per configuration
(rays, cells visited, misses) and the wall time per add; the device times of k_dm_insert and k_dm_carve come from running it under
`rocprofv3 --kernel-trace`, whose dispatches scripts/carve_trace_summary.py groups by configuration (each configuration launches the
same number of adds, in the order given here)."""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx, synth

ap = argparse.ArgumentParser()
ap.add_argument("--sensor", default="HDL-64E", choices=("HDL-64E", "VLP-16"))
ap.add_argument("--sweeps", type=int, default=100)
ap.add_argument("--configs", default="off,1,4,16", help="comma-separated: off, or a ray_stride")
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--max-steps", type=int, default=4096)
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

for cfg in args.configs.split(","):
    d = loamx.DenseMap(leaf=args.leaf)
    if cfg != "off":
        d.enable_carving(ray_stride=int(cfg), max_steps=args.max_steps)
    t0 = time.perf_counter()
    for p, o in clouds:
        d.add(p, o)
    st = d.stats()   # (waits for every add)
    dt = (time.perf_counter() - t0) / len(clouds)
    line = "config %-3s  %.0f us/add (wall: staging + H2D + kernels)  voxels %d  slots %d  rehashes %d" % (
        cfg, dt * 1e6, st["voxels"], st["slots"], d.rehashes)
    if cfg != "off":
        cs = d.carve_stats()
        line += "  traced %d  skipped stride/range/steps %d/%d/%d  cells visited %d  misses %d (%.2f %% of the cells visited)" % (
            cs["traced"], cs["skipped_stride"], cs["skipped_range"], cs["skipped_steps"], cs["cells_visited"], cs["misses"],
            100.0 * cs["misses"] / max(cs["cells_visited"], 1))
    print(line, flush=True)
    d.close()
