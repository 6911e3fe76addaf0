"""Dense global map (loamx_densemap_*): the add of HDL-64E revolutions (131,072 points) — host-fed and from a mapper's registered cloud —
and the sequential live VLP-16 chain (linked entry points, 200 k-pt live map, one sweep in flight, pinned host memory in and out) with and
without a dense map attached.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel times (k_dm_insert, k_dm_rehash).
BENCH_DENSEMAP_LIVE=<sweeps> sets the timed sweeps of each live run (default 150, 10 warm-up sweeps in front)."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx, synth


# ---- host-fed HDL-64E revolutions along a drive (origins 1 m apart)
w = synth.World()
sw = synth.make_sweep(w, "HDL-64E", np.zeros(6), np.array([0, 0.01, 0, 0.2, 0, 1.0]), seed=1)
pts = loamx.pinned_copy(sw.points)
n = len(pts)
K = 40
for combine in (True, False, True, False):   # (A/B of the in-wave combining of equal keys, alternated)
    d = loamx.DenseMap(leaf=0.1)
    d.set_combine(combine)
    d.add(pts, (0, 0, 0))
    d.stats()                                  # (warm-up, and a wait for it)
    shifted = [pts.copy() for _ in range(4)]
    for j, s in enumerate(shifted):
        s[:, 2] += np.float32(1.0 + j)
    t0 = time.perf_counter()
    for k in range(K):
        d.add(shifted[k % 4], (0, 0, 1.0 + k % 4))
    st = d.stats()                             # (waits for every add)
    dt = (time.perf_counter() - t0) / K
    print("host add    HDL-64E %d pts  combine=%d  %.1f us/sweep (host staging + H2D + insert, wall)  voxels %d  slots %d  rehashes %d"
          % (n, combine, dt * 1e6, st["voxels"], st["slots"], d.rehashes))
    d.close()

# ---- from the mapper: HDL-64E revolutions through the host-message chain, the registered cloud added where it lies
cm, sm = w.make_map(300_000)
poses = synth.trajectory(12)
hsw = [synth.make_sweep(w, "HDL-64E", poses[t], poses[t + 1], seed=70 + t) for t in range(12)]
sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
mp.load_cubes(cm, sm)
d = loamx.DenseMap(leaf=0.1)
enq = []
for t, s in enumerate(hsw):
    f = sr.process(s.points, s.ring_sizes)
    od.process(f)
    lc, ls = od.last_clouds()
    full = od.transform_to_end(f["full"])
    mp.update_odometry(od.transform_sum)
    mp.process(lc, ls, full)
    a = time.perf_counter()
    d.add_from(mp)
    enq.append(time.perf_counter() - a)
st = d.stats()
print("add_from_map HDL-64E  %d sweeps  host time of the call %.1f us (median; enqueue only)  voxels %d  slots %d  rehashes %d"
      % (len(hsw), np.median(enq[2:]) * 1e6, st["voxels"], st["slots"], d.rehashes))
d.close()

# ---- live VLP-16 chain, with and without a dense map attached (alternated: A B A B)
KL = int(os.environ.get("BENCH_DENSEMAP_LIVE", "150"))
W = 10
T = 1 + W + KL
wl = synth.World(half_extent=65.0)
lcm, lsm = wl.make_map(200_000)
lposes = synth.trajectory(T)
lsw = [synth.make_sweep(wl, "VLP-16", lposes[t], lposes[t + 1], seed=500 + t) for t in range(T)]
lpts = [loamx.pinned_copy(s.points) for s in lsw]
landing = loamx.pinned_empty((max(len(s.points) for s in lsw), 4))


def live(dense):
    import gc
    sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
    mp.load_cubes(lcm, lsm)
    d = loamx.DenseMap(leaf=0.1) if dense else None
    gc.collect()
    gc.disable()
    t0 = None
    for t in range(T):
        if t == 1 + W:
            t0 = time.perf_counter()
        sr.process_linked(lpts[t], lsw[t].ring_sizes)
        od.process_linked(sr)
        mp.process_linked(od, landing)
        if d is not None:
            d.add_from(mp)
    if d is not None:
        voxels = len(d)   # (waits for the adds: inside the timed region)
    dt = time.perf_counter() - t0
    gc.enable()
    rate = KL / dt
    extra = "  voxels %d  rehashes %d" % (voxels, d.rehashes) if d is not None else ""
    return rate, extra


rates = {False: [], True: []}
for dense in (False, True, False, True, False, True):
    r, extra = live(dense)
    rates[dense].append(r)
    print("live VLP-16  dense map %-3s  %.0f sweeps/s%s" % ("on" if dense else "off", r, extra))
off, on = np.median(rates[False]), np.median(rates[True])
print("live VLP-16 median: off %.0f sweeps/s  on %.0f sweeps/s  (%+.1f %%)" % (off, on, 100.0 * (on / off - 1.0)))
