"""Dense map, connected components (loamx_densemap_segment): the synthetic terrain of scripts/bench_densemap_grid.py (--side x --side
voxels at --leaf: a rolling ground of one voxel per column, two points each, and --pillars random pillars of ten voxels on it, about
a million voxels at the default side of 1000) is added from the host; then the blocking call is timed at the three connectivities,
with and without labels (median, min, max of --reps, the first call apart: it allocates the work arrays), and beside it, in the same
run, download(): the cost of merely getting the voxels to a clusterer on the host.  Where scipy is importable, scipy.ndimage.label on
the dense window of the same voxels is timed too (without the time to build that window).  Needs a device."""
import argparse, ctypes as C, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=1000)
ap.add_argument("--leaf", type=float, default=0.125)
ap.add_argument("--pillars", type=int, default=2000)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--download-reps", type=int, default=5)
args = ap.parse_args()

from loam_velodyne_amd import loamx

rng = np.random.default_rng(1)
n = args.side
ix, iz = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
height = np.floor(3.0 * np.sin(ix / 40.0) + 2.0 * np.cos(iz / 55.0)).astype(np.int64)   # a rolling ground, steps of one leaf
px, pz = rng.integers(0, n, args.pillars), rng.integers(0, n, args.pillars)
cols = [np.stack([ix.ravel(), height.ravel(), iz.ravel()], axis=1)]
for k in range(1, 11):
    cols.append(np.stack([px, height[px, pz] + k, pz], axis=1))
vox = np.concatenate(cols)
pts = np.zeros((2 * len(vox), 4), np.float32)
pts[:, :3] = (np.repeat(vox, 2, axis=0) + rng.uniform(0.1, 0.9, (2 * len(vox), 3))) * args.leaf

d = loamx.DenseMap(leaf=args.leaf, initial_slots=1 << 22)
t0 = time.perf_counter()
for k in range(0, len(pts), 1 << 21):
    d.add(pts[k:k + (1 << 21)], (0.0, 0.0, 0.0))
st = d.stats()
print("map: %d points, %d voxels, %d slots in %.1f s" % (len(pts), st["voxels"], st["slots"], time.perf_counter() - t0), flush=True)

t0 = time.perf_counter()
labels, segs, stats = d.segment()
print("first call (allocates the work arrays): %.1f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)

# the C call alone, into arrays that stand
L = loamx.lib()
lab = np.zeros(st["voxels"], np.uint32)
rec = np.zeros(st["voxels"], loamx.SEGMENT)
for conn in (6, 18, 26):
    cfg = loamx.SegmentConfig(connectivity=conn)
    for with_labels in (True, False):
        nv, ns, s6 = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 6)()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rc = L.loamx_densemap_segment(d.h, C.byref(cfg), None, lab.ctypes.data_as(C.c_void_p) if with_labels else None, C.c_uint64(len(lab)),
                                          C.byref(nv), rec.ctypes.data_as(C.c_void_p), C.c_uint64(len(rec)), C.byref(ns), s6)
            times.append(time.perf_counter() - t0)
            assert rc == loamx.OK
        t = np.array(times) * 1e3
        print("loamx_densemap_segment connectivity %2d, %s: median %.2f ms [min %.2f, max %.2f] per call (wall); %d components, largest %d, "
              "%d hooks lost in the last call" % (conn, "labels   " if with_labels else "no labels", np.median(t), t.min(), t.max(), ns.value,
                                                  s6[4], s6[5]), flush=True)

times = []
for _ in range(args.download_reps):
    t0 = time.perf_counter()
    p = d.points()
    times.append(time.perf_counter() - t0)
t = np.array(times) * 1e3
print("DenseMap.points():     %d voxels, %d bytes: median %.1f ms [min %.1f, max %.1f] per call (wall)"
      % (len(p), p.nbytes, np.median(t), t.min(), t.max()), flush=True)
d.close()

try:
    from scipy import ndimage
except ImportError:
    print("scipy is not importable here: scipy.ndimage.label was not measured")
else:
    lo = vox.min(axis=0)
    dense = np.zeros(tuple(vox.max(axis=0) - lo + 1), bool)
    dense[tuple((vox - lo).T)] = True
    for conn, rank in ((6, 1), (18, 2), (26, 3)):
        structure = ndimage.generate_binary_structure(3, rank)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            _, count = ndimage.label(dense, structure)
            times.append(time.perf_counter() - t0)
        print("scipy.ndimage.label connectivity %2d on the dense %s window: median %.1f ms, %d components (the window given)"
              % (conn, dense.shape, np.median(times) * 1e3, count), flush=True)
