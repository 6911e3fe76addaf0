"""Dense map, native save / load and merge (loamx_densemap_save, _load, _merge, _merge_file): the noisy ground plane of
scripts/bench_densemap_align.py, --side x --side metres at --leaf with moments on (100 m at 0.1 m: about a million voxels), as two
maps that overlap by half — A holds the strip x in [0, 2/3 side], B the strip [1/3 side, side] — and as their merge, the whole plane.
Prints medians of --reps wall times (each call blocks until its result stands) of: save and load of the whole plane; merge of B into
a copy of A; merge_file of B's file into a copy of A.  For comparison, from the same run and on the unchanged growth path: one add
that forces the table of the whole plane to double (and the same add again, which does not: the difference is the growth rehash),
and the re-adding of B's sweeps from the host into a copy of A, which is what a merge replaces."""
import argparse, os, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=float, default=100.0)
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--per-voxel", type=float, default=12.0)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

rng = np.random.default_rng(1)
origin = np.float32([args.side / 2, args.side / 2, 2.0])


def strip(x0, x1):
    """the sweeps of the strip x in [x0, x1) of the plane: chunks of at most 2^21 points"""
    total = int(args.per_voxel * (x1 - x0) * args.side / args.leaf ** 2)
    out = []
    for k in range(0, total, 1 << 21):
        n = min(1 << 21, total - k)
        p = np.zeros((n, 4), np.float32)
        p[:, 0] = rng.uniform(x0, x1, n)
        p[:, 1] = rng.uniform(0.0, args.side, n)
        p[:, 2] = args.leaf / 2 + rng.normal(0.0, args.leaf / 10, n)
        out.append(p)
    return out


def fresh():
    d = loamx.DenseMap(leaf=args.leaf, initial_slots=1 << 20)
    d.enable_moments()
    return d


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def report(name, times, note=""):
    q = np.percentile(np.array(times), [0, 50, 100])
    print("%-34s %9.1f ms  [%.1f, %.1f]%s" % (name, q[1], q[0], q[2], note), flush=True)


tmp = tempfile.mkdtemp(prefix="lxdm_bench_")
file_a, file_b, file_all = (os.path.join(tmp, n) for n in ("a.lxdm", "b.lxdm", "all.lxdm"))
sweeps_a, sweeps_b = strip(0.0, args.side * 2 / 3), strip(args.side / 3, args.side)
a, b = fresh(), fresh()
for d, sw in ((a, sweeps_a), (b, sweeps_b)):
    for p in sw:
        d.add(p, origin)
a.save(file_a)
b.save(file_b)
print("A: %d voxels in %d slots, B: %d voxels in %d slots; files of %.1f and %.1f MB"
      % (len(a), a.stats()["slots"], len(b), b.stats()["slots"], os.path.getsize(file_a) / 1e6, os.path.getsize(file_b) / 1e6), flush=True)


def copy_of_a():
    d = fresh()
    d.load(file_a)
    return d


t_merge, t_merge_file, t_readd = [], [], []
for _ in range(args.reps):
    d = copy_of_a()
    t_merge.append(timed(lambda: d.merge(b)))
    whole, slots = len(d), d.stats()["slots"]
    if _ == 0:
        d.save(file_all)
    d.close()
    d = copy_of_a()
    t_merge_file.append(timed(lambda: d.merge_file(file_b)))
    assert len(d) == whole
    d.close()
    d = copy_of_a()

    def readd():
        for p in sweeps_b:
            d.add(p, origin)
        d.stats()    # (waits for the adds)
    t_readd.append(timed(readd))
    assert len(d) == whole
    d.close()
print("the whole plane: %d voxels in %d slots, a file of %.1f MB" % (whole, slots, os.path.getsize(file_all) / 1e6), flush=True)

t_save, t_load, t_grow, t_same = [], [], [], []
for _ in range(args.reps):
    d = fresh()
    t_load.append(timed(lambda: d.load(file_all)))
    t_save.append(timed(lambda: d.save(os.path.join(tmp, "again.lxdm"))))
    st = d.stats()
    n = st["slots"] // 2 - st["voxels"] + 1    # the smallest call the host must double the table for
    p = sweeps_b[0][:n]
    r0 = d.rehashes

    def add():
        d.add(p, origin)
        d.stats()
    t_grow.append(timed(add))
    assert d.rehashes == r0 + 1 and d.stats()["slots"] == 2 * st["slots"]
    t_same.append(timed(add))
    assert d.rehashes == r0 + 1
    d.close()

report("save (whole plane)", t_save)
report("load (whole plane)", t_load)
report("merge B into A", t_merge)
report("merge_file B's file into A", t_merge_file)
report("re-add B's sweeps into A", t_readd, "   (%d points from the host)" % sum(len(p) for p in sweeps_b))
report("add that doubles the table", t_grow, "   (%d points into %d slots)" % (n, st["slots"]))
report("the same add again (no doubling)", t_same)
print("growth rehash of the whole plane's table ~ %.1f ms (difference of the two medians)" % (np.median(t_grow) - np.median(t_same)), flush=True)
for f in os.listdir(tmp):
    os.remove(os.path.join(tmp, f))
os.rmdir(tmp)
