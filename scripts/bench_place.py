"""Place recognition (loamx_place_*): describe + add of VLP-16 / HDL-64E sweeps (with the dense map's add of the same sweeps beside it, as
the yardstick: both read the sweep once), queries against 1 k / 10 k / 100 k random entries (exhaustive, K = 10, K = 50), and the batched
step with and without add_from_pipeline after every step.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel times
(k_pl_*, k_dm_insert); one part per run keeps the sensors apart in the statistics:

    python scripts/bench_place.py [vlp16|hdl64|query|batch|all]

BENCH_PLACE_ENTRIES=1000,10000 shortens the query part; BENCH_PLACE_STEPS the timed steps of the batched part (default 30)."""
import os, struct, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx, synth

part = sys.argv[1] if len(sys.argv) > 1 else "all"
R, S = 20, 60


def add_part(sensor, az):
    w = synth.World()
    poses = synth.trajectory(4)
    sweeps = [loamx.pinned_copy(synth.make_sweep(w, sensor, poses[t], poses[t + 1], seed=t, az_steps=az).points) for t in range(4)]
    n = len(sweeps[0])
    K = 40
    db = loamx.PlaceDB()
    db.add(sweeps[0])
    db.descriptor(0)                           # (warm-up, and a wait for it)
    t0 = time.perf_counter()
    for k in range(K):
        db.add(sweeps[k % 4])
    db.descriptor(K)                           # (waits for every add)
    dt = (time.perf_counter() - t0) / K
    print("place add    %-8s %6d pts  %.1f us/sweep (host staging + H2D + describe + ring key, wall)" % (sensor, n, dt * 1e6))
    t0 = time.perf_counter()
    for k in range(K):
        db.query(sweeps[k % 4], n_results=5)
    dt = (time.perf_counter() - t0) / K
    print("place query  %-8s %6d pts  %.1f us/query against %d entries (staging + describe + search + wait, wall)" % (sensor, n, dt * 1e6, len(db)))
    d = loamx.DenseMap(leaf=0.1)               # the yardstick: k_dm_insert on the same sweeps in the same run
    d.add(sweeps[0])
    d.stats()
    t0 = time.perf_counter()
    for k in range(K):
        d.add(sweeps[k % 4])
    d.stats()
    dt = (time.perf_counter() - t0) / K
    print("dense add    %-8s %6d pts  %.1f us/sweep (host staging + H2D + insert, wall)" % (sensor, n, dt * 1e6))


def query_part():
    sizes = [int(x) for x in os.environ.get("BENCH_PLACE_ENTRIES", "1000,10000,100000").split(",")]
    rng = np.random.default_rng(0)
    nmax = max(sizes)
    desc = rng.uniform(0.0, 10.0, (nmax, R, S)).astype(np.float32)
    desc[rng.random((nmax, R, S)) < 0.4] = 0.0           # (empty cells, as real sweeps have them)
    keys = np.zeros((nmax, R), np.float32)
    for k in range(S):
        keys = keys + desc[:, :, k]
    keys = keys / np.float32(S)
    w = synth.World()
    q = loamx.pinned_copy(synth.make_sweep(w, "HDL-64E", np.zeros(6), np.zeros(6), seed=3, az_steps=1024).points)
    with tempfile.TemporaryDirectory() as tmp:
        for n in sizes:
            path = os.path.join(tmp, "db_%d.lxpl" % n)
            with open(path, "wb") as f:
                f.write(struct.pack("<5I3f", 0x4c50584c, 1, R, S, n, 80.0, 0.0, 2.0))
                f.write(desc[:n].tobytes())
                f.write(keys[:n].tobytes())
            for K in (0, 10, 50):
                db = loamx.PlaceDB(n_candidates=K, exclude_recent=0)
                db.load(path)
                db.query_entry(n - 1, n_results=5)       # warm-up
                reps = 20 if n <= 10000 else 5
                t0 = time.perf_counter()
                for i in range(reps):
                    res = db.query_entry(n - 1 - i, n_results=5)
                dt = (time.perf_counter() - t0) / reps
                t0 = time.perf_counter()
                for i in range(reps):
                    db.query(q, n_results=5)
                dq = (time.perf_counter() - t0) / reps
                print("query  %6d entries  %-12s  stored entry %.1f us   HDL-64E cloud %.1f us  (wall, result on the host)  best %s"
                      % (n, "exhaustive" if K == 0 else "K = %d" % K, dt * 1e6, dq * 1e6, res[0][:2]))
                db.close()
            os.remove(path)


def batch_part():
    ns = 4
    KS = int(os.environ.get("BENCH_PLACE_STEPS", "30"))
    W = 5
    T = W + KS
    w = synth.World(half_extent=45.0)
    cm, sm = w.make_map(60_000)
    sweeps, starts = [[None] * ns for _ in range(T)], []
    for s in range(ns):
        poses = synth.trajectory(T, step=0.3, start=(1.5 * s, 0.0, 2.0 * s))
        starts.append(np.array([0, 0, 0, 1.5 * s, 0, 2.0 * s], np.float32))
        for t in range(T):
            sw = synth.make_sweep(w, "VLP-16", poses[t], poses[t + 1], seed=30 * s + t, az_steps=900)
            sweeps[t][s] = (np.ascontiguousarray(sw.points, np.float32), sw.ring_sizes)

    def run(attach):
        p = loamx.Pipeline(ns)
        p.set_frozen(cm, sm)
        for s in range(ns):
            p.set_state(s, aft=starts[s])
        p.upload(sweeps)
        dbs = [loamx.PlaceDB() for _ in range(ns)] if attach else None
        t0 = None
        for t in range(T):
            if t == W:
                t0 = time.perf_counter()
            rc = p.step(t)
            if attach and rc == loamx.OK:
                for k in range(ns):
                    dbs[k].add_from_pipeline(p, k)
        if attach:
            for d in dbs:
                d.descriptor(len(d) - 1)   # (waits for the adds: inside the timed region)
        return (time.perf_counter() - t0) / KS

    times = {False: [], True: []}
    for attach in (False, True, False, True, False, True):
        dt = run(attach)
        times[attach].append(dt)
        print("batched step  %d VLP-16 streams  place database %-3s  %.1f us/step" % (ns, "on" if attach else "off", dt * 1e6))
    off, on = np.median(times[False]), np.median(times[True])
    print("batched step median: off %.1f us  on %.1f us  (%+.1f %%)" % (off * 1e6, on * 1e6, 100.0 * (on / off - 1.0)))


if part in ("vlp16", "all"):
    add_part("VLP-16", 1800)
if part in ("hdl64", "all"):
    add_part("HDL-64E", 2048)
if part in ("query", "all"):
    query_part()
if part in ("batch", "all"):
    batch_part()
