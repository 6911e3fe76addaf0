"""Place recognition in a prior map (loamx_place_add_views): a seeded synthetic hall from loam_velodyne_amd/synth.py (World.make_map:
ground, ceiling and pillar faces, --points samples inside +-(--extent) m, about a million voxels at --leaf) is added from the host;
the navigation grid of the whole hall gives --origins view origins (loamx_grid_view_origins, --sensor-height above the ground); then
the blocking call is timed for --rings x --azimuths rays of --range metres per view (CAST) and for the voxel list (VOXELS): the host
clock around the call, after a warm-up call, median [min, max] of --reps, into a fresh database each time.

Alternating with those runs, in the same process, the same views go through the single calls that existed before: per origin
DenseMap.raycast (ends up, 40-byte records back through pinned memory) and PlaceDB.add of the hit positions (up again); for VOXELS
one DenseMap.points() and PlaceDB.add of that cloud per origin, on --voxel-origins origins only (each add moves the whole map up).
The bytes both paths move over PCIe are counted from the sizes of what crosses.  The entries of both paths are compared, byte for
byte, on the first repetition.

Every step that uses the device runs under a time limit of its own (--step-timeout seconds, SIGALRM: the process ends there); one
process.  The kernel time comes from a run of its own under `rocprofv3 --kernel-trace --stats -- python scripts/time_place_views.py
--reps 2 --no-single`."""
import argparse, os, signal, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loam_velodyne_amd import loamx, synth

ap = argparse.ArgumentParser()
ap.add_argument("--extent", type=float, default=27.0)
ap.add_argument("--points", type=int, default=2_400_000)
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--origins", type=int, default=1024)
ap.add_argument("--rings", type=int, default=16)
ap.add_argument("--azimuths", type=int, default=360)
ap.add_argument("--range", type=float, default=30.0)
ap.add_argument("--sensor-height", type=float, default=1.8)
ap.add_argument("--cell-leaves", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--voxel-origins", type=int, default=16)
ap.add_argument("--step-timeout", type=int, default=120)
ap.add_argument("--no-single", action="store_true", help="the one-call path alone (for a profiled run)")
args = ap.parse_args()


class step:
    """a device step under its own time limit: the default action of SIGALRM ends the process"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        print("step: %s" % self.name, flush=True)
        signal.alarm(args.step_timeout)
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        signal.alarm(0)
        print("      %.2f s" % (time.perf_counter() - self.t0), flush=True)


def stat(times):
    t = np.array(times) * 1e3
    return "median %.1f ms [min %.1f, max %.1f] of %d" % (np.median(t), t.min(), t.max(), len(t))


w = synth.World(half_extent=args.extent + 5.0)
corner, surf = w.make_map(args.points, half_extent=args.extent)
pts = np.concatenate([corner, surf])
d = loamx.DenseMap(leaf=args.leaf, initial_slots=1 << 22)
with step("the map: %d points from the host" % len(pts)):
    for k in range(0, len(pts), 1 << 21):
        d.add(pts[k:k + (1 << 21)], (0.0, w.ground_y + args.sensor_height, 0.0))
    st = d.stats()
print("map: %d voxels in %d slots at leaf %.3f" % (st["voxels"], st["slots"], args.leaf), flush=True)

with step("the grid and the view origins"):
    cfg = loamx.grid_window(args.leaf, 0.0, 0.0, args.extent, cell_leaves=args.cell_leaves)
    cells = d.grid(cfg)
    for stride in (8, 6, 5, 4, 3, 2, 1):
        origins = loamx.grid_view_origins(cells, cfg, args.leaf, stride, 4, args.sensor_height)
        if len(origins) >= args.origins:
            break
    assert len(origins) >= args.origins, "the grid has only %d view origins" % len(origins)
    origins = np.ascontiguousarray(origins[:args.origins])
print("grid %d x %d cells of %.2f m, stride %d: %d view origins, y from %.2f to %.2f"
      % (cfg.nx, cfg.nz, args.leaf * args.cell_leaves, stride, len(origins), origins[:, 1].min(), origins[:, 1].max()), flush=True)

offsets = loamx.view_rays(args.azimuths, np.deg2rad(np.linspace(-15.0, 15.0, args.rings)), args.range)
n, n_rays = len(origins), len(offsets)
PLACE = dict(n_rings=20, n_sectors=60, max_range=args.range, height_offset=args.sensor_height + 0.5, exclude_recent=0, initial_entries=2048)


def entries(db, ids):
    return [db.descriptor(i)[0].tobytes() + db.descriptor(i)[1].tobytes() for i in ids]


def one_call(mode):
    db = loamx.PlaceDB(**PLACE)
    t0 = time.perf_counter()
    first, stats = db.add_views(d, origins, offsets if mode == "cast" else None)
    return time.perf_counter() - t0, db, stats


def single_cast():
    db = loamx.PlaceDB(**PLACE)
    up = down = hits = 0
    t0 = time.perf_counter()
    for o in origins:
        ends = np.zeros((n_rays, 4), np.float32)
        ends[:, :3] = o[None, :] + offsets
        rec, counts = d.raycast(ends, o)
        hit = rec["status"] >= loamx.RAY_HIT
        cloud = np.zeros((int(hit.sum()), 4), np.float32)
        cloud[:, 0], cloud[:, 1], cloud[:, 2] = rec["x"][hit], rec["y"][hit], rec["z"][hit]
        db.add(cloud, o)
        up += ends.nbytes + cloud.nbytes
        down += rec.nbytes + 40
        hits += len(cloud)
    db.descriptor(n - 1)    # (waits for the adds)
    return time.perf_counter() - t0, db, up, down, hits


def single_voxels(m):
    db = loamx.PlaceDB(**PLACE)
    t0 = time.perf_counter()
    cloud = d.points()
    for o in origins[:m]:
        db.add(cloud, o)
    db.descriptor(m - 1)
    return time.perf_counter() - t0, db, cloud.nbytes * m, cloud.nbytes


for mode in ("cast", "voxels"):
    with step("%s: warm-up call" % mode):
        _, db, stats = one_call(mode)
    print("%s: stats %s" % (mode, stats), flush=True)
    t_one, t_single = [], []
    for rep in range(args.reps):
        with step("%s: add_views, repetition %d" % (mode, rep)):
            t, db, stats = one_call(mode)
            t_one.append(t)
        if args.no_single:
            continue
        if mode == "cast":
            with step("cast: raycast + add per origin, repetition %d" % rep):
                t, sdb, up, down, hits = single_cast()
                t_single.append(t)
            if rep == 0:
                with step("cast: the entries of both paths"):
                    assert entries(db, range(n)) == entries(sdb, range(n)), "the two paths differ"
                print("cast: the %d entries of both paths are the same bytes" % n, flush=True)
        else:
            m = min(args.voxel_origins, n)
            with step("voxels: points() + add per origin, %d origins, repetition %d" % (m, rep)):
                t, sdb, up, down = single_voxels(m)
                t_single.append(t)
            if rep == 0:
                with step("voxels: the entries of both paths"):
                    assert entries(db, range(m)) == entries(sdb, range(m)), "the two paths differ"
                print("voxels: the first %d entries of both paths are the same bytes" % m, flush=True)
    one_up = (n + (n_rays if mode == "cast" else 0)) * 16
    print("%s, one call:     %d views, %s; PCIe %d bytes up, 48 down; stats %s" % (mode, n, stat(t_one), one_up, stats), flush=True)
    if t_single:
        if mode == "cast":
            print("cast, single calls: %d views, %s; PCIe %d bytes up, %d down; %d hits" % (n, stat(t_single), up, down, hits), flush=True)
            print("cast: ratio single / one call %.1f" % (np.median(t_single) / np.median(t_one)), flush=True)
        else:
            per = np.median(t_single) / m
            print("voxels, single calls: %d views, %s (%.1f ms per view: %.1f s for %d); PCIe %d bytes up, %d down"
                  % (m, stat(t_single), per * 1e3, per * n, n, up, down), flush=True)
            print("voxels: ratio single (scaled to %d views) / one call %.1f" % (n, per * n / np.median(t_one)), flush=True)
d.close()
